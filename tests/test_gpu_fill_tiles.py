"""The tile form of the sparse fill (star_fill_tile_kernel, hite_fill_tile.h) on the device: every case runs with the tile form and
then with the per-cell form (Context.fill_config), and both must equal the twin's alignment under the twin's column selection, byte
for byte.  The inputs: every label of star_layout_cases.py and its long group once more with the tile form on (more deferred blocks
than FILL_DEFER_CAP, rows beyond MSA_MAXR, dropped rows, padded rows, short and long launches), then the cases of
fill_tile_cases.py at the tile form's own limits (tile edges, the window slot, kept columns, output alignment, row counts, pads),
alone and in ONE call beside the long group -- where a stale layout word or LDS slot of a neighbour would show.  The limits come
from the build (Context.fill_tile_limits); every case asserts its precondition on the twin alone before it compares."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fill_tile_cases as FC  # noqa: E402
import star_layout_cases as SC  # noqa: E402
from test_gpu_star_layout import check  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import hite_amd

    c = hite_amd.Context(0)
    yield c
    c.fill_config(None)
    c.close()


def limits():
    """the tile form's constants from the build (the call copies constants: no GPU is touched)"""
    import hite_amd

    return hite_amd.Context.fill_tile_limits(_Lib())


class _Lib:
    """what Context.fill_tile_limits needs of a context"""

    def __init__(self):
        import hite_amd

        self.lib = hite_amd.load()

    def _check(self, rc, what):
        assert rc == 0, what


def both_forms(ctx, groups):
    """[(form, full alignments, sparse alignments)]: the tile form first, then the per-cell form"""
    out = []
    try:
        for tiles in (True, False):
            ctx.fill_config(tiles)
            out.append(("tiles" if tiles else "cells", ctx.star_msa(groups), ctx.star_msa(groups, sparse=True)))
    finally:
        ctx.fill_config(None)
    return out


def test_limits_are_exported(ctx):
    T, slot, rows, z = ctx.fill_tile_limits()
    assert (T, slot, rows, z) == tuple(limits()) and T % 64 == 0 and T >= 256 and 0 < slot and rows >= 1 and z >= 1


@pytest.mark.parametrize("label", SC.LABELS + ["long"])
def test_layout_cases_both_forms(ctx, label):
    if label == "long":
        gs = [SC.long_group()]
        exp = [SC.twin_full(gs[0])]
        assert SC.measured(SC.layout_profile(exp[0]), exp[0]) == SC.LONG_TWIN
    else:
        SC.check_precondition(label)
        gs, exp = SC.groups(label), [f for f, _ in SC.twin(label)]
    for form, full, sparse in both_forms(ctx, gs):
        for i, (g, f, s, e) in enumerate(zip(gs, full, sparse, exp)):
            check("%s[%d] %s" % (label, i, form), g, f, s, e)


KINDS = ("edge_", "ins_", "rows_tiles", "slot_", "keep_", "widths", "rows_R", "pads")


def _tile_labels(kind=""):
    return [x for x in FC.labels(limits()) if x.startswith(kind)]


def test_kinds_cover_every_case():
    assert sorted(x for k in KINDS for x in _tile_labels(k)) == sorted(_tile_labels())


@pytest.mark.parametrize("kind", KINDS)
def test_tile_limit_cases_both_forms(ctx, kind):
    for label in _tile_labels(kind):
        gs, ds = FC.case(limits(), label)            # (asserts the precondition on the twin)
        for form, full, sparse in both_forms(ctx, gs):
            for i, (g, f, s, d) in enumerate(zip(gs, full, sparse, ds)):
                check("%s[%d] %s" % (label, i, form), g, f, s, d["full"])


def test_every_kind_in_one_call(ctx):
    """a candidate of every kind beside the long group in ONE call of each form"""
    every, exp, names = [], [], []
    for label in _tile_labels():
        gs, ds = FC.case(limits(), label)
        for i, (g, d) in enumerate(zip(gs, ds)):
            every.append(g); exp.append(d["full"]); names.append("%s[%d]" % (label, i))
    long = SC.long_group()
    every.insert(len(every) // 2, long); exp.insert(len(exp) // 2, SC.twin_full(long)); names.insert(len(names) // 2, "long")
    assert max(len(w) for w in long) > SC.LONG_WIN
    for form, full, sparse in both_forms(ctx, every):
        for n, g, f, s, e in zip(names, every, full, sparse, exp):
            check("%s in one call, %s" % (n, form), g, f, s, e)
