"""The layout / fill kernels of the star alignment (hite_msa.hip, hite_fill.h) at their fixed capacities: HIP == the twin
(oracle/hite_oracle_msa.c) byte for byte, the full form (star_layout_kernel / star_fill_kernel) and the fused sparse form
(star_layout_sparse_kernel / star_fill_sparse_kernel<4> and <8>), with dropped rows (msa_compact_rows_kernel) and padded rows
(ops_pad_fix_kernel).  The inputs are those of tests/star_layout_cases.py, whose limits test_star_layout_cases.py checks on the CPU
and this file asserts again before it compares: more kept-block positions in a layout round than LAY_KW_LIST (255 .. 258 and beyond,
in round 0 and in round 1), more deferred blocks in a fill workgroup than FILL_DEFER_CAP, rows beyond MSA_MAXR and around the 64-row
trips of the k-th-largest loop, centres that end beside a round of either layout kernel with and without an extra last column,
rows dropped beyond row 128 and down to the centre alone, pads that end on the 64-position trips of the pad fix.

Every group runs twice: in a call of its own (or with its own small family) -- short windows: star_fill_sparse_kernel<4> -- and in
ONE call with all others and a group with a window above 1536 bases, which makes the whole launch run <8>.  Nothing here is a
tolerance: the sparse form is the twin's alignment under the twin's column selection, itself checked against the plain rule."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle_lib as O  # noqa: E402
import star_layout_cases as SC  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import hite_amd

    c = hite_amd.Context(0)
    yield c
    c.close()


def where(got, exp):
    d = np.argwhere(got != exp)
    return "%d bytes differ, first (row, column) %s" % (len(d), d[:5].tolist())


def check(what, group, got_full, got_sparse, exp_full):
    """full form == twin; sparse form == twin under the twin's column selection (== the plain rule); shapes and row counts too"""
    assert got_full is not None, what + ": no full alignment"
    assert got_full.shape == exp_full.shape, (what, "full", got_full.shape, exp_full.shape, len(group))
    assert np.array_equal(got_full, exp_full), (what, "full", where(got_full, exp_full))
    keep = O.sparse_cols(exp_full)
    assert np.array_equal(keep, SC.plain_sparse_keep(exp_full)), what
    exp = np.ascontiguousarray(exp_full[:, keep.astype(bool)])
    assert got_sparse is not None, what + ": no sparse alignment"
    assert got_sparse.shape == exp.shape, (what, "sparse", got_sparse.shape, exp.shape, len(group))
    assert np.array_equal(got_sparse, exp), (what, "sparse", where(got_sparse, exp))


@pytest.fixture(scope="module")
def one_launch(ctx):
    """every group of every case and the long group in ONE call of each form"""
    every, first = [], {}
    for label in SC.LABELS:
        first[label] = len(every)
        every.extend(SC.groups(label))
    first["long"] = len(every)
    every.append(SC.long_group())
    assert max(len(w) for w in every[-1]) > SC.LONG_WIN
    return first, ctx.star_msa(every), ctx.star_msa(every, sparse=True)


@pytest.mark.parametrize("label", SC.LABELS)
def test_case_alone(ctx, label):
    SC.check_precondition(label)
    gs = SC.groups(label)
    full, sparse = ctx.star_msa(gs), ctx.star_msa(gs, sparse=True)
    assert len(full) == len(sparse) == len(gs)
    for i, (g, f, s, (exp_full, _)) in enumerate(zip(gs, full, sparse, SC.twin(label))):
        check("%s[%d] alone" % (label, i), g, f, s, exp_full)


@pytest.mark.parametrize("label", SC.LABELS)
def test_case_in_one_long_launch(one_launch, label):
    """the same groups beside all others and a window above 1536 bases: the eight-positions-per-thread fill, candidates that are
    compacted beside candidates that are not -- the same bytes as alone (both equal the twin's)"""
    SC.check_precondition(label)
    first, full, sparse = one_launch
    for i, (g, (exp_full, _)) in enumerate(zip(SC.groups(label), SC.twin(label))):
        check("%s[%d] in one launch" % (label, i), g, full[first[label] + i], sparse[first[label] + i], exp_full)


def test_long_group_of_the_one_launch(ctx, one_launch):
    first, full, sparse = one_launch
    g = SC.long_group()
    exp_full = SC.twin_full(g)
    assert SC.measured(SC.layout_profile(exp_full), exp_full) == SC.LONG_TWIN
    check("long in one launch", g, full[first["long"]], sparse[first["long"]], exp_full)
    alone_full, alone_sparse = ctx.star_msa([g])[0], ctx.star_msa([g], sparse=True)[0]
    check("long alone", g, alone_full, alone_sparse, exp_full)
