"""The two forms of the wide fall-back's traceback (hite_amd/csrc/hite_align.hip: align_wide_tb_runs_kernel, up to 64 path steps per
trip, and align_wide_tb_kernel, a column per step; the switch Context.wide_tb_runs) on the pairs of tests/wide_walk_cases.py, each
of which test_wide_walk_cases.py proves on the CPU to end in the fall-back with the runs it is named for.  Both forms, in the same
process, through align_check.check_pairs at cap 8: ops, info and the hite_align_stats counters == the twin byte for byte, the dropped
pairs dropped by both; then more than 64 fall-back pairs in one call."""
import pytest

import wide_walk_cases as WC
from align_check import FALLBACK, check_pairs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import hite_amd

    c = hite_amd.Context(0)
    yield c
    c.wide_tb_runs(None)
    c.close()


def both_forms(ctx, cases):
    res = []
    for mode in (0, 1):
        ctx.wide_tb_runs(mode)
        try:
            res.append(check_pairs(ctx, [(c.a, c.b) for c in cases], WC.CAP))
        finally:
            ctx.wide_tb_runs(None)
    for r in res:
        assert len(r.classes) == len(cases)
        for c, cls in zip(cases, r.classes):
            assert WC.is_class(c, cls) and cls[0] == FALLBACK, (c.name, cls)
        assert r.n_drop == sum(c.dropped for c in cases)
    assert res[0] == res[1]
    return res[1]


def test_the_table_through_both_forms(ctx):
    cases = WC.table()
    r = both_forms(ctx, cases)
    assert r.n_drop == 2


def test_more_than_64_pairs_in_one_call(ctx):
    cases = WC.many()
    assert len(cases) > 64
    r = both_forms(ctx, cases)
    assert r.n_drop == 0


def test_the_switch_takes_only_its_three_values(ctx):
    for bad in (-2, 2):
        assert ctx.lib.hite_wide_tb_runs_ctx(ctx.h, bad) != 0
    for ok in (-1, 0, 1):
        assert ctx.lib.hite_wide_tb_runs_ctx(ctx.h, ok) == 0
    ctx.wide_tb_runs(None)
