"""The tables of the FMEA limit tests (tests/fmea_limit_cases.py), checked on the CPU alone: every builder's case reaches the limit it
is named for -- asserted with a plain python sweep next to the twin (oracle/hite_oracle_coarse.c: orc_fmea) -- and every check_* of
the module runs with the twin behind tests/oracle_ctx.py in the place of the device.  The device side of the same cases:
test_gpu_fmea_limits.py."""
import pytest

import fmea_limit_cases as FC
from conftest import load_golden
from oracle_ctx import OracleCtx


@pytest.fixture(scope="module")
def twin_chain():
    return OracleCtx().fmea_chain


@pytest.mark.parametrize("nseg", FC.RANK_NSEG)
def test_rank_case_reaches_its_limit(nseg, twin_chain):
    cl = FC.check_ranks_case(nseg)
    print("ranks: nseg %(segments)d, np2 %(np2)d, %(queries)d queries (top rank %(top_rank)d), %(subject_only)d subject-only and "
          "%(unused)d unused ids, %(n_rows)d rows, %(slots)d slots" % cl)
    FC.check_ranks(twin_chain, nseg)


def test_sweep_cases_reach_their_rounds(twin_chain):
    for label, cl in FC.check_sweep_cases():
        print("%s: closing member %s places back, round %s" % (label, cl["members_back"], cl["round"]))
    FC.check_sweep(twin_chain)


def test_filter_case_goes_past_the_stride(twin_chain):
    for q, fig in enumerate(FC.check_filter_case()["queries"]):
        print("filter query %d: %d candidates, %d kept, sorted positions %s" % (q, fig["candidates"], fig["kept"], fig["position"]))
    FC.check_filter(twin_chain)


def test_limit_cases_and_key_bounds(twin_chain):
    print("first values pack_key refuses: %s" % FC.check_key_bounds())
    FC.check_limit_cases()
    FC.check_limits(twin_chain)
    for label, inside, _at in FC.guards():                 # (the twin has no packing limit: only the device side refuses a table)
        FC.compare(twin_chain, inside, label)


def test_order_cases_reach_the_shortcut(twin_chain):
    print("orders: %s" % FC.check_order_cases())
    FC.check_orders(twin_chain)


def test_block_sort_model_sorts():
    """bitonic_order, the model of the kernels' block sort behind the rank cases' claim, is a stable sort by (key, id)"""
    import numpy as np

    rng = np.random.default_rng(3)
    for n in (1, 2, 3, 17, 256, 257, 1000):
        keys = rng.integers(0, 50, size=n)
        keys[rng.integers(0, n, size=n // 3)] = 0x7FFFFFFF
        assert FC.bitonic_order(keys).tolist() == np.argsort(keys, kind="stable").tolist()


def test_fixture_is_todays_tables(twin_chain):
    """tests/golden/fmea_limits.json.gz (the reference's own answers on the small cases) against the builders and the twin"""
    FC.check_fixture(twin_chain, load_golden("fmea_limits"))
