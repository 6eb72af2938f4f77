"""FMEA on the device (hite_fmea_chain, hite_amd/csrc/hite_fmea.hip) at the limits of its own kernels, against the CPU twin
(oracle/hite_oracle_coarse.c: orc_fmea) on the tables of tests/fmea_limit_cases.py -- the same check_* functions that
test_fmea_limit_cases.py runs with the twin in the device's place, where every table is also shown to reach its limit:
   * segment ranks: 1 .. 4096 segments whose ids are not their ranks (block sort over up to 4096 slots, the 12 bits of query rank
     in the candidate sort key, more slots than one pass of the cluster sweep's grid); 4097 segments are an error;
   * cluster sweep: the only member that takes an HSP in sits 64 .. 301 places back (rounds 1, 2, 3 and 5 of 64 lanes);
   * containment filter: 700 candidates per query, pairs on the 95 % threshold on either side of the 256-wide stride;
   * lengths 79 / 80 / 81 and max_len - 1 / max_len / max_len + 1, ends = 0, 1, 9 mod 10, 5 000 chains on one rounded interval,
     one chain, and the bounds of the 64-bit key packing: an error for the whole table, never a wrong interval;
   * one multiset of HSPs shuffled and grouped, with exact self hits where the first-appearance kernel's shortcut looks."""
import os
import subprocess
import sys

import pytest

import fmea_limit_cases as FC
from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import hite_amd

    c = hite_amd.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("nseg", FC.RANK_NSEG)
def test_ranks(ctx, nseg):
    FC.check_ranks(ctx.fmea_chain, nseg)


def test_too_many_segments_are_an_error(ctx):
    FC.check_too_many_segments(ctx.fmea_chain)


def test_sweep_rounds(ctx):
    FC.check_sweep(ctx.fmea_chain)


def test_containment_filter(ctx):
    FC.check_filter(ctx.fmea_chain)


def test_length_and_key_limits(ctx):
    FC.check_limits(ctx.fmea_chain)


def test_key_packing_bounds_are_errors(ctx):
    FC.check_guards(ctx.fmea_chain)


def test_table_orders(ctx):
    FC.check_orders(ctx.fmea_chain)


def test_reference_fixture(ctx):
    """the reference's own answers on the small cases (tests/golden/fmea_limits.json.gz)"""
    FC.check_fixture(ctx.fmea_chain, load_golden("fmea_limits"))


def test_limits_with_the_wide_radix_sort():
    """the rank cases up to 1000 segments, the sweep rounds and the containment filter once more with the 10-bit staged radix
    scatter forced onto their small sorts (as test_gpu_parity.py::test_wide_radix_sort_on_small_inputs does), in a fresh process"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HITE_SORT_WIDE_MIN="2")
    rc = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k",
                         "(test_ranks and not 409) or test_sweep_rounds or test_containment_filter"],
                        env=env, capture_output=True, text=True, cwd=root, timeout=300)
    assert rc.returncode == 0, rc.stdout[-3000:] + rc.stderr[-2000:]
    assert "9 passed" in rc.stdout, rc.stdout[-1000:]
