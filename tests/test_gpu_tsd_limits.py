"""The two kernels of hite_amd/csrc/hite_tsd.hip on the device at the limits of their own code, against the CPU twins
(oracle/hite_oracle_coarse.c: orc_tir_kmer, oracle/hite_oracle.c: orc_search_polyA_TSD) on the sequences of tests/tsd_limit_cases.py
-- the same check_* functions that test_tsd_limit_cases.py runs with the twins in the device's place, where every case is also
shown to reach its limit.  Exact integer equality everywhere.
   * hite_tsd_kmer: flanks 0 .. 63 (windows of 1 .. 127 of the 128 LDS slots, one and two passes of 64 lanes; 65 and 67 slots), bodies
     of 99 / 100 / 101 bases, candidates shorter than two flanks and no longer than one; more than 100 records before the cut with
     ties in distance across it, exactly 100 and 101; k-mers that differ only in WHICH byte outside ACGT they hold; one batch in
     three orders; flank 64 / -1 are errors;
   * hite_nonltr_prep: all 65 536 pairs of 8-mers over two letters and the single-edit families of k = 9 .. 20 through np_near1; two
     equal poly runs; the wrapped 5' window whose first match is at index 64 or more (second round of 64 lanes); 14 094 sequences
     of 0 .. 260 bases at flanks 0 .. 100 and win5 0 .. 25; batches of 1, 3, 4, 5, 257; win5 26 / -1 and flank -1 are errors."""
import pytest

import tsd_limit_cases as TC
from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import hite_amd

    c = hite_amd.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("flank", TC.KMER_FLANKS)
def test_kmer_flanks(ctx, flank):
    TC.check_flanks(ctx.tsd_kmer, flank)


def test_kmer_cut_at_100(ctx):
    TC.check_cut(ctx.tsd_kmer)


def test_kmer_alphabet(ctx):
    TC.check_alphabet(ctx.tsd_kmer)


def test_kmer_batch_independence(ctx):
    TC.check_batch_independence(ctx.tsd_kmer)


def test_kmer_guards(ctx):
    TC.check_kmer_guards(ctx.tsd_kmer)


def test_nonltr_closed_form_all_8mer_pairs(ctx):
    TC.check_exhaustive(ctx.nonltr_prep)


def test_nonltr_closed_form_edit_families(ctx):
    TC.check_family(ctx.nonltr_prep)


def test_nonltr_equal_runs(ctx):
    TC.check_ties(ctx.nonltr_prep)


def test_nonltr_wrapped_window(ctx):
    TC.check_wrapped(ctx.nonltr_prep)


def test_nonltr_short_sequences(ctx):
    TC.check_grid(ctx.nonltr_prep)


def test_nonltr_block_tail(ctx):
    TC.check_batches(ctx.nonltr_prep)


def test_nonltr_guards(ctx):
    TC.check_nonltr_guards(ctx.nonltr_prep)


def test_reference_fixture(ctx):
    """the reference's own answers on a thinned set of the small cases (tests/golden/tsd_limits.json.gz)"""
    TC.check_fixture(ctx.tsd_kmer, ctx.nonltr_prep, load_golden("tsd_limits"))
