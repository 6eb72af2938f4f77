"""The sequences of the TSD limit tests (tests/tsd_limit_cases.py), checked on the CPU alone: every builder's cases reach the limit
they are named for -- asserted with the twins (oracle/hite_oracle_coarse.c: orc_tir_kmer, oracle/hite_oracle.c: orc_search_polyA_TSD)
and with the plain python statement of the k-mer rule before its cut -- and every check_* of the module runs with the twins behind
tests/oracle_ctx.py in the place of the device.  The device side of the same cases: test_gpu_tsd_limits.py."""
import pytest

import tsd_limit_cases as TC
from conftest import load_golden
from oracle_ctx import OracleCtx


@pytest.fixture(scope="module")
def twin():
    return OracleCtx()


def test_flank_cases_reach_their_windows(twin):
    fig = TC.check_flank_cases()
    print("k-mer flank cases: %(cases)d, %(with records)d with records, %(at 100)d with 100, plant changes %(plant matters)d, "
          "%(past the first pass)d with a record from window slot 64 or later, %(empty by length)d no longer than a flank" % fig)
    for f in TC.KMER_FLANKS:
        TC.check_flanks(twin.tsd_kmer, f)


def test_cut_cases_reach_the_cut(twin):
    for label, n, tie, k_alone in TC.check_cut_cases():
        print("%s: %d records before the cut, records 100 and 101 at one distance: %s, kept pairs that differ in k alone: %d"
              % (label, n, tie, k_alone))
    TC.check_cut(twin.tsd_kmer)


def test_alphabet_cases_tell_bytes_apart(twin):
    print("k-mer alphabet cases: %s" % TC.check_alphabet_cases())
    TC.check_alphabet(twin.tsd_kmer)


def test_kmer_batch_and_guards(twin):
    TC.check_batch_independence(twin.tsd_kmer)
    TC.check_kmer_guards(twin.tsd_kmer)


def test_uncut_rule_is_the_twin_below_the_cut():
    """kmer_records_uncut, the statement behind the cut cases' claim, against the twin on the committed k-mer fixtures' inputs"""
    n = 0
    for case in load_golden("tir_kmer")[::4] + load_golden("tir_kmer_edge")[::2]:
        f, plant, s = case["flank"], case["plant"], case["seq"]
        full = TC.kmer_records_uncut(s, f, plant)
        assert TC.kmer_expected([s], f, plant)[0] == full[:TC.TOP]
        n += len(full) > TC.TOP
    print("fixture inputs with more than 100 records before the cut: %d" % n)


def test_exhaustive_pairs_all_have_a_direction(twin):
    fig = TC.check_exhaustive_cases()
    print("closed form: %s (pairs, found)" % fig)
    TC.check_exhaustive(twin.nonltr_prep)


def test_edit_families(twin):
    for k, (n, at_k, below, none) in TC.check_family_cases().items():
        print("edit family k = %d: %d cases, %d found with k, %d with a shorter TSD, %d not found" % (k, n, at_k, below, none))
    TC.check_family(twin.nonltr_prep)


def test_equal_runs(twin):
    print("two equal runs: %d cases" % TC.check_tie_cases())
    TC.check_ties(twin.nonltr_prep)


def test_wrapped_window_reaches_the_second_round(twin):
    print("wrapped 5' window: %s" % TC.check_wrapped_cases())
    TC.check_wrapped(twin.nonltr_prep)


def test_short_sequences_and_parameters(twin):
    print("short sequences: %s" % TC.check_grid_cases())
    TC.check_grid(twin.nonltr_prep)


def test_nonltr_batches_and_guards(twin):
    print("block tail pool: %s" % TC.check_batch_cases())
    TC.check_batches(twin.nonltr_prep)
    TC.check_nonltr_guards(twin.nonltr_prep)


def test_closed_form_model():
    """near1_model, the statement of np_near1 behind the exhaustive case's claim, against the twin's find_near_matches on pairs the
    sequences do not hold: 8-mers over three letters and 11-mers one or two edits apart"""
    import ctypes as C

    import numpy as np

    import oracle_lib as O

    rng = np.random.default_rng(9)
    pairs = [(TC.rand_seq(rng, 8, "ACT"), TC.rand_seq(rng, 8, "ACT")) for _ in range(2000)]
    p = TC.rand_seq(rng, 11)
    pairs += [(p, t) for t in TC.edit_family(rng, p)]
    out = (C.c_int * 4)()
    hits = 0
    for p, t in pairs:
        a, b = O._u8(p), O._u8(t)
        n = O.lib().orc_find_near_matches(O._ptr(a, O.u8p), len(p), O._ptr(b, O.u8p), len(t), 1, out)
        assert (n > 0) == TC.near1_model(p, t), (p, t)
        hits += n > 0
    assert 100 < hits < len(pairs) - 100


def test_fixture_is_todays_cases(twin):
    """tests/golden/tsd_limits.json.gz (the reference's own answers on a thinned set of the small cases) against the builders and the twins"""
    TC.check_fixture(twin.tsd_kmer, twin.nonltr_prep, load_golden("tsd_limits"))
