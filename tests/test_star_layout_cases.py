"""The cases of the star alignment's layout / fill edge tests (tests/star_layout_cases.py), checked on the CPU alone: every case reaches
the limit it exists for -- measured on the TWIN's full alignment (oracle/hite_oracle_msa.c) with plain numpy and asserted with the
recorded figure -- the twin's alignment holds every row's window, and the twin's sparse-column selection is the rule itself.  The device
side of the same cases: test_gpu_star_layout.py."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle_lib as O  # noqa: E402
import star_layout_cases as SC  # noqa: E402


def test_layout_profile_on_a_hand_made_alignment():
    """layout_profile / plain_sparse_keep / defer_items against figures worked out by hand"""
    full = O.msa_array(["-A--CG-T--",
                        "TAGGC--TAC",
                        "-AG-CGATC-",
                        "-A--CG-T--",
                        "-AG-C--TA-"])
    p = SC.layout_profile(full)
    assert (p["m"], p["R"], p["h"]) == (4, 5, 3)
    assert p["ins"].tolist() == [[1, 2, 0, 0, 2], [0, 1, 0, 1, 1], [0, 0, 0, 0, 0], [0, 1, 0, 0, 1]]
    assert p["count"].tolist() == [1, 3, 0, 1, 3] and p["widest"].tolist() == [1, 2, 0, 1, 2] and p["kth"].tolist() == [0, 1, 0, 0, 1]
    assert p["kept"].tolist() == [1, 4] and p["per_round"] == [2] and p["extra_last"] and (p["last_widest"], p["last_kth"]) == (2, 1)
    assert SC.defer_items(p) == 2 * 3                          # rows 0 and 4 of workgroup 0; positions 0 (first column), 1 and 4
    assert SC.plain_sparse_keep(full).tolist() == [1, 1, 1, 0, 1, 1, 0, 1, 1, 1]
    assert SC.plain_sparse_keep(full).tolist() == O.sparse_cols(full).tolist()
    assert SC.lead_gap_positions(full, 3) == 0 and SC.trail_gap_positions(full, 1) == 0
    one = O.msa_array(["ACGT"])
    p1 = SC.layout_profile(one)
    assert (p1["m"], p1["per_round"], p1["extra_last"], SC.defer_items(p1)) == (4, [0], False, 0)


def test_the_table_names_every_case():
    assert sorted(SC.TWIN) == sorted(SC.LABELS)
    assert {"kwlist_%d" % n for n in (255, 256, 257, 258)} <= set(SC.LABELS)
    assert {"rows_R%d" % R for R in (63, 64, 65, 66, 127, 128, 129, 130, 200)} <= set(SC.LABELS)
    assert {"edge_m%d" % m for m in (1022, 1023, 1024, 1025, 1027, 2047, 2048, 2049, 255, 256, 257)} <= set(SC.LABELS)
    assert max(len(w) for w in SC.long_group()) > SC.LONG_WIN
    full = SC.twin_full(SC.long_group())
    assert SC.measured(SC.layout_profile(full), full) == SC.LONG_TWIN
    assert [l for l in SC.LABELS if max(len(w) for g in SC.groups(l) for w in g) > SC.LONG_WIN] == SC.OWN_CALL_LONG
    assert {R % 4 for R in SC.ROWS_R} == {0, 1, 2, 3}


@pytest.mark.parametrize("label", SC.LABELS)
def test_case_reaches_its_limit(label):
    SC.check_precondition(label)


@pytest.mark.parametrize("label", SC.LABELS)
def test_twin_alignment_holds_the_windows_and_the_plain_rule(label):
    for g, (full, prof) in zip(SC.groups(label), SC.twin(label)):
        if full.shape[0] == len(g):              # (a dropped row leaves the alignment: "dropped" checks its rows below)
            for r, w in enumerate(g):
                assert SC.ungapped(full[r]) == SC.strip_pads(w).encode(), (label, r)
        assert np.array_equal(SC.plain_sparse_keep(full), O.sparse_cols(full)), label
        assert prof["m"] == len(g[0]) and SC.ungapped(full[0]) == g[0].encode()


def test_dropped_rows_are_the_short_ones():
    big, whole, alone = SC.groups("dropped")
    (fb, _), (fw, _), (fa, _) = SC.twin("dropped")
    left = [w for r, w in enumerate(big) if r not in (1, 64, 129, 139)]
    assert fb.shape[0] == 136 and [SC.ungapped(row) for row in fb] == [w.encode() for w in left]
    assert all(2 * len(big[r]) < len(big[0]) for r in (1, 64, 129, 139)) and all(2 * len(w) < len(alone[0]) for w in alone[1:])
    assert fa.shape == (1, len(alone[0])) and bytes(fa[0]) == alone[0].encode()


@pytest.mark.parametrize("label", ["tiny", "kwlist_256", "edge_m257", "pads", "defer_R73"])
def test_one_run_twin_is_the_suites_twin(label):
    """twin_full (one run of the twin) == oracle_lib.star_msa (the form every other test of the stage compares with)"""
    for g, (full, _) in zip(SC.groups(label), SC.twin(label)):
        exp, kept = O.star_msa(g, rows=True)
        assert kept == full.shape[0] and np.array_equal(full, exp)
