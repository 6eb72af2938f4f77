"""CPU-only: the twin of hite_pair_hsps (tests/pairhsp_twin.py, tests/pairhsp_twin.c) against itself and against what does not
depend on it -- the two forms agree on every small case, the closed forms of tests/pairhsp_cases.py hold, and where the best path
provably stays inside one band the banded result is the unbanded, quadratic local alignment."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pairhsp_cases as PC  # noqa: E402
import pairhsp_twin as T  # noqa: E402


def test_the_two_forms_agree_on_every_small_case():
    cases = PC.small_cases()
    assert len(cases) > 80
    got_c = PC.run(T.pair_hsps, cases)
    n_hsp = 0
    for (label, q, s, dm), c in zip(cases, got_c):
        assert T.pair_hsps_one(q, s, dm) == c, label
        n_hsp += len(c)
    assert n_hsp > 60


def test_steps_of_the_two_forms_on_sub_rectangles():
    rng = np.random.default_rng(3)
    for _ in range(40):
        m, n = int(rng.integers(30, 120)), int(rng.integers(30, 120))
        a = PC.dna(rng, m)
        b = (PC.mutate(rng, a, 0.1) + PC.dna(rng, n))[:n]
        dlo = int(rng.integers(-40, 10))
        dhi = dlo + int(rng.integers(0, 192))
        r0, c0 = int(rng.integers(1, m + 1)), int(rng.integers(1, n + 1))
        r1, c1 = int(rng.integers(r0, m + 1)), int(rng.integers(c0, n + 1))
        assert T.align(T.codes(a), T.codes(b), dlo, dhi, r0, r1, c0, c1) == T.align_c(a, b, dlo, dhi, r0, r1, c0, c1)


def test_closed_forms():
    forms = PC.closed_forms()
    got = PC.run(T.pair_hsps, [f[:4] for f in forms])
    for (label, q, s, dm, recs), g in zip(forms, got):
        assert g == recs, (label, g)
        if len(q) * len(s) <= 100000:
            assert T.pair_hsps_one(q, s, dm) == recs, label


def test_refused_pairs_and_the_capacity():
    seqs, pairs, ok = PC.refused()
    got = T.pair_hsps(seqs, pairs)
    assert [g is not None for g in got] == ok
    assert got[0] == [(1, 100, 1, 100, 200, 100, 100)] and got[3] == []
    assert T.pair_hsps(seqs, []) == []


def test_banded_equals_unbanded_where_the_path_stays_in_the_band():
    """m, n <= 150.  The unbanded best cell has a path of g = 2 * columns - rows - columns-of-S gap steps, and a gap step moves the
    path by one diagonal: it stays within g diagonals of its two ends.  Where that range lies inside the band of the first window
    (and the path is the only one of its score there), the band's first HSP must be that cell."""
    rng = np.random.default_rng(5)
    checked = 0
    for k in range(120):
        m, n = int(rng.integers(60, 151)), int(rng.integers(60, 151))
        a = PC.dna(rng, m)
        b = (PC.dna(rng, int(rng.integers(0, 30))) + PC.mutate(rng, a[int(rng.integers(0, 20)):], 0.08, indel=0.3) + PC.dna(rng, n))[:n]
        qc, sc = T.codes(a), T.codes(b)
        full = T.align(qc, sc, -10 ** 6, 10 ** 6, 1, m, 1, n)
        wins = T.windows(T.votes(qc, sc))
        if full is None or full[4] < T.MIN_SCORE or not wins:
            continue
        dlo, dhi = T.band_of(wins[0], m)
        gaps = 2 * full[6] - (full[1] - full[0] + 1) - (full[3] - full[2] + 1)
        ds, de = full[2] - full[0], full[3] - full[1]
        if dlo <= min(ds, de) - gaps and max(ds, de) + gaps <= dhi:
            assert T.align(qc, sc, dlo, dhi, 1, m, 1, n) == full, (k, a, b)
            assert T.align_c(a, b, dlo, dhi, 1, m, 1, n) == full, (k, a, b)
            assert T.pair_hsps_one(a, b)[0] == full, (k, a, b)
            checked += 1
    assert checked >= 60, checked
