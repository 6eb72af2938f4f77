"""CPU-only: the twin of the pairwise identity (tests/identity_twin.c, the definition in include/hite_gpu.h) against what the
definition says in the plainest terms: an exhaustive enumeration of all alignments, the Levenshtein distance, a dense band-limited
dynamic programme in Python, and tie cases with their values written out."""
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import identity_cases as IC  # noqa: E402
import identity_twin as T  # noqa: E402


def _match(x, y):
    return x == y and x in "ACGT"


def enumerate_all(a, b):
    """the lexicographic optimum over EVERY alignment of a and b (no band, no memo: each path is walked)"""
    m, n = len(a), len(b)

    def walk(i, j):
        if i == m and j == n:
            return (0, 0)
        best = None
        if i < m and j < n:
            c, g = walk(i + 1, j + 1)
            r = (c, g - 1) if _match(a[i], b[j]) else (c + 1, g)
            best = r
        if i < m:
            c, g = walk(i + 1, j)
            r = (c + 1, g)
            best = r if best is None or r < best else best
        if j < n:
            c, g = walk(i, j + 1)
            r = (c + 1, g)
            best = r if best is None or r < best else best
        return best

    c, g = walk(0, 0)
    return c, -g


def dense_band(a, b, band):
    """(cost, matches) by a dense matrix of (cost, -matches) tuples restricted to the band, or (-1, 0)"""
    m, n = len(a), len(b)
    lo, hi = min(0, n - m) - band, max(0, n - m) + band
    D = [[None] * (n + 1) for _ in range(m + 1)]
    for i in range(m + 1):
        for j in range(n + 1):
            if not lo <= j - i <= hi:
                continue
            c = [(0, 0)] if i == 0 and j == 0 else []
            if i and j and D[i - 1][j - 1] is not None:
                p = D[i - 1][j - 1]
                c.append((p[0], p[1] - 1) if _match(a[i - 1], b[j - 1]) else (p[0] + 1, p[1]))
            if i and D[i - 1][j] is not None:
                c.append((D[i - 1][j][0] + 1, D[i - 1][j][1]))
            if j and D[i][j - 1] is not None:
                c.append((D[i][j - 1][0] + 1, D[i][j - 1][1]))
            D[i][j] = min(c) if c else None
    return (D[m][n][0], -D[m][n][1]) if D[m][n] is not None else (-1, 0)


def levenshtein(a, b):
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = min(prev[j - 1] + (0 if _match(a[i - 1], b[j - 1]) else 1), prev[j] + 1, cur[j - 1] + 1)
        prev = cur
    return prev[len(b)]


def _fold(s):
    return "".join(c if c in "ACGT" else "N" for c in s.decode("latin-1").upper())


def test_tiny_sequences_equal_exhaustive_enumeration():
    """every pair of: all sequences of at most 3 bases over ACGN, and 25 random ones of 4 and 5 bases"""
    rng = np.random.default_rng(1)
    seqs = ["".join(t) for k in range(4) for t in itertools.product("ACGN", repeat=k)]
    seqs += ["".join(rng.choice(list("ACGN"), size=int(rng.integers(4, 6)))) for _ in range(25)]
    assert len(seqs) == 85 + 25 and max(len(s) for s in seqs) == 5
    pairs = [(a, 0, len(seqs[a]), b, 0, len(seqs[b]), 0) for a in range(len(seqs)) for b in range(len(seqs))]
    got = T.pair_identity(seqs, pairs, band=5, max_width=0)          # |n - m| + 11 diagonals: the whole matrix
    memo = {}
    for (a, _0, _1, b, _2, _3, _4), g in zip(pairs, got.tolist()):
        key = (seqs[a], seqs[b])
        if key not in memo:
            memo[key] = enumerate_all(*key)
        assert tuple(g) == memo[key], (key, g, memo[key])


def test_random_pairs_full_band_is_levenshtein_and_narrow_band_is_dense_dp():
    rng = np.random.default_rng(2)
    n_limited = 0
    for case in range(40):
        a = IC.rand_seq(rng, int(rng.integers(0, 201)))
        b = IC.mutate(rng, a, float(rng.choice([0, 0.05, 0.3])), float(rng.choice([0, 0.05, 0.2])))[:200] if case % 4 else IC.rand_seq(rng, int(rng.integers(0, 201)))
        if case % 5 == 0 and len(b) > 3:
            b = b[:2] + b"N" + b[3:]
        fa, fb = _fold(a), _fold(b)
        cost, matches = T.one(a, b, band=200)
        assert cost == levenshtein(fa, fb), (case, cost)
        assert (cost, matches) == dense_band(fa, fb, 200), case
        for band in (0, 1, 3, 10):
            exp = dense_band(fa, fb, band)
            assert T.one(a, b, band=band) == exp, (case, band)
            n_limited += exp[0] > cost
    assert n_limited > 10          # narrow bands that changed the result


def test_strand_and_case_folding():
    a, b = b"ACGGTNAC", b"gtnaccgt"
    assert T.one(a, b, band=8, strand=1) == dense_band("ACGGTNAC", "ACGGTNAC", 8) == (1, 7)       # N against N is a mismatch
    assert T.one(a, b, band=8, strand=0) == dense_band("ACGGTNAC", "GTNACCGT", 8)


# (a, b, band) -> (cost, matches), worked out by hand from the definition
TIES = [
    ("ACACAC", "CACACA", 0, (6, 0)),       # one diagonal: six mismatches
    ("ACACAC", "CACACA", 1, (2, 5)),       # delete the first A, insert the last: five matches
    ("AAC", "ACA", 2, (2, 2)),             # two substitutions (one match) tie with delete + insert (two matches): the latter counts
    ("AAC", "ACA", 0, (2, 1)),             # ... which the band of one diagonal forbids
    ("AAAAA", "AAAA", 0, (1, 4)),          # a homopolymer with one deletion: wherever it is placed
    ("AAAA", "AAAAA", 3, (1, 4)),
    ("AAAATTTT", "AAATTTTT", 1, (1, 7)),   # one substitution beats delete + insert on cost
    ("ACGT", "CGTA", 1, (2, 3)),
    ("ACGT", "TGCA", 4, (4, 1)),            # four substitutions (no match) tie with delete A, C>T, G=G, T>C, insert A (one match)
    ("ACGT", "TGCA", 0, (4, 0)),            # ... which needs a second diagonal
    ("NNNN", "NNNN", 2, (4, 0)),
    ("", "", 0, (0, 0)),
    ("", "ACG", 0, (3, 0)),
    ("ACG", "", 5, (3, 0)),
]


def test_tie_cases_written_out():
    for a, b, band, exp in TIES:
        assert T.one(a.encode(), b.encode(), band=band) == exp, (a, b, band)
        assert dense_band(a, b, band) == exp, (a, b, band)
        if band >= max(len(a), len(b)):
            assert enumerate_all(a, b) == exp, (a, b)


def test_limits_and_refused_pairs():
    for label, seqs, pairs, band in IC.invalid():
        got = T.pair_identity(seqs, pairs, band).tolist()
        assert got == [[1, 9], [-1, 0], [1, 9], [-1, 0], [-1, 0], [1, 9], [-1, 0], [-1, 0], [-1, 0], [1, 9]], label
    a = b"A" * 40
    assert T.one(a, a + b"C" * (T.MAX_WIDTH - 1), band=0, max_width=T.MAX_WIDTH) == (T.MAX_WIDTH - 1, 40)
    assert T.one(a, a + b"C" * T.MAX_WIDTH, band=0, max_width=T.MAX_WIDTH) == (-1, 0)
    assert T.pair_identity([], [], 3).shape == (0, 2)
