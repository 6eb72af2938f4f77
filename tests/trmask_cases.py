"""Inputs of the tandem-repeat masker's edge tests, shared by the host-compiled check of the `tr_seed` block (test_host_compiled.py) and
the device tests (test_gpu_trmask.py): a genome for a sweep over max_period, arrays planted on the 4096-base tile borders and the
2048-base reseed points with contig ends beside them, and genomes shorter than a block, a word or a tile.  Every recorded count is
the TWIN's (oracle/hite_oracle_trf.c) masked-base count: a record of the reference, so that a changed generator cannot turn a
comparison into one of empty masks."""
import numpy as np

import casegen

_ACGT = np.frombuffer(b"ACGT", np.uint8)


def split(seq, cuts):
    """seq cut into contigs ending at `cuts` (the last one is len(seq))"""
    out, at = [], 0
    for c in cuts:
        out.append(seq[at:c])
        at = c
    assert at == len(seq)
    return out


# ---- the period sweep ------------------------------------------------------------------------------------------------------------
N_RUN = 40                  # N inserted at base 9777 of the sequence (inside the second contig)


def period_case():
    """-> (contigs, planted): the genome of test_tr_seed_kernel_logic_vs_twin -- three long contigs, an N run, two short contigs that
    are arrays themselves -- and the arrays planted in its sequence (make_tandem_case's coordinates: before the N run went in)"""
    seq, planted = casegen.make_tandem_case(777, G=40_000, n_arr=40)
    contigs = [seq[:9_000], seq[9_000:9_777] + "N" * N_RUN + seq[9_777:30_003], seq[30_003:], "ACGT" * 10, "ACGTTGCA" * 5]
    return contigs, planted


def period_genome():
    return period_case()[0]


def period_locate(x):
    """position x of make_tandem_case's sequence -> (contig, 0-based offset in it) in period_genome"""
    if x < 9_000:
        return 0, x
    if x < 9_777:
        return 1, x - 9_000
    if x < 30_003:
        return 1, x - 9_000 + N_RUN
    return 2, x - 30_003


# both sides of every group-of-16 border of tr_scan_word, the stride changes at 32 and 64, both parities above 64, ragged last groups
PERIODS = [1, 2, 7, 8, 15, 16, 17, 31, 32, 33, 47, 48, 63, 64, 65, 66, 79, 80, 81, 95, 96, 127, 128, 255, 256, 400, 495, 496, 497, 499, 500]
TWIN_MASKED = {}
for _ps, _n in [((1,), 91), ((2,), 133), ((7,), 311), ((8,), 351), ((15, 16, 17), 461), ((31, 32), 881), ((33,), 1804),
                ((47, 48, 63, 64, 65, 66), 3004), ((79, 80, 81, 95, 96), 3774), ((127, 128), 4368),
                ((255, 256, 400, 495, 496, 497, 499), 5466), ((500,), 6469)]:
    for _p in _ps:
        TWIN_MASKED[_p] = _n
assert sorted(TWIN_MASKED) == PERIODS

# ---- arrays on tile borders, reseed points and the genome start ---------------------------------------------------------------------
BORDER_G = 3 * 4096 + 77
# (position the array straddles, period)
BORDER_ARRAYS = [(4096, 1), (4096, 7), (4096, 31), (4096, 32), (8192, 63), (8192, 64), (8192, 65), (2048, 3), (6144, 127), (12288, 16),
                 (10240, 500), (0, 5)]


def border_genome(seed=3, G=BORDER_G):
    """random background; for every (at, p) of BORDER_ARRAYS an array of period p, max(3 p, 48) bases long with 3 % of its bases redrawn,
    that starts before `at` and ends behind it (at = 0: at the genome start)"""
    rng = np.random.default_rng(seed)
    seq = rng.choice(_ACGT, size=G)
    for at, p in BORDER_ARRAYS:
        unit = rng.choice(_ACGT, size=p)
        L = max(3 * p, 48)
        a = 0 if at == 0 else max(0, at + int(rng.integers(-L + 1, 0)))
        b = min(G, a + L)
        arr = np.tile(unit, L // p + 1)[:b - a].copy()
        hit = rng.random(b - a) < 0.03
        arr[hit] = rng.choice(_ACGT, size=int(hit.sum()))
        seq[a:b] = arr
    return seq.tobytes().decode()


# contig ends: no border; one on a tile border; two just beside one; one a stride of 32 past one
BORDER_CUTS = [[BORDER_G], [4096, BORDER_G], [4090, 8200, BORDER_G], [8224, BORDER_G]]
BORDER_PERIODS = [500, 64, 63, 33]
# twin's masked bases per cut: at max_period 500, and at 64 / 63 / 33 (the same three times: no array of period 34 .. 64 survives its 3 %)
BORDER_TWIN_MASKED = {500: [2321, 2319, 2122, 2130], 64: [247, 245, 239, 247], 63: [247, 245, 239, 247], 33: [247, 245, 239, 247]}


def border_cases():
    """-> [(label, contigs, max_period, twin's masked bases)]"""
    seq = border_genome()
    return [("cut%d-P%d" % (k, P), split(seq, cuts), P, BORDER_TWIN_MASKED[P][k]) for P in BORDER_PERIODS for k, cuts in enumerate(BORDER_CUTS)]


# ---- periods 16 .. 31 whose leftmost seed is the SECOND 8-block of its word --------------------------------------------------------------
# Below 32 a word carries two seed blocks (positions 0-7 and 8-15).  An array that starts at 8 modulo 16 has its leftmost seed in
# the second one; every later seed of the run has a seed before it and stays silent, so the array is found through that block alone.
# (None of the cases above depends on it for the group 16 .. 31: found by changing `g < 2` to `g < 1` in tr_scan_word, which passed them.)
BLOCK1_ARRAYS = [(520, 16), (1016, 17), (1512, 24), (2552, 31), (4104, 20), (4600, 31)]
BLOCK1_PERIODS = [31, 500]
BLOCK1_TWIN_MASKED = {31: 481, 500: 481}          # (465 bases of arrays, 16 of background beside them)


def block1_genome(seed=11, G=4096 + 1000):
    """random background with exact arrays of three copies and eight bases, each starting at 8 modulo 16, away from the reseed points"""
    rng = np.random.default_rng(seed)
    seq = rng.choice(_ACGT, size=G)
    for a, p in BLOCK1_ARRAYS:
        assert a % 16 == 8 and (a % 2048) + 3 * p + 8 < 2048
        seq[a:a + 3 * p + 8] = np.tile(rng.choice(_ACGT, size=p), 4)[:3 * p + 8]
    return seq.tobytes().decode()


# ---- degenerate genomes: one contig each ------------------------------------------------------------------------------------------------
TINY = ["A", "ACGTACG", "A" * 8, "A" * 9, "A" * 15, "A" * 16, "A" * 17, "A" * 31, "A" * 32, "A" * 33,
        "AC" * 20, "ACG" * 11, "N" * 50,
        "ACGTTGCA" * 513, "A" * 4095, "A" * 4096, "A" * 4097, "AC" * 2049, "A" * 5000]
TINY_PERIODS = [1, 2, 500]


def tiny_label(s):
    unit = next(s[:k] for k in range(1, len(s) + 1) if len(s) % k == 0 and s[:k] * (len(s) // k) == s)
    return "%sx%d" % (unit, len(s) // len(unit)) if len(unit) < len(s) else s


def tiny_expect_500(s):
    """what the twin does at max_period 500, where the definition says so outright: None = not stated"""
    if len(s) <= 17 or set(s) == {"N"}:
        return 0
    if set(s) == {"A"} and len(s) >= 31:
        return len(s)
    return None


def all_cases():
    """every (label, contigs, max_period) the host-compiled block is run on; the device tests run the same ones"""
    out = [("period-P%d" % P, period_genome(), P) for P in PERIODS]
    out += [(lab, contigs, P) for lab, contigs, P, _n in border_cases()]
    out += [("block1-P%d" % P, [block1_genome()], P) for P in BLOCK1_PERIODS]
    out += [("tiny-%s-P%d" % (tiny_label(s), P), [s], P) for s in TINY for P in TINY_PERIODS]
    return out
