"""Inputs of the pairwise-identity tests (hite_pair_identity): the CPU tests run them through the twin and through the kernel's cell update
built for the host, the GPU tests through the kernel.  Every case is (label, seqs, pairs, band); pairs are rows
(a_id, a_start, a_end, b_id, b_start, b_end, strand)."""
import numpy as np

MAX_WIDTH = 2048     # HITE_IDENT_MAX_WIDTH
MAX_LEN = 32767

_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def rand_seq(rng, n):
    return rng.choice(np.frombuffer(b"ACGT", np.uint8), size=int(n)).tobytes()


def revcomp(s):
    return s.translate(_COMP)[::-1]


def substitute(rng, s, rate):
    """every base replaced by a DIFFERENT one with probability `rate`"""
    a = np.frombuffer(s, np.uint8).copy()
    hit = np.flatnonzero(rng.random(len(a)) < rate)
    for k in hit:
        a[k] = rng.choice([c for c in b"ACGT" if c != a[k]])
    return a.tobytes()


def mutate(rng, s, sub, indel):
    out = bytearray()
    for c in s:
        x = rng.random()
        if x < indel / 2:
            continue
        if x < indel:
            out.append(int(rng.choice(list(b"ACGT"))))
        out.append(int(rng.choice(list(b"ACGT"))) if rng.random() < sub else c)
    return bytes(out)


def whole(seqs, a, b, strand=0):
    return (a, 0, len(seqs[a]), b, 0, len(seqs[b]), strand)


def degenerate():
    seqs = [b"", b"A", b"C", b"AC", b"CA", b"ACGTACGTAC", b"ACGTACGTAC", b"AAAAAAAA", b"CCCCCCCC", b"NNNNNN", b"NNNNNN", b"acgtacgtac",
            b"AcGtaCgTAc", b"AC-T*RYK\x00\xffGT", b"ac-t*ryk\x00\xffgt", b"ACNTNRYKNNGT", b"GTACGTACGT", b"nnnn", b"ACGTNACGT", b"acgtnacgt"]
    pairs = [whole(seqs, a, b, st) for a in range(len(seqs)) for b in range(len(seqs)) for st in (0, 1)]
    return [("degenerate", seqs, pairs, 4)]


def reverse_strand():
    rng = np.random.default_rng(41)
    s0 = rand_seq(rng, 90)
    s1 = revcomp(mutate(rng, s0, 0.05, 0.03))
    s2 = rand_seq(rng, 40) + revcomp(s0[10:60]) + rand_seq(rng, 7)
    seqs = [s0, s1, s2]
    pairs = []
    for st in (0, 1):
        pairs += [(0, 0, 50, 1, len(s1) - 52, len(s1), st),        # the first base of one, the last base of the other
                  (0, 40, len(s0), 1, 0, 47, st),
                  (0, 0, len(s0), 1, 0, len(s1), st),
                  (0, 10, 60, 2, 40, 90, st),
                  (0, 5, 45, 0, 30, 75, st),                          # both intervals from the same sequence
                  (2, 0, 50, 2, 40, len(s2), st),
                  (0, 20, 20, 1, 10, 40, st),                         # a length of 0 in the middle of a sequence
                  (0, 20, 50, 1, 33, 33, st),
                  (2, 44, 44, 2, 44, 44, st)]
    return [("reverse", seqs, pairs, 6)]


def band_widths():
    """band = 8: the width is |n - m| + 17; 64 at a difference of 47, 128 at 111.  The widest band allowed and one diagonal more."""
    rng = np.random.default_rng(42)
    seqs, pairs = [], []
    for diff in (46, 47, 48, 110, 111, 112, MAX_WIDTH - 17, MAX_WIDTH - 16, MAX_WIDTH - 17):
        a = rand_seq(rng, 140)
        at = int(rng.integers(0, len(a)))
        b = substitute(rng, a[:at], 0.05) + rand_seq(rng, diff) + substitute(rng, a[at:], 0.05)
        seqs += [a, b]
        k = len(seqs) - 2
        pairs += [whole(seqs, k, k + 1), whole(seqs, k + 1, k), (k, 0, len(a), k + 1, 0, len(b), 1)]
    return [("band_widths", seqs, pairs, 8)]


def row_counts():
    rng = np.random.default_rng(43)
    base = rand_seq(rng, 300)
    lens = (63, 64, 65, 255, 256, 257)
    seqs = [mutate(rng, base, 0.06, 0.04)[:n] for n in lens] + [revcomp(mutate(rng, base, 0.06, 0.04)[:n]) for n in lens]
    for k, n in enumerate(lens):
        assert len(seqs[k]) == n and len(seqs[6 + k]) == n
    pairs = [whole(seqs, a, b) for a in range(6) for b in range(6)] + [whole(seqs, a, 6 + b, 1) for a in range(6) for b in range(6)]
    return [("row_counts", seqs, pairs, 8)]


def edge_paths():
    """one long insertion or deletion at the very start or the very end: with band = 0 and n = m + d the band is exactly d + 1 diagonals
    and the path runs along lo or along hi.  Then an indel longer than the band allows: the result is the band-limited cost."""
    rng = np.random.default_rng(44)
    out = []
    seqs, pairs = [], []
    for d in (1, 5, 63, 64, 65, 130):
        a = rand_seq(rng, 150)
        ins = rand_seq(rng, d)
        for b in (ins + a, a + ins, ins[:d // 2] + a + ins[d // 2:]):
            seqs += [a, b]
            k = len(seqs) - 2
            pairs += [whole(seqs, k, k + 1), whole(seqs, k + 1, k)]
    out.append(("edge_band0", seqs, pairs, 0))
    seqs, pairs = [], []
    for d in (4, 9, 40):
        a = rand_seq(rng, 200)
        for b in (a[d:] + rand_seq(rng, d), rand_seq(rng, d) + a[:-d], a[:100] + a[100 + d:] + rand_seq(rng, d)):
            seqs += [a, b]
            k = len(seqs) - 2
            pairs += [whole(seqs, k, k + 1), whole(seqs, k + 1, k)]
    out.append(("edge_beyond_band", seqs, pairs, 3))
    return out


def longest():
    rng = np.random.default_rng(45)
    a = rand_seq(rng, MAX_LEN + 1)
    b = substitute(rng, a, 0.05)
    seqs = [a, b]
    pairs = [(0, 0, MAX_LEN, 1, 0, MAX_LEN, 0), (0, 0, MAX_LEN + 1, 1, 0, MAX_LEN + 1, 0), (0, 1, MAX_LEN + 1, 1, 0, MAX_LEN + 1, 0),
             (0, 100, 400, 1, 100, 400, 0)]
    return [("longest", seqs, pairs, 8)]


def batch(n_pair=3000, max_len=600, seed=46):
    rng = np.random.default_rng(seed)
    seqs, pairs = [], []
    for _ in range(n_pair):
        n = int(rng.integers(0, max_len + 1))
        a = rand_seq(rng, n)
        div = float(rng.choice([0.0, 0.02, 0.1, 0.2, 0.4]))
        b = mutate(rng, a, div * 0.75, div * 0.25)[:max_len]
        st = int(rng.integers(0, 2))
        if st:
            b = revcomp(b)
        if rng.random() < 0.1:
            b = b.lower()
        if rng.random() < 0.05 and len(b):
            b = b[:len(b) // 2] + b"N" + b[len(b) // 2 + 1:]
        seqs += [a, b]
        k = len(seqs) - 2
        if rng.random() < 0.3 and len(a) > 10 and len(b) > 10:
            x, y = int(rng.integers(0, 5)), int(rng.integers(0, 5))
            pairs.append((k, x, len(a) - y, k + 1, y if st else x, len(b) - (x if st else y), st))
        else:
            pairs.append(whole(seqs, k, k + 1, st))
    order = rng.permutation(len(pairs))
    return [("batch", seqs, [pairs[i] for i in order], 32)]


def invalid():
    """ids and intervals outside their sequences between good pairs"""
    seqs = [b"ACGTACGTAC", b"ACGAACGTAC"]
    good = (0, 0, 10, 1, 0, 10, 0)
    pairs = [good, (2, 0, 1, 0, 0, 1, 0), good, (0, 0, 11, 1, 0, 10, 0), (0, -1, 5, 1, 0, 5, 0), good, (0, 6, 5, 1, 0, 5, 0), (0, 0, 5, -1, 0, 5, 0),
             (0, 0, 5, 1, 3, 11, 1), good]
    return [("invalid", seqs, pairs, 2)]


def small_cases():
    """everything but the longest pair and the large batch"""
    return degenerate() + reverse_strand() + band_widths() + row_counts() + edge_paths() + invalid()
