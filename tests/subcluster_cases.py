"""TEST INFRASTRUCTURE: the inputs of the sub-clustering tests (tests/test_subcluster_cases.py on the CPU, tests/test_gpu_subcluster.py
on the device), each case a (label, alignments, cutoff): `alignments` is what Context.msa_subcluster takes -- per alignment a list
of equal-length byte strings or a 2-D uint8 array -- and goes to it as ONE batch."""
import numpy as np

GAP = 45
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
CHUNK = 64       # HITE_SUBCLUSTER_CHUNK (the tests assert that the library says the same)


def rand_rows(rng, R, C):
    return ACGT[rng.integers(0, 4, size=(R, C))]


def other_base(row, cols):
    """row with another base (the next of ACGT) in the columns `cols`"""
    out = row.copy()
    idx = np.searchsorted(ACGT, out[cols])          # ACGT is ascending
    out[cols] = ACGT[(idx + 1) & 3]
    return out


# ---- 1. degenerate ------------------------------------------------------------------------------------------------------------------
def degenerate():
    a = b"ACGTACGTAC"
    return [
        ("nmat-0", [], 0.2),
        ("R-0", [[]], 0.2),
        ("R-0-array", [np.zeros((0, 7), dtype=np.uint8)], 0.2),
        ("R-1", [[a]], 0.2),
        ("R-2", [[a, b"TTTTTTTTTT"]], 0.2),
        ("C-0", [[b"", b"", b""]], 0.2),
        ("C-1", [[b"A", b"A", b"-", b"C", b"-", b"A"]], 0.2),
        ("all-gap-rows", [[b"----", b"ACGT", b"----", b"ACGT"]], 0.2),
        ("identical", [[a, a]], 0.2),
        ("empty-between", [[a, a, b"TTTTTTTTTT"], [], [b"GGGGG", b"GGGGC", b"CCCCC"]], 0.2),
        ("no-columns-between", [[a, a], [b"", b""], [b"GGGGG", b"GGGGC"]], 0.2),
    ]


DEGENERATE_EXPECT = {
    "nmat-0": [], "R-0": [[]], "R-0-array": [[]], "R-1": [[[0]]], "R-2": [[[0], [1]]], "C-0": [[[0], [1], [2]]],
    "C-1": [[[0, 1, 5], [2], [3], [4]]], "all-gap-rows": [[[0], [1, 3], [2]]], "identical": [[[0, 1]]],
    "empty-between": [[[0, 1], [2]], [], [[0, 1], [2]]], "no-columns-between": [[[0, 1]], [[0], [1]], [[0, 1]]],
}


# ---- 2. column tails and unaligned starts ----------------------------------------------------------------------------------------
TAIL_COLS = (1, 3, 4, 5, 15, 16, 17, 31, 33, 63, 64, 65, 127, 129, 255, 257, 1023, 1025)


def tail_alignment(rng, C):
    """9 rows x C.  Against row 0 every pair has n = 5k (k = C // 5; the C - 5k other columns hold gaps in every row, right after the
    first column) and diff = k or k + 1, and which of the two is decided by the first column or by the last one to three columns.
    (C < 5 has no such n: there n = C and diff = 0 .. 3, where one difference already decides.)"""
    k = C // 5
    m = np.repeat(rand_rows(rng, 1, C), 9, axis=0)
    both = np.arange(1, 1 + C - 5 * k) if C >= 5 else np.zeros(0, dtype=np.int64)
    hinge = sorted({0, C - 1, max(C - 2, 0), max(C - 3, 0)})
    middle = np.array([c for c in range(C) if c not in hinge and c not in set(both.tolist())], dtype=np.int64)

    def vary(r, total, ends, gap=False):
        """row r: `total` differences from row 0, as many of them as fit in the columns `ends`, the rest in the middle"""
        ends = [c for c in dict.fromkeys(ends) if 0 <= c < C][:total]
        cols = rng.permutation(middle)[:min(total - len(ends), len(middle))]
        m[r] = other_base(m[r], cols)
        if gap:
            m[r, ends] = GAP
        else:
            m[r] = other_base(m[r], np.array(ends, dtype=np.int64))

    vary(1, k, [0])                          # k with the first column: joins
    vary(2, k + 1, [0])                      # k + 1 with it: does not
    vary(3, k + 1, [C - 1])
    vary(4, k, [C - 1])
    vary(5, k, [C - 1, C - 2])
    vary(6, k + 1, [C - 1, C - 2, C - 3])
    vary(7, k + 1, [C - 1], gap=True)        # a base against a gap in the last column
    vary(8, k, [0], gap=True)
    m[:, both] = GAP
    return m


def tails():
    rng = np.random.default_rng(4102)
    return [("tails", [tail_alignment(rng, C) for C in TAIL_COLS], 0.2)]


# ---- 3. the threshold ---------------------------------------------------------------------------------------------------------------
THRESHOLD_N = (5, 10, 15, 16, 17, 18, 19, 100, 4095, 4096, 4097, 4098, 4099, 65535)


def threshold_alignment(rng, n):
    """3 rows: the leader, a row with diff = n // 5 (joins) and one with n // 5 + 1 (does not).  Columns where all rows hold gaps
    are added in the number that would let the third row join if they counted towards n.  A third of the differences have a gap
    in the leader, a third a gap in the row."""
    f = n // 5
    extra = min(5 * (f + 1) - n, 65535 - n)
    base = rand_rows(rng, 1, n)[0]
    cols = rng.permutation(n)[:f + 1]
    rows = [base.copy(), other_base(base, cols[:f]), other_base(base, cols)]
    a, b = (f + 2) // 3, 2 * ((f + 2) // 3)
    rows[0][cols[:min(a, f)]] = GAP            # (the other two rows hold a base there)
    for r in (1, 2):
        rows[r][cols[a:min(b, f)]] = GAP
    m = np.stack(rows)
    if extra > 0:
        at = np.sort(rng.integers(0, n + 1, size=extra))
        m = np.insert(m, at, GAP, axis=1)
    return np.ascontiguousarray(m)


def threshold():
    rng = np.random.default_rng(4103)
    return [("threshold", [threshold_alignment(rng, n) for n in THRESHOLD_N], 0.2)]


# ---- 4. order -----------------------------------------------------------------------------------------------------------------------
def order():
    L0 = b"A" * 20
    L1 = b"C" * 20
    L2 = b"GGGGGG" + b"A" * 14                 # 6 of 20 from L0: no match
    X = b"GGGAAA" + b"A" * 14                  # 3 from L0, 3 from L2: matches both
    A = b"A" * 20
    B = b"TTTT" + b"A" * 16                    # 4 from A
    Cc = b"TTTTTTTT" + b"A" * 12               # 4 from B, 8 from A
    abc = {"A": A, "B": B, "C": Cc}
    out = [("first-of-two-leaders", [[L0, L1, L2, X]], 0.2)]
    for perm in ("ABC", "ACB", "BAC", "BCA", "CAB", "CBA"):
        out.append(("order-" + perm, [[abc[ch] for ch in perm]], 0.2))
    return out


ORDER_EXPECT = {
    "first-of-two-leaders": [[[0, 3], [1], [2]]],
    "order-ABC": [[[0, 1], [2]]],              # C matches B, a member, and not the leader A: it founds its own
    "order-ACB": [[[0, 2], [1]]],
    "order-BAC": [[[0, 1, 2]]],
    "order-BCA": [[[0, 1, 2]]],
    "order-CAB": [[[0, 2], [1]]],              # B matches both leaders: the first
    "order-CBA": [[[0, 1], [2]]],
}


# ---- 5. leader counts ---------------------------------------------------------------------------------------------------------------
LEADER_ROWS = (63, 64, 65, 255, 256, 257, 1025)


def leader_alignment(rng, R, C=40):
    m = rand_rows(rng, R, C)
    tail = []
    for src in (0, 63, 64, R - 1):
        if src < R:
            tail.append(m[src])
            tail.append(other_base(m[src], rng.permutation(C)[:3]))
    return np.concatenate([m, np.stack(tail)])


def leader_counts():
    rng = np.random.default_rng(4105)
    return [("leaders-%d" % R, [leader_alignment(rng, R)], 0.2) for R in LEADER_ROWS]


# ---- 6. chunk boundaries ------------------------------------------------------------------------------------------------------------
def family_alignment(rng):
    """R < 40 rows x C < 60 columns: 1 to 4 families, every row 5 - 20 % from the centre of its family, a few gaps"""
    R, C = int(rng.integers(1, 40)), int(rng.integers(1, 60))
    centres = rand_rows(rng, int(rng.integers(1, 5)), C)
    m = centres[rng.integers(0, len(centres), size=R)].copy()
    for r in range(R):
        noisy = rng.random(C) < rng.uniform(0.05, 0.20)
        m[r] = other_base(m[r], np.nonzero(noisy)[0])
    m[rng.random((R, C)) < 0.03] = GAP
    return m


def family_batch(n=300, seed=4106):
    rng = np.random.default_rng(seed)
    return [family_alignment(rng) for _ in range(n)]


def chunk_boundary_alignment(rng, R, B=CHUNK, C=40):
    """unrelated rows with, where R has room for them:
      rows 0, 1         a leader and a later row of its chunk that joins it
      rows 2, 3, 4      3 joins 2; 4 matches 3 (6 columns away) and not 2 (12 away): it founds a sub-cluster
      rows B-2, B-1, B  the same triple across the chunk border
      rows 5, B+2, B+5  B+2 is 12 columns from the old leader 5 and becomes a leader of the second chunk; B+5 is 6 from either
                        and joins the old one
      the last row      a copy of row 0, where none of the above stands there"""
    m = rand_rows(rng, R, C)
    cols = np.arange(12)

    def triple(a, b, c):
        if b < R:
            m[b] = other_base(m[a], cols[:6])
        if c < R:
            m[c] = other_base(m[b], cols[6:])
    m[R - 1] = m[0]
    m[1] = other_base(m[0], cols[:3])
    triple(2, 3, 4)
    triple(B - 2, B - 1, B)
    if B + 5 < R:
        m[B + 2] = other_base(m[5], cols)
        m[B + 5] = other_base(m[5], cols[:6])
    return m


def chunk_boundary(B=CHUNK):
    rng = np.random.default_rng(4107)
    return [("chunk-boundary", [chunk_boundary_alignment(rng, R, B) for R in (B - 1, B, B + 1, 2 * B + 1)], 0.2)]


# ---- 7. bytes -----------------------------------------------------------------------------------------------------------------------
def byte_values():
    rows = [b"ACGTACGTAC", b"acgtacgtac", b"ACGTACGTAc", b"NNNNNNNNNN", b"ACGTACGTNN", b"\x00" * 10, b"\xff" * 10,
            b"\x00" * 8 + b"\xff\xff", b"-" * 10, b"." * 10, b"-" * 8 + b"..", b"." * 8 + b"--"]
    wide = [r * 7 for r in rows]             # the same through the whole words
    return [("bytes", [rows, wide], 0.2)]


BYTES_EXPECT = {"bytes": [[[0, 2, 4], [1], [3], [5, 7], [6], [8], [9, 11], [10]]] * 2}


# ---- 8. size ------------------------------------------------------------------------------------------------------------------------
def planted_families(rng, R, C, n_fam, spread, apart):
    """centres `apart` from each other (each apart / 2 from a common ancestor), every row `spread` around its centre"""
    root = rand_rows(rng, 1, C)[0]
    centres = [other_base(root, np.nonzero(rng.random(C) < apart / 2)[0]) for _ in range(n_fam)]
    m = np.stack([centres[k] for k in rng.integers(0, n_fam, size=R)])
    noisy = rng.random((R, C)) < spread
    idx = np.searchsorted(ACGT, m)
    m[noisy] = ACGT[(idx[noisy] + rng.integers(1, 4, size=int(noisy.sum()))) & 3]
    return m


def size_batch():
    rng = np.random.default_rng(4108)
    big = [rand_rows(rng, 600, 2000), planted_families(rng, 3000, 1500, 6, 0.08, 0.30)]
    return [("size", big + family_batch(200, seed=4109), 0.2)]


# ---- 10. host layer -----------------------------------------------------------------------------------------------------------------
def _seq(codes):
    return ACGT[codes].tobytes().decode()


def cons_clusters(seed=4110):
    """clusters for _generate_cons_batch, each a list of (name, sequence): three with two sub-families 30 % apart (copies 2 %
    around their centres), one of them with a member the aligner drops (shorter than half the centre), and a singleton"""
    rng = np.random.default_rng(seed)
    out = []
    for ci in range(3):
        L = int(rng.integers(240, 400))
        root = rng.integers(0, 4, size=L)
        centres = []
        for _ in range(2):
            c = root.copy()
            ch = rng.random(L) < 0.15
            c[ch] = (c[ch] + rng.integers(1, 4, size=int(ch.sum()))) & 3
            centres.append(c)
        cl = []
        for k in range(int(rng.integers(5, 9))):
            c = centres[k % 2].copy()
            ch = rng.random(L) < 0.02
            c[ch] = (c[ch] + rng.integers(1, 4, size=int(ch.sum()))) & 3
            cl.append(("c%d_m%d" % (ci, k), _seq(c)))
        if ci == 1:
            cl.insert(3, ("c1_short", _seq(centres[0][:L // 3])))
        out.append(cl)
    out.append([("single", _seq(rng.integers(0, 4, size=200)))])
    return out


def small_cases():
    """everything but the size batch and the 300 random alignments"""
    return degenerate() + tails() + threshold() + order() + leader_counts() + chunk_boundary() + byte_values()
