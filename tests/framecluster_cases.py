"""TEST INFRASTRUCTURE: the inputs of the frame-clustering tests (tests/test_framecluster_cases.py on the CPU,
tests/test_gpu_framecluster.py on the device).  A case is (label, groups, kw): `groups` is what Context.frame_cluster takes, `kw` its
keyword arguments.  Where a result follows from the construction alone it stands beside the case (EXPECT[label]); everything
else is decided by the twin.  plain_cluster is a slow statement of the definition that shares no code with the twin: tuple
arithmetic on Python lists."""
import numpy as np

MAX_ROWS, MAX_LEN = 128, 256
SORT = dict(ident=0.8, cov_short=0.3, cov_long=0.0, min_cov=20, min_len=10, both_strands=True)       # sort_frame's options
JOINED = dict(ident=0.95, cov_short=0.95, cov_long=0.95, min_cov=50, min_len=10, both_strands=True)  # filter_ltr_by_flanking_cluster_sub's
EXPECT = {}


def kw(base=SORT, **over):
    d = dict(base)
    d.update(over)
    return d


def dna(rng, n, alphabet="ACGT"):
    return "".join(alphabet[k] for k in rng.integers(0, len(alphabet), n))


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGTacgt", "TGCAtgca"))


def substitute(s, positions):
    """another base at every position (the next of ACGT)"""
    s = list(s)
    for p in positions:
        s[p] = "ACGT"[("ACGT".index(s[p]) + 1) % 4]
    return "".join(s)


def mutate(rng, s, rate):
    """substitutions, insertions and deletions at `rate` per base"""
    out = []
    for ch in s:
        x = rng.random()
        if x < rate / 3:
            continue
        if x < 2 * rate / 3:
            out.append("ACGT"[rng.integers(0, 4)])
        if x < rate:
            out.append("ACGT"[("ACGT".index(ch) + 1 + rng.integers(0, 3)) % 4])
        else:
            out.append(ch)
    return "".join(out)


# ---- the plain model -------------------------------------------------------------------------------------------------------------
def _base(ch):
    ch = ch.upper()
    return ch if ch in "ACGT" else None


def plain_value(a, b):
    """R(a, b) of two str, one strand: lists of tuples, row by row"""
    E = (0, 0, 0, 0, 0)
    best = E
    prev = [E] * (len(b) + 1)
    for i in range(1, len(a) + 1):
        cur = [E]
        for j in range(1, len(b) + 1):
            x, y = _base(a[i - 1]), _base(b[j - 1])
            step = (2, 1, 1, 1, 1) if x is not None and x == y else (-2, 0, 1, 1, 1)
            cands = [tuple(p + q for p, q in zip(prev[j - 1], step)), tuple(p + q for p, q in zip(prev[j], (-3, 0, 1, 1, 0))),
                     tuple(p + q for p, q in zip(cur[j - 1], (-3, 0, 1, 0, 1)))]
            v = max(cands)
            if v[0] <= 0:
                v = E
            cur.append(v)
            best = max(best, v)
        prev = cur
    return best


def plain_pair(a, b, both_strands):
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    r = plain_value(a, b)
    if both_strands:
        rc = "".join(comp.get(ch.upper(), "N") for ch in reversed(b))
        r = max(r, plain_value(a, rc))
    return r


def plain_cluster(rows, ident, cov_short=0.0, cov_long=0.0, min_cov=0, min_len=10, both_strands=True):
    rows = [r.decode("latin-1") if isinstance(r, bytes) else r for r in rows]
    if len(rows) > MAX_ROWS or max([len(r) for r in rows] + [0]) > MAX_LEN:
        return None
    kept = [k for k in range(len(rows)) if len(rows[k]) > min_len]
    kept.sort(key=lambda k: -len(rows[k]))          # (stable: ties stay in index order)
    reps, clusters = [], []
    for k in kept:
        home = None
        for c, q in enumerate(reps):
            _s, m, cols, a, b = plain_pair(rows[q], rows[k], both_strands)
            if cols > 0 and float(m) >= ident * float(cols) and a >= min_cov and b >= min_cov and float(a) >= cov_long * float(len(rows[q])) \
                    and float(b) >= cov_short * float(len(rows[k])):
                home = c
                break
        if home is None:
            reps.append(k)
            clusters.append([k])
        else:
            clusters[home].append(k)
    return clusters


# ---- pairs with a known value ------------------------------------------------------------------------------------------------------
def _core(seed, n):
    """a core over G and T only: the fillers around it (A on one row, C on the other) never match it or each other"""
    return dna(np.random.default_rng(seed), n, "GT")


def pair_values():
    """(label, a, b, both_strands, R) with R worked out by hand"""
    c12, d12, c20 = _core(1, 12), _core(2, 12), _core(3, 20)
    x = c20
    out = [
        ("identical", x, x, False, (40, 20, 20, 20, 20)),
        # 16 matches in 20 columns: mismatches at 3, 7, 11, 15 leave every prefix and every suffix of the path positive
        ("16 of 20", x, substitute(x, [3, 7, 11, 15]), False, (24, 16, 20, 20, 20)),
        # the same score twice: after the core, a mismatch and a match (-2 + 2); the larger (matches, columns) is the value
        ("one score, two paths", c12 + "GT", c12 + "TT", False, (24, 13, 14, 14, 14)),
        # match, mismatch: the score is back at 0 and the path starts again behind them
        ("zero-score prefix", "TG" + c12, "TT" + c12, False, (24, 12, 12, 12, 12)),
        ("a gap in b", c12 + "A" + d12, c12 + d12, False, (45, 24, 25, 25, 24)),
        ("a gap in a", c12 + d12, c12 + "C" + d12, False, (45, 24, 25, 24, 25)),
        ("N matches nothing", c12 + "N" + d12, c12 + "N" + d12, False, (46, 24, 25, 25, 25)),
        ("lower case", (c12 + d12).lower(), c12 + d12, False, (48, 24, 24, 24, 24)),
        ("other bytes", c12 + "-" + d12, c12 + "-" + d12, False, (46, 24, 25, 25, 25)),
        ("reverse strand", "A" * 5 + x + "A" * 5, "A" * 3 + revcomp(x) + "A" * 3, True, None),
        ("empty", "", x, True, (0, 0, 0, 0, 0)),
    ]
    return out


# ---- cases -----------------------------------------------------------------------------------------------------------------------
def family(rng, n_rows, length, n_seed=3, rate=0.06, jitter=4):
    """n_rows rows around `length` bases drawn from n_seed unrelated seeds, each mutated and trimmed a little"""
    seeds = [dna(rng, length + jitter) for _ in range(n_seed)]
    rows = []
    for _ in range(n_rows):
        s = mutate(rng, seeds[rng.integers(0, n_seed)], rate)
        cut = int(rng.integers(0, jitter + 1))
        s = s[cut:cut + length] if rng.random() < 0.5 else s[:max(0, length - cut)]
        rows.append(revcomp(s) if rng.random() < 0.3 else s)
    return rows


def degenerate():
    rng = np.random.default_rng(11)
    a, b = dna(rng, 40), dna(rng, 40)
    s10, s11 = dna(rng, 10), dna(rng, 11)
    out = [("no groups", [], kw()),
           ("groups of 0, 1 and 2 rows", [[], [a], [a, a], [a, b], []], kw()),
           ("rows of length 0, 1, min_len, min_len + 1", [["", "A", s10, s11, s11, a]], kw(min_cov=11)),
           ("all rows dropped", [["", "ACGT", s10], [a, a]], kw()),
           ("only empty groups", [[], [], []], kw())]
    EXPECT["no groups"] = []
    EXPECT["groups of 0, 1 and 2 rows"] = [[], [[0]], [[0, 1]], [[0], [1]], []]
    EXPECT["rows of length 0, 1, min_len, min_len + 1"] = [[[5], [3, 4]]]
    EXPECT["all rows dropped"] = [[], [[0, 1]]]
    EXPECT["only empty groups"] = [[], [], []]
    return out


def row_edges():
    """groups at the row limit and around the 64 rows of a wavefront; 129 rows between two groups that are served"""
    rng = np.random.default_rng(12)
    out = []
    for n in (63, 64, 65, 127, 128):
        out.append(("%d rows" % n, [family(rng, n, 30, n_seed=5)], kw(min_cov=12)))
    small, mid = family(rng, 5, 40), family(rng, 7, 40)
    out.append(("129 rows between served groups", [small, family(rng, 129, 14), mid], kw(min_cov=12)))
    return out


def length_edges():
    rng = np.random.default_rng(13)
    out = []
    for n in (63, 64, 65, 255, 256):
        rows = family(rng, 5, n, n_seed=2, jitter=0)
        rows = [(r + dna(rng, n))[:n] for r in rows]        # every row exactly n bases
        out.append(("%d bases" % n, [rows], kw()))
    long_rows = [dna(rng, 257), dna(rng, 40)]
    out.append(("257 bases between served groups", [family(rng, 4, 64), long_rows, family(rng, 3, 256, n_seed=1)], kw()))
    x = dna(rng, 256)
    out.append(("12 next to 256", [[x[100:112], x, x[3:250], dna(rng, 12), x[200:230]]], kw(min_cov=0, cov_short=0.9)))
    out.append(("odd byte offsets", [[x[:31], x[:33], x[1:36]], [x[50:91], x[50:89]], [x[7:100], x[7:98]]], kw()))
    return out


def thresholds():
    """each threshold at its value and one base either side"""
    rng = np.random.default_rng(14)
    out = []
    x = _core(3, 20)
    rows = lambda core_a, core_b, n: ["A" * 35 + core_a + "A" * (n - 35 - len(core_a)), "C" * 20 + core_b + "C" * (n - 20 - len(core_b))]  # noqa: E731
    for n_mis, same in ((3, True), (4, True), (5, False)):
        label = "ident 0.8 at %d of 20" % (20 - n_mis)
        pos = [3, 7, 11, 15][:n_mis] if n_mis <= 4 else [2, 5, 8, 11, 14]
        out.append((label, [[x, substitute(x, pos)]], kw(ident=0.8, cov_short=0.0, min_cov=0)))
        EXPECT[label] = [[[0, 1]]] if same else [[[0], [1]]]
    for n in (19, 20, 21):
        label = "min_cov 20 at %d" % n
        c = _core(20 + n, n)
        out.append((label, [rows(c, c, 60)], kw(ident=0.8, cov_short=0.0, min_cov=20)))
        EXPECT[label] = [[[0, 1]]] if n >= 20 else [[[0], [1]]]
    for n in (29, 30, 31):
        label = "cov_short 0.3 at %d of 100" % n
        c = _core(40 + n, n)
        out.append((label, [rows(c, c, 100)], kw(ident=0.8, cov_short=0.3, min_cov=20)))
        EXPECT[label] = [[[0, 1]]] if n >= 30 else [[[0], [1]]]
    a = dna(rng, 200)
    for e in (0, 1, 2, 3, 10, 11):
        b = substitute(a, [7 + 17 * k for k in range(e)])
        out.append(("joined options, %d substitutions" % e, [[a, b]], kw(JOINED)))
    for e in (1, 2, 3):
        b = a
        for k in range(e):
            b = b[:40 + 50 * k] + b[41 + 50 * k:]
        out.append(("joined options, %d deletions" % e, [[a, b]], kw(JOINED)))
        out.append(("joined options, %d bases off the end" % (5 * e), [[a, a[:200 - 5 * e]]], kw(JOINED)))
    return out


def rule_order():
    rng = np.random.default_rng(15)
    p, q, s, u = (dna(rng, 30) for _ in range(4))
    k = kw(ident=0.8, cov_short=0.0, min_cov=20)
    out = [("A~B, B~C, A!~C", [[p + q + "AA", q + s + "C", s + u]], k),
           ("equal lengths by index", [[p + q, q + s, s + u], [s + u, q + s, p + q]], k),
           ("similar to two representatives", [[p + q, s + u[:29], q[:28] + s[:28]], [s + u[:29], p + q, q[:28] + s[:28]],
                                               [s + u, p + q[:29], q[:28] + s[:28]]], k)]
    EXPECT["A~B, B~C, A!~C"] = [[[0, 1], [2]]]
    EXPECT["equal lengths by index"] = [[[0, 1], [2]], [[0, 1], [2]]]
    EXPECT["similar to two representatives"] = [[[0, 2], [1]], [[1, 2], [0]], [[0, 2], [1]]]
    return out


def recurrence():
    """the pairs of pair_values as groups of two rows, with thresholds that a wrong value of the pair would miss"""
    c12, d12 = _core(1, 12), _core(2, 12)
    free = dict(cov_short=0.0, cov_long=0.0, min_cov=0, min_len=10, both_strands=False)
    out = [("one score, two paths: 13 of 14", [[c12 + "GT", c12 + "TT"]], dict(free, ident=0.95)),
           ("zero-score prefix is cut", [["TG" + c12, "TT" + c12]], dict(free, ident=1.0)),
           ("a gap in b: 25 and 24 bases", [[c12 + "A" + d12, c12 + d12]], dict(free, ident=0.9, min_cov=25)),
           ("a gap in b: 24 bases", [[c12 + "A" + d12, c12 + d12]], dict(free, ident=0.9, min_cov=24)),
           ("a gap in a: cov_long 1.0 on 24 of 25", [[c12 + d12 + "A", c12 + "C" + d12]], dict(free, ident=0.9, cov_long=1.0)),
           ("a gap in a: cov_long 0.96 on 24 of 25", [[c12 + d12 + "A", c12 + "C" + d12]], dict(free, ident=0.9, cov_long=0.96)),
           ("N against N", [[c12 + "N" + d12, c12 + "N" + d12]], dict(free, ident=0.97)),
           ("lower case and other bytes", [[(c12 + d12).lower(), c12 + d12, c12 + "-" + d12, c12 + "\t" + d12, c12 + "\xff" + d12,
                                            "n" * 24, "N" * 24]], dict(free, ident=0.97))]
    EXPECT["one score, two paths: 13 of 14"] = [[[0], [1]]]
    EXPECT["zero-score prefix is cut"] = [[[0, 1]]]
    EXPECT["a gap in b: 25 and 24 bases"] = [[[0], [1]]]
    EXPECT["a gap in b: 24 bases"] = [[[0, 1]]]
    EXPECT["a gap in a: cov_long 1.0 on 24 of 25"] = [[[0], [1]]]
    EXPECT["a gap in a: cov_long 0.96 on 24 of 25"] = [[[0, 1]]]
    EXPECT["N against N"] = [[[0], [1]]]
    return out


def strands():
    rng = np.random.default_rng(16)
    a = dna(rng, 90)
    b = revcomp(mutate(rng, a, 0.04))[:88]
    out = [("reverse complement, both strands", [[a, b]], kw(both_strands=True)),
           ("reverse complement, one strand", [[a, b]], kw(both_strands=False))]
    EXPECT["reverse complement, both strands"] = [[[0, 1]]]
    EXPECT["reverse complement, one strand"] = [[[0], [1]]]
    return out


def closed_forms():
    rng = np.random.default_rng(17)
    x = dna(rng, 100)
    out = [("identical rows", [[x] * 9, [x[:77]] * 70], kw(JOINED)),
           ("poly-A against poly-C", [["A" * 50, "C" * 49], ["A" * 50, "C" * 49, "G" * 48, "T" * 47]], kw(both_strands=False))]
    EXPECT["identical rows"] = [[list(range(9))], [list(range(70))]]
    EXPECT["poly-A against poly-C"] = [[[0], [1]], [[0], [1], [2], [3]]]
    return out


def many_small(n_group=3000, seed=18):
    """groups of 2 to 6 rows of 20 to 100 bases"""
    rng = np.random.default_rng(seed)
    groups = []
    for _ in range(n_group):
        n = int(rng.integers(2, 7))
        groups.append(family(rng, n, int(rng.integers(20, 101)), n_seed=2, rate=0.08))
    return groups


def small_cases():
    """every case the plain model can take in a few seconds"""
    return degenerate() + thresholds() + rule_order() + recurrence() + strands() + closed_forms()


def all_cases():
    return small_cases() + row_edges() + length_edges()
