"""Records for tests/test_itr_limit_cases.py and tests/test_gpu_itr_limits.py: itr_search_kernel (hite_amd/csrc/hite_itr.hip) at the
limits of its own code -- the two homes of the traceback store (LDS up to h = 64, a scratch slot in HBM above, chosen by the longest
record of a batch), the strips of 64 columns (lane 0 reads what lane 63 of the strip before left behind; row 1 has its own
diagonal), the end cell as the first maximum in row-major order (per-lane best over all strips, then a wave reduction), slots that
several records pass through, and the lengths (h = min(500, L / 2), ends that overlap, end_len beyond the cap).  Pure numpy /
python, seeded.  Written once and run twice: every check_* takes a callable with the signature of
Context.itr_search(seqs, end_len, **kw) -> int32 [n, 8] and compares all 8 fields, exact integer equality, with the CPU twin
(oracle/hite_oracle_itr.c through oracle_lib.itr_search), with a closed form, or with the tool's own answer
(tests/golden/itr_limits.json.gz).

restate() states the definition a second time, in plain numpy over full C / E / F matrices with a textbook first-maximum scan and an
explicit traceback that returns the path; it was written from the comment block of oracle/hite_oracle_itr.c, not from its code.  The
builders use it to show what a case reaches (a gap across a strip boundary, several cells at the maximum, a traceback that depends
on the open / extend tie or on the N wildcard of seq2)."""
import numpy as np

import casegen
import oracle_lib as O

# ITR_MAX_H, ITR_LDS_H, ITR_WAVES, grid cap on the LDS path, grid cap on the HBM path, columns of a strip: what the CPU test works
# with; the GPU test asserts that Context.itr_limits() says the same
TABLE = (500, 64, 4, 2048, 128, 64)
MAX_H, LDS_H, WAVES, LDS_BLOCKS, HBM_BLOCKS, STRIP = TABLE

DEF = (0.7, 7, 10, 16, 32, 32)          # min_identity, min_len, match, mismatch, gap_open, gap_extend: the tool's run in the reference
SCORINGS = ((10, 16, 32, 32), (5, 4, 8, 2), (1, 3, 5, 2))
TIE_SCORINGS = ((1, 3, 5, 2), (4, 8, 8, 1), (5, 10, 15, 5))      # mismatch a multiple of match
BAND_SCORINGS = SCORINGS + ((4, 8, 8, 1),)
BASES = "ACGT"
EMPTY_ROW = [0, 0, 0, 0, 0, 0, -1, 0]
SKIPPED_ROW = [0, 0, 0, 0, 0, 0, -1, 8]
EINVAL = -1

_memo = {}


def cached(key, build):
    if key not in _memo:
        _memo[key] = build()
    return _memo[key]


def rand_seq(rng, n, alphabet=BASES):
    return "".join(alphabet[i] for i in rng.integers(0, len(alphabet), size=n))


_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
_OTHER = {"A": "C", "C": "A", "G": "T", "T": "G", "N": "N"}


def revcomp(s):
    return "".join(_COMP.get(c, "N") for c in reversed(s))


def record(seq1, seq2, spacer=""):
    """the sequence whose first bases are seq1 and whose last bases, reverse-complemented, are seq2"""
    return seq1 + spacer + revcomp(seq2)


def params(scoring=None, min_identity=0.7, min_len=7):
    return (min_identity, min_len) + tuple(scoring or DEF[2:])


def kw_of(p):
    return dict(min_identity=p[0], min_len=p[1], match=p[2], mismatch=p[3], gap_open=p[4], gap_extend=p[5])


def case(label, seq, end_len=0, p=DEF):
    return (label, seq, int(end_len), tuple(p))


def h_of(c):
    L = len(c[1])
    return min(MAX_H, min(L, c[2]) if c[2] > 0 else L // 2)


def run(itr_search, cases):
    """rows of `cases` in their order: one call per (end_len, parameters)"""
    out = np.zeros((len(cases), 8), dtype=np.int32)
    groups = {}
    for k, c in enumerate(cases):
        groups.setdefault((c[2], c[3]), []).append(k)
    for (e, p), idx in groups.items():
        res = np.asarray(itr_search([cases[k][1] for k in idx], e, **kw_of(p)))
        assert res.shape == (len(idx), 8) and res.dtype == np.int32, (res.shape, res.dtype)
        out[idx] = res
    return out


def twin_search(seqs, end_len=40, min_identity=0.7, min_len=7, match=10, mismatch=16, gap_open=32, gap_extend=32):
    return O.itr_search(seqs, end_len, min_identity, min_len, match, mismatch, gap_open, gap_extend)


def twin(name, cases):
    """the twin's rows of a family, computed once and never written to"""
    def build():
        r = run(twin_search, cases)
        r.setflags(write=False)
        return r
    return cached(("twin", name), build)


def assert_rows(got, exp, cases, what):
    bad = np.nonzero((np.asarray(got) != np.asarray(exp)).any(axis=1))[0]
    assert bad.size == 0, "%s: %d of %d rows differ, first %s: got %s, expected %s" % (
        what, bad.size, len(cases), cases[bad[0]][0], np.asarray(got)[bad[0]].tolist(), np.asarray(exp)[bad[0]].tolist())


# ------------------------------------------------------------------------------------------------------------------------------
# the definition, stated a second time
# ------------------------------------------------------------------------------------------------------------------------------
NEG = -(1 << 40)


def ends_of(seq, end_len):
    """(seq1, seq2) as byte arrays folded to ACGTN: the first h bases and the reverse complement of the last h"""
    b = seq.encode() if isinstance(seq, str) else bytes(seq)
    if end_len > 0:
        e = min(len(b), end_len)
        b = b[:e] + b[len(b) - e:]
    h = min(MAX_H, len(b) // 2)
    fold = np.full(256, ord("N"), dtype=np.uint8)
    comp = np.full(256, ord("N"), dtype=np.uint8)
    for x, y in _COMP.items():
        fold[ord(x)] = ord(x)
        comp[ord(x)] = ord(y)
    a = np.frombuffer(b, dtype=np.uint8)
    return fold[a[:h]], comp[a[::-1][:h]]


def restate(seq, end_len=0, min_identity=0.7, min_len=7, match=10, mismatch=16, gap_open=32, gap_extend=32, tie_opens=False,
            n2_wild=True):
    """-> (row of 8, info).  Gotoh's recurrences from (0,0) with a free end:
        C(i,0) = C(0,i) = -(go + i ge), C(0,0) = 0
        E(i,j) = max(E(i,j-1), C(i,j-1) - go) - ge       (a step along seq2; a tie extends)
        F(i,j) = max(F(i-1,j), C(i-1,j) - go) - ge       (a step along seq1; a tie extends)
        C(i,j) = max(D, F, E), D = C(i-1,j-1) + w(i,j) -- for j = 1 the tool takes C(i,0) in the place of C(i-1,0) --
        w = +match if the bases are equal or either is N, else -mismatch; D wins ties, then F, then E
    end = the first cell in row-major order with the largest score, if that is > 0; the traceback jumps every gap back to the cell
    before the one it opened in; identity = equal bytes / diagonal steps.  info: gaps [(kind, row or column, first, last)] of the
    path, cells [(i, j)] at the maximum in row-major order.  tie_opens / n2_wild: two OTHER rules (a tie of open and extend marks an
    opening in the traceback; an N of seq2 is no wildcard) -- a case whose row changes under one of them is a case that tells the
    rules apart."""
    go, ge = gap_open, gap_extend
    s1, s2 = ends_of(seq, end_len)
    h = len(s1)
    info = dict(h=h, gaps=[], cells=[])
    if h <= 0:
        return list(EMPTY_ROW), info
    N = ord("N")
    W = (s1[:, None] == s2[None, :]) | (s1[:, None] == N)
    if n2_wild:
        W |= s2[None, :] == N
    Wf = np.fliplr(np.where(W, match, -mismatch).astype(np.int64))
    # anti-diagonal storage: X[d, i] = X(i, d - i)
    Cs = np.full((2 * h + 1, h + 1), NEG, dtype=np.int64)
    Es = np.full((2 * h + 1, h + 1), NEG, dtype=np.int64)
    Fs = np.full((2 * h + 1, h + 1), NEG, dtype=np.int64)
    edge = -(go + np.arange(h + 1, dtype=np.int64) * ge)
    edge[0] = 0
    Cs[np.arange(h + 1), np.arange(h + 1)] = edge      # C(i, 0)
    Cs[np.arange(h + 1), 0] = edge                     # C(0, j)
    for d in range(2, 2 * h + 1):
        lo, hi = max(1, d - h), min(h, d - 1)
        cl, el = Cs[d - 1, lo:hi + 1], Es[d - 1, lo:hi + 1]          # (i, j - 1)
        cu, fu = Cs[d - 1, lo - 1:hi], Fs[d - 1, lo - 1:hi]          # (i - 1, j)
        e = np.maximum(el, cl - go) - ge
        f = np.maximum(fu, cu - go) - ge
        cd = Cs[d - 2, lo - 1:hi].copy()                             # (i - 1, j - 1)
        if hi == d - 1:
            cd[-1] = edge[hi]                                        # j = 1: C(i, 0)
        dg = cd + Wf.diagonal(h - 1 - (d - 2))
        Cs[d, lo:hi + 1] = np.where((dg >= f) & (dg >= e), dg, np.where(f >= e, f, e))
        Es[d, lo:hi + 1] = e
        Fs[d, lo:hi + 1] = f
    ii, jj = np.ogrid[0:h + 1, 0:h + 1]
    Cm, Em, Fm = Cs[ii + jj, ii], Es[ii + jj, ii], Fs[ii + jj, ii]
    inner = Cm[1:, 1:]
    mx = int(inner.max())
    if mx <= 0:
        return list(EMPTY_ROW), info
    flat = np.flatnonzero(inner == mx)
    info["cells"] = [(int(x // h) + 1, int(x % h) + 1) for x in flat]
    ei, ej = info["cells"][0]
    bi, bj, matches, aligned, flags = ei, ej, 0, 0, 0

    def opened(c_before, x_before):
        return c_before - go >= x_before if tie_opens else c_before - go > x_before

    while bi > 0 and bj > 0:
        dg = (edge[bi] if bj == 1 else Cm[bi - 1, bj - 1]) + (match if W[bi - 1, bj - 1] else -mismatch)
        e, f = Em[bi, bj], Fm[bi, bj]
        if dg >= f and dg >= e:
            aligned += 1
            matches += int(s1[bi - 1] == s2[bj - 1])
            bi, bj = bi - 1, bj - 1
        elif f >= e:
            k = bi
            while k >= 1 and not opened(Cm[k - 1, bj], Fm[k - 1, bj] if k > 1 else Cm[0, bj] - go):
                k -= 1
            if k < 1:
                flags, k = flags | 1, 1
            info["gaps"].append(("F", bj, k, bi))
            bi = k - 1
        else:
            k = bj
            while k >= 1 and not opened(Cm[bi, k - 1], Em[bi, k - 1] if k > 1 else Cm[bi, 0] - go):
                k -= 1
            if k < 1:
                flags, k = flags | 1, 1
            info["gaps"].append(("E", bi, k, bj))
            bj = k - 1
    ident = float(matches & 0xFFFF) / float(aligned & 0xFFFF) if aligned & 0xFFFF else float("nan")
    found = int((min_len & 0xFFFFFFFF) <= ei and ident >= min_identity)
    return [mx, ei, ej, matches, aligned, found, ei - 1, flags], info


def restate_case(c, **rules):
    if rules:
        return restate(c[1], c[2], **kw_of(c[3]), **rules)
    return cached(("restate", c[1], c[2], c[3]), lambda: restate(c[1], c[2], **kw_of(c[3])))


# ------------------------------------------------------------------------------------------------------------------------------
# closed form: a perfect inverted repeat of k bases scores match k - (gap_open + gap_extend) and ends at (k, k)
# ------------------------------------------------------------------------------------------------------------------------------
def closed_ks():
    s, m = STRIP, MAX_H
    return (6, 7, 8, s - 1, s, s + 1, 2 * s - 1, 2 * s, 2 * s + 1, 3 * s - 1, 3 * s, 3 * s + 1, m - 1, m, m + 1, m + 100)


def closed_row(k, L, p):
    """the row of a perfect repeat of k bases in a record of L: every alignment pays the handicap of its first diagonal step, so no
    cell beats match min(i, j) - (go + ge) and (k, k) is alone at the top"""
    k = min(k, MAX_H)
    score = p[2] * k - (p[4] + p[5])
    if score <= 0:
        return list(EMPTY_ROW)
    return [score, k, k, k, k, int(p[1] <= k and 1.0 >= p[0]), k - 1, 0]


def closed_form():
    def build():
        rng = np.random.default_rng(9101)
        cases, rows = [], []
        for sc in SCORINGS:
            p = params(sc)
            for k in closed_ks():
                u = rand_seq(rng, k)
                for sp in ("", "A", "AA"):      # AA: one more row and column, A against T
                    cases.append(case("closed k=%d spacer=%d %s" % (k, len(sp), sc), record(u, u, sp), 0, p))
                    rows.append(closed_row(k, len(cases[-1][1]), p))
        return cases, np.asarray(rows, dtype=np.int32)
    return cached("closed_form", build)


def check_closed_form(itr_search):
    cases, rows = closed_form()
    assert_rows(run(itr_search, cases), rows, cases, "closed form")
    return len(cases)


# ------------------------------------------------------------------------------------------------------------------------------
# strip seams: a gap planted across a boundary column; an alignment that enters row 1 in the first column of a later strip
# ------------------------------------------------------------------------------------------------------------------------------
def seam_ps():
    s = STRIP
    return list(range(s - 4, s + 3)) + list(range(2 * s - 2, 2 * s + 3)) + list(range(3 * s - 2, 3 * s + 3))


SEAM_INS = (1, 2, 3, 8, 12, 30)


def seams():
    """seq1 = P + Q, seq2 = P + INS + Q (the E-gap: columns without a row) and the mirror (the F-gap); Q long enough to pay for
    the gap.  Then: seq2 = J + U, J of 64 s - 1, 64 s, 64 s + 1 bases that match nothing: the best alignment leaves (0, |J|) on the
    diagonal and its first cell is (1, |J| + 1) -- the first column of strip s when |J| = 64 s."""
    def build():
        rng = np.random.default_rng(9102)
        cases = []
        for sc in SCORINGS:
            p = params(sc)
            for pl in seam_ps():
                for n_ins in SEAM_INS:
                    q = (sc[2] + n_ins * sc[3]) // sc[0] + 20
                    P, Q = rand_seq(rng, pl), rand_seq(rng, q)
                    # the inserted bases differ from the base after them: the gap cannot slide to the right
                    ins = rand_seq(rng, n_ins - 1) + _OTHER[Q[0]]
                    for kind in "EF":
                        a, b = P + Q + rand_seq(rng, n_ins), P + ins + Q
                        if kind == "F":
                            a, b = b, a
                        cases.append(case("seam %s |P|=%d |INS|=%d %s" % (kind, pl, n_ins, sc), record(a, b), 0, p))
        for sc in SCORINGS:
            p = params(sc)
            for s in (1, 2, 3):
                for off in (s * STRIP - 1, s * STRIP, s * STRIP + 1):
                    k = (sc[2] + off * sc[3]) // sc[0] + 30
                    if off + k > MAX_H:
                        continue
                    u = rand_seq(rng, k, "CG")
                    cases.append(case("row 1 enters at column %d %s" % (off + 1, sc), record(u + "A" * off, "T" * off + u), 0, p))
        # a tie of open and extend on the path: seq1 = P + B + Q, seq2 = P + B' + Y + B + R + Q, B' = B with one mismatch,
        # gap_open = match + mismatch.  One gap over Y + B + R after the mismatch scores what a gap over B' + Y, B matched, and a
        # second gap over R score; in the cell before R the open and the extension tie, and the gap is the one that extends.
        for sc in ((4, 8, 12, 3), (4, 4, 8, 2)):
            p = params(sc)
            assert sc[2] == sc[0] + sc[1]
            for pl in (STRIP - 4, STRIP - 2, STRIP - 1, STRIP, STRIP + 1, 2 * STRIP - 2, 2 * STRIP):
                P, B, Y, R = rand_seq(rng, pl - 10), rand_seq(rng, 10), rand_seq(rng, 2), rand_seq(rng, 3)
                Q = rand_seq(rng, (2 * sc[2] + 15 * sc[3]) // sc[0] + 20)
                R = R[:-1] + _OTHER[Q[0]]
                b2 = B[:4] + _OTHER[B[4]] + B[5:]
                a, b = P + B + Q + rand_seq(rng, 15), P + b2 + Y + B + R + Q
                cases.append(case("open tie E |P+B|=%d %s" % (pl, sc), record(a, b), 0, p))
                cases.append(case("open tie F |P+B|=%d %s" % (pl, sc), record(b, a), 0, p))
        return cases
    return cached("seams", build)


def seam_reach(cases):
    """{(kind, boundary): cases whose path has a gap that starts at or before the boundary and ends after it}, and the cases whose
    alignment begins in row 1 at the first column of a later strip"""
    reach, row1 = {}, 0
    for c in cases:
        row, info = restate_case(c)
        for kind, _at, first, last in info["gaps"]:
            for s in (1, 2, 3):
                if first <= s * STRIP < last:
                    reach[(kind, s * STRIP)] = reach.get((kind, s * STRIP), 0) + 1
        if c[0].startswith("row 1") and row[0] > 0 and row[2] - row[1] >= STRIP and (row[2] - row[1]) % STRIP == 0 and not info["gaps"] \
                and row[4] == row[1]:
            row1 += 1
    return reach, row1


def check_seams(itr_search):
    cases = seams()
    assert_rows(run(itr_search, cases), twin("seams", cases), cases, "strip seams")
    return len(cases)


# ------------------------------------------------------------------------------------------------------------------------------
# ties for the end cell
# ------------------------------------------------------------------------------------------------------------------------------
TIE_AS = (62, 63, 64, 126, 127)


def ties():
    """(a) a perfect run of a bases, one mismatch, mismatch / match matches: (a, a) and (a + 1 + m, a + 1 + m) carry the same
    score, in different lanes and (for these a) different strips.  (b) the same row, 64 columns apart -- the same LANE in two
    strips: seq1 = U, seq2 = U[:k] + G + U[k:] with G of 64 bases that begins like U[k:] with every second of its first 2 x bases changed,
    x (match + mismatch) = gap_open + 64 gap_extend: the path along the diagonal (x mismatches) and the path through the gap of 64
    columns meet row a with the same score.  The first in row-major order is the end."""
    def build():
        rng = np.random.default_rng(9103)
        cases = []

        def drawn(make, wanted):
            """a case whose cells at the maximum are the wanted ones and whose twin row has no flag; drawn again otherwise"""
            for _try in range(50):
                c = make()
                if wanted(restate_case(c)[1]["cells"]) and int(run(twin_search, [c])[0][7]) == 0:
                    return c
            raise AssertionError("no tie after 50 draws: " + c[0])

        for sc in TIE_SCORINGS:
            p = params(sc)
            m = sc[1] // sc[0]
            for a in TIE_AS:
                for rep in range(2):
                    def diagonal():
                        u = rand_seq(rng, a + 1 + m, "ACG")
                        v = u[:a] + _OTHER[u[a]] + u[a + 1:]
                        return case("tie diagonal a=%d %s #%d" % (a, sc, rep), record(u + "T" * 8, v + "A" * 8), 0, p)
                    cases.append(drawn(diagonal, lambda cells: len(cells) >= 2 and cells[0] == (a, a)))
        # gaps dear enough that no pair of gaps pays for stepping around a mismatch, the mismatches one base apart
        for sc in ((4, 8, 12, 3), (4, 4, 8, 2)):
            p = params(sc)
            x, rem = divmod(sc[2] + STRIP * sc[3], sc[0] + sc[1])
            assert rem == 0
            for a in TIE_AS + (65, 128):
                for tail in (x * (sc[0] + sc[1]) // sc[0] + 4, 60):
                    assert 2 * x <= tail <= STRIP and sc[0] * (tail - x) > sc[1] * x
                    def row():
                        k = a - tail
                        u = rand_seq(rng, a, "ACG")
                        g = "".join(_OTHER[ch] if n % 2 == 0 and n < 2 * x else ch for n, ch in enumerate(u[k:])) + "A" * (STRIP - tail)
                        assert len(g) == STRIP
                        return case("tie row a=%d tail=%d %s" % (a, tail, sc), record(u + "T" * STRIP, u[:k] + g + u[k:]), 0, p)
                    cases.append(drawn(row, lambda cells: cells[:1] == [(a, a)] and (a, a + STRIP) in cells))
        return cases
    return cached("ties", build)


def tie_reach(cases):
    """(fewest cells at the maximum over the cases, cases whose first and last such cell lie in different strips, cases with two such
    cells in one row a multiple of 64 columns apart)"""
    fewest, strips, same_lane = 1 << 30, 0, 0
    for c in cases:
        _row, info = restate_case(c)
        cells = info["cells"]
        fewest = min(fewest, len(cells))
        if cells and (cells[0][1] - 1) // STRIP != (cells[-1][1] - 1) // STRIP:
            strips += 1
        if any(x[0] == y[0] and x[1] != y[1] and (y[1] - x[1]) % STRIP == 0 for x in cells for y in cells):
            same_lane += 1
    return fewest, strips, same_lane


def check_ties(itr_search):
    cases = ties()
    assert_rows(run(itr_search, cases), twin("ties", cases), cases, "ties")
    return len(cases)


# ------------------------------------------------------------------------------------------------------------------------------
# alphabet and thresholds
# ------------------------------------------------------------------------------------------------------------------------------
IDENT_FRACTIONS = ((7, 10), (14, 20), (21, 30), (3, 4), (4, 5), (6, 8), (8, 10), (69, 100))
IDENT_THRESHOLDS = (0.7, 0.75, 0.8, 0.0, 1.0, 1.01)


def alphabet():
    """-> (cases, expected `found` or None per case, names of the cases only ACGTN reaches)"""
    def build():
        rng = np.random.default_rng(9104)
        cases, found = [], []

        def add(c, f=None):
            cases.append(c)
            found.append(f)

        for h in (LDS_H, LDS_H + 1, MAX_H):
            add(case("all N h=%d" % h, "N" * (2 * h)))
        for k in (20, LDS_H, LDS_H + 6, 2 * STRIP + 2):
            u = rand_seq(rng, k)
            for r in (1, 3, 9):
                n = "N" * r
                add(case("N run: head of seq1 k=%d r=%d" % (k, r), record(n + u[r:], u)))
                add(case("N run: head of seq2 k=%d r=%d" % (k, r), record(u, n + u[r:])))
                add(case("N run: tail of seq1 k=%d r=%d" % (k, r), record(u[:-r] + n, u, "A")))
                add(case("N run: tail of seq2 k=%d r=%d" % (k, r), record(u, u[:-r] + n, "A")))
                add(case("N run: inside seq2 k=%d r=%d" % (k, r), record(u, u[:k // 2] + n + u[k // 2 + r:])))
                add(case("N run: both k=%d r=%d" % (k, r), record(n + u[r:], u[:-r] + n)))
        for k in (30, LDS_H + 2):
            u = rand_seq(rng, k)
            s = record(u, u, "ACGTA")
            for letters in ("acgt", "RYKMSWBDHV", "nXx-*"):
                b = list(s)
                for x in rng.choice(k, size=6, replace=False):
                    b[int(x)] = letters[int(rng.integers(0, len(letters)))]
                for x in rng.choice(k, size=6, replace=False):
                    b[len(s) - 1 - int(x)] = letters[int(rng.integers(0, len(letters)))]
                add(case("letters %s k=%d" % (letters, k), "".join(b)))
                add(case("letters %s k=%d end_len" % (letters, k), "".join(b), 25))
        # identity m / n: N of seq1 against a base scores as a match and is not an equal base
        for m, n in IDENT_FRACTIONS:
            sc = (10, 16, 32, 32) if n >= 7 else (5, 4, 8, 2)
            u = rand_seq(rng, n)
            v = list(u)
            for x in rng.choice(np.arange(1, n), size=n - m, replace=False):
                v[int(x)] = "N"
            for thr in IDENT_THRESHOLDS:
                add(case("identity %d/%d at %r" % (m, n, thr), record("".join(v), u), 0, params(sc, thr, 1)), int(m / n >= thr))
        u = rand_seq(rng, 20)
        for ml, f in ((20, 1), (21, 0), (0, 1), (-1, 0)):        # the comparison is unsigned: -1 finds nothing
            add(case("min_len %d at end1 20" % ml, record(u, u), 0, params(None, 0.7, ml)), f)
        return cases, found
    return cached("alphabet", build)


def check_alphabet(itr_search):
    cases, found = alphabet()
    got = run(itr_search, cases)
    assert_rows(got, twin("alphabet", cases), cases, "alphabet and thresholds")
    for c, f, r in zip(cases, found, got):
        assert f is None or int(r[5]) == f, (c[0], r.tolist())
    return len(cases)


# ------------------------------------------------------------------------------------------------------------------------------
# lengths
# ------------------------------------------------------------------------------------------------------------------------------
WHOLE_LS = (0, 1, 2, 3, 12, 13, 14, 15)
END_LENS = (1, 7, 39, 40, 41, 63, 64, 65, 499, 500, 501, 600)


def palindrome(rng, L, sub=0):
    """L bases whose second half is the reverse complement of the first (odd L: one base between), `sub` substitutions"""
    u = rand_seq(rng, L // 2)
    v = list(u)
    for x in rng.integers(0, max(1, L // 2), size=sub if L >= 2 else 0):
        v[int(x)] = _OTHER[v[int(x)]]
    return u + ("A" if L & 1 else "") + revcomp("".join(v))


def lengths():
    def build():
        rng = np.random.default_rng(9105)
        cases = [case("whole L=%d" % L, palindrome(rng, L)) for L in WHOLE_LS]
        for e in END_LENS:
            for L in sorted({max(0, e - 1), e, e + 1, (3 * e) // 2, 2 * e - 1, 2 * e, 2 * e + 1, 3 * e + 5}):
                for sub in (0, 2):
                    cases.append(case("end_len=%d L=%d sub=%d" % (e, L, sub), palindrome(rng, L, sub), e))
        return cases
    return cached("lengths", build)


def check_lengths(itr_search):
    cases = lengths()
    assert_rows(run(itr_search, cases), twin("lengths", cases), cases, "lengths")
    return len(cases)


# ------------------------------------------------------------------------------------------------------------------------------
# bands: seeded records whose h lies around 64, 128 and 500
# ------------------------------------------------------------------------------------------------------------------------------
def bands(n=1500):
    def build():
        rng = np.random.default_rng(9106)
        halves = (list(range(STRIP - 4, STRIP + 7)) + list(range(2 * STRIP - 4, 2 * STRIP + 5)) + list(range(MAX_H - 5, MAX_H + 4)))
        def draw(k):
            half = int(halves[int(rng.integers(0, len(halves)))])
            L = 2 * half + int(rng.integers(0, 2))
            t = rand_seq(rng, half - int(rng.integers(0, 4)))
            a = casegen._mut_indel(rng, t, float(rng.choice([0, .05, .1, .2, .3])), float(rng.choice([0, 0, .03, .08])))
            if rng.random() < 0.1:
                a = rand_seq(rng, len(a))
            a = a[:L - len(t)]
            s = t + rand_seq(rng, L - len(t) - len(a)) + revcomp(a)
            if rng.random() < 0.15:
                x = int(rng.integers(0, len(s)))
                s = s[:x] + "N" * min(len(s) - x, int(rng.integers(1, 12))) + s[x + 12:]
                s = (s + rand_seq(rng, L))[:L]
            assert len(s) == L
            return case("band #%d L=%d" % (k, L), s, 0, params(BAND_SCORINGS[k % 4]))

        cases = [draw(k) for k in range(n)]
        for _round in range(20):
            # a record whose traceback runs a gap into the matrix edge (seen with gap_extend 1 only) is drawn again: the tool's
            # stale state would matter there (flags bit 0), and the kernel is held to the clean formulation
            flagged = np.flatnonzero(run(twin_search, cases)[:, 7])
            if flagged.size == 0:
                break
            for k in flagged:
                cases[int(k)] = draw(int(k))
        else:
            raise AssertionError("band records keep running gaps into the matrix edge")
        return cases
    return cached(("bands", n), build)


def check_bands(itr_search):
    cases = bands()
    assert_rows(run(itr_search, cases), twin("bands", cases), cases, "bands")
    return len(cases)


# ------------------------------------------------------------------------------------------------------------------------------
# every short record alone, and beside a record that moves the batch to the store in HBM; one batch in three orders
# ------------------------------------------------------------------------------------------------------------------------------
def all_families():
    """[(name, cases)] of every family above (the slot batches repeat records of a pool: see slot_batches)"""
    return [("closed_form", closed_form()[0]), ("seams", seams()), ("ties", ties()), ("alphabet", alphabet()[0]), ("lengths", lengths()),
            ("bands", bands()), ("slots", slot_pool())]


def short_groups():
    """{(end_len, parameters): the records with h <= ITR_LDS_H of every family} -- and the record of h = ITR_LDS_H + 1 each group
    meets (an end_len up to ITR_LDS_H keeps every h at or below it: such a group has none)"""
    def build():
        groups = {}
        for _name, cases in all_families():
            for c in cases:
                if 0 < h_of(c) <= LDS_H:
                    groups.setdefault((c[2], c[3]), []).append(c)
        rng = np.random.default_rng(9107)
        u = rand_seq(rng, LDS_H + 1)
        return groups, record(u, u[:40] + _OTHER[u[40]] + u[41:])
    return cached("short_groups", build)


def check_path_equivalence(itr_search):
    groups, long_rec = short_groups()
    n = n_hbm = 0
    for (e, p), cases in groups.items():
        seqs = [c[1] for c in cases]
        alone = np.asarray(itr_search(seqs, e, **kw_of(p)))
        assert_rows(alone, run(twin_search, cases), cases, "short records alone")
        n += len(seqs)
        if e == 0 or e > LDS_H:
            first = np.asarray(itr_search([long_rec] + seqs, e, **kw_of(p)))
            last = np.asarray(itr_search(seqs + [long_rec], e, **kw_of(p)))
            assert_rows(first[1:], alone, cases, "short records after one of h = %d" % (LDS_H + 1))
            assert_rows(last[:-1], alone, cases, "short records before one of h = %d" % (LDS_H + 1))
            assert first[0].tolist() == last[-1].tolist() and first[0][1] > 0
            n_hbm += len(seqs)
    return n, n_hbm


def order_batch():
    def build():
        cases = [c for _n, cs in all_families() for c in cs if c[2] == 0 and c[3] == DEF]
        rng = np.random.default_rng(9108)
        pick = rng.permutation(len(cases))[:240]
        return [cases[int(k)] for k in pick]
    return cached("order_batch", build)


def check_order(itr_search):
    cases = order_batch()
    hs = np.asarray([h_of(c) for c in cases])
    asc = np.argsort(hs, kind="stable")
    inter = np.empty_like(asc)
    inter[0::2], inter[1::2] = asc[:(len(asc) + 1) // 2], asc[::-1][:len(asc) // 2]      # shortest, longest, second shortest, ...
    base = twin("order", cases)
    for name, perm in (("ascending", asc), ("descending", asc[::-1]), ("interleaved", inter)):
        got = run(itr_search, [cases[int(k)] for k in perm])
        assert_rows(got, base[perm], [cases[int(k)] for k in perm], "order " + name)
    return len(cases), int(hs.min()), int(hs.max())


# ------------------------------------------------------------------------------------------------------------------------------
# slots that several records pass through
# ------------------------------------------------------------------------------------------------------------------------------
def slot_pool():
    """the distinct records of the two slot batches: h = 500 repeats with planted indels, h = 65 .. 70, and up to 80 bases"""
    def build():
        rng = np.random.default_rng(9109)
        pool = []
        for k in range(10):
            u = rand_seq(rng, MAX_H)
            x = int(rng.integers(100, 400))
            n_ins = int(rng.integers(1, 4))
            v = u[:x] + rand_seq(rng, n_ins) + u[x:]
            a, b = (u + rand_seq(rng, n_ins), v) if k & 1 else (v, u + rand_seq(rng, n_ins))
            pool.append(case("slot long #%d" % k, record(a, b)))
        for k in range(12):
            h = LDS_H + 1 + k % 6
            u = rand_seq(rng, h)
            x = int(rng.integers(10, h - 10))
            pool.append(case("slot mid #%d h=%d" % (k, h), record(u, u[:x] + _OTHER[u[x]] + u[x + 1:], "A" * (k & 1))))
        for s in casegen.make_itr_cases(9110, 400):
            pool.append(case("slot short", s[:80]))
        return pool
    return cached("slot_pool", build)


def slot_batches():
    """(HBM batch, LDS batch).  Record k runs in slot k mod (blocks x waves), after record k - blocks x waves: the HBM batch
    alternates long and short records ALONG a slot as well as across the slots; the LDS batch ends with 7 short records that follow
    records of 80 bases through slots 0 .. 6."""
    def build():
        pool = slot_pool()
        longs = [c for c in pool if c[0].startswith("slot long")]
        mids = [c for c in pool if c[0].startswith("slot mid")]
        shorts = sorted((c for c in pool if c[0] == "slot short"), key=lambda c: -len(c[1]))
        slots = HBM_BLOCKS * WAVES
        hbm = []
        for k in range(4 * HBM_BLOCKS + 5):
            hbm.append(longs[k % len(longs)] if (k + k // slots) & 1 == 0 else mids[k % len(mids)])
        slots = LDS_BLOCKS * WAVES
        lds = [shorts[k % 40] if k < 7 else shorts[k % len(shorts)] for k in range(slots)]
        lds += [shorts[-1 - k] for k in range(4 * LDS_BLOCKS + 7 - slots)]
        return hbm, lds
    return cached("slot_batches", build)


def check_slots(itr_search, which):
    cases = slot_batches()[which]
    pool = slot_pool()
    rows = dict((id(c), r) for c, r in zip(pool, twin("slot_pool", pool)))
    exp = np.asarray([rows[id(c)] for c in cases])
    seqs = [c[1] for c in cases]
    once = np.asarray(itr_search(seqs, 0, **kw_of(DEF)))
    assert_rows(once, exp, cases, "slot batch in one call")
    pieces = np.concatenate([np.asarray(itr_search(seqs[k:k + 100], 0, **kw_of(DEF))) for k in range(0, len(seqs), 100)])
    assert_rows(pieces, once, cases, "slot batch in pieces of 100")
    return len(cases)


# ------------------------------------------------------------------------------------------------------------------------------
# guards: the device entry's max_h promise, bad arguments, empty batches
# ------------------------------------------------------------------------------------------------------------------------------
GUARD_MAX_H = (0, LDS_H - 1, LDS_H, LDS_H + 1, MAX_H - 1, MAX_H, 10000)


def guard_batch():
    def build():
        rng = np.random.default_rng(9111)
        cases = [case("guard empty", "")]
        for h in (1, 7, 20, LDS_H - 1, LDS_H, LDS_H + 1, LDS_H + 2, 2 * STRIP, 2 * STRIP + 1, MAX_H - 1, MAX_H, MAX_H + 1, 7, LDS_H):
            u = rand_seq(rng, h)
            x = h // 2
            cases.append(case("guard h=%d" % min(h, MAX_H), record(u, u[:x] + _OTHER[u[x]] + u[x + 1:] if h > 12 else u, "A" * (h & 1))))
        return cases
    return cached("guard_batch", build)


def guard_expected(max_h):
    cases = guard_batch()
    exp = np.array(twin("guard", cases))
    for k, c in enumerate(cases):
        if h_of(c) > max_h:
            exp[k] = SKIPPED_ROW
    return exp


def check_max_h(dev_search):
    """dev_search(seqs, end_len, max_h) -> rows of hite_itr_search_dev"""
    cases = guard_batch()
    seqs = [c[1] for c in cases]
    got = {}
    for mh in GUARD_MAX_H:
        got[mh] = np.asarray(dev_search(seqs, 0, mh))
        assert_rows(got[mh], guard_expected(mh), cases, "max_h = %d" % mh)
    short = [k for k, c in enumerate(cases) if h_of(c) <= LDS_H]
    assert len(short) >= 6 and np.array_equal(got[LDS_H][short], got[LDS_H + 1][short])
    return len(cases)


# ------------------------------------------------------------------------------------------------------------------------------
# the tool's own answers (tests/golden/itr_limits.json.gz, written by oracle/gen_golden.py itr_limits)
# ------------------------------------------------------------------------------------------------------------------------------
FIXTURE_RUNS = ((0.7, 7), (0.8, 10))       # -i / -l of the reference's call, and the tool's defaults


def compose(c):
    """the record the stage composes from its ends, handed over whole"""
    s, e = c[1], c[2]
    if e <= 0:
        return s
    e = min(len(s), e)
    return s[:e] + s[len(s) - e:]


def fixture_cases():
    """[(label, record)]: a thinned set of the closed-form, seam, alphabet and length cases at the tool's default scoring, over
    ACGTN only (the tool compares other letters literally), no shorter than 2 bases"""
    out = []
    for name, cases, step in (("closed_form", closed_form()[0], 1), ("seams", seams(), 1), ("alphabet", alphabet()[0], 1),
                              ("lengths", lengths(), 2)):
        kept = [c for c in cases if c[3][2:] == DEF[2:] and set(c[1]) <= set("ACGTN") and not c[0].startswith(("identity", "min_len"))]
        seen = set()
        for c in kept[::step]:
            s = compose(c)
            if len(s) >= 2 and s not in seen:
                seen.add(s)
                out.append((c[0], s))
    return out


def parse_itr_header(line, L):
    """'>name ITR(1,e1)..(L,p) Length itr=x' -> (x, e1, L - p + 1)"""
    body = line.split(" ITR(")[1]
    first, rest = body.split(")..(")
    second = rest.split(")")[0]
    e1, (l2, p2) = int(first.split(",")[1]), [int(x) for x in second.split(",")]
    assert int(first.split(",")[0]) == 1 and l2 == L, line
    return int(line.split("Length itr=")[1]), e1, L - p2 + 1


def check_fixture(itr_search, g):
    """the tool's found / "Length itr=" / end1 / end2 of every record of the fixture, at both -i / -l"""
    cases = fixture_cases()
    assert [s for _l, s in cases] == g["seqs"], "tests/golden/itr_limits.json.gz is not of these cases: rerun oracle/gen_golden.py itr_limits"
    n_found = 0
    for (ident, ml), res in zip(FIXTURE_RUNS, g["runs"]):
        rows = np.asarray(itr_search(g["seqs"], 0, min_identity=ident, min_len=ml))
        assert int(rows[:, 7].max()) == 0
        got = [[1, int(r[6]), int(r[1]), int(r[2])] if r[5] else [0, -1, 0, 0] for r in rows]
        bad = [k for k in range(len(got)) if got[k] != res[k]]
        assert not bad, "-i %r -l %d: %d records differ from the tool, first %s: %s, the tool %s" % (
            ident, ml, len(bad), cases[bad[0]][0], got[bad[0]], res[bad[0]])
        n_found += sum(r[0] for r in res)
    return len(cases), n_found
