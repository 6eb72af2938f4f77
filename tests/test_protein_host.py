"""CPU-only checks of the translated protein search (hite_amd/csrc/hite_prot.hip): the codon and score tables, the seed rule and the
ungapped extension are cut out of the .hip file between `// >>> prot_tables` / `// <<< prot_tables`, compiled for the host and
compared with the twin (tests/protein_twin.py + tests/protein_twin.c); the twin's known answers are checked by hand; task formation,
the HSP filter and the E-value threshold are host code of the library and run through its entry points."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import protein_twin as T  # noqa: E402

PRELUDE = r"""
#include <stdint.h>
#include <algorithm>
#define __device__
#define __forceinline__ inline
using std::min;
using std::max;
"""


def _block(path, name):
    src = open(path).read()
    m = re.search(r"// >>> %s.*?\n(.*?)// <<< %s" % (name, name), src, re.S)
    assert m, name
    return m.group(1)


def _build(tmp_path, name, body, wrapper):
    """as tests/test_host_compiled.py builds its blocks"""
    cpp = tmp_path / (name + ".cpp")
    so = tmp_path / (name + ".so")
    cpp.write_text(PRELUDE + body + wrapper)
    extra = os.environ.get("HITE_HOST_CXXFLAGS", "").split()
    subprocess.run(["g++", "-O2", "-shared", "-fPIC"] + extra + ["-o", str(so), str(cpp)], check=True)
    return C.CDLL(str(so))

WRAPPER = r"""
static int8_t g_tab[PROT_TABW * PROT_TABW];
static bool g_ready = false;
static const int8_t *host_tab() {
    if (!g_ready) {
        for (int a = 0; a < PROT_TABW; a++) for (int b = 0; b < PROT_TABW; b++)
            g_tab[a * PROT_TABW + b] = (a < PROT_NCODE && b < PROT_NCODE) ? (int8_t)prot_score(a, b) : (int8_t)0;
        g_ready = true;
    }
    return g_tab;
}
extern "C" int host_codon(int c0, int c1, int c2, int comp) {
    return prot_codon(prot_base_code((uint8_t)c0, comp != 0), prot_base_code((uint8_t)c1, comp != 0), prot_base_code((uint8_t)c2, comp != 0));
}
extern "C" int host_letter(int c) { return prot_letter_code((uint8_t)c); }
extern "C" int host_score(int a, int b) { return prot_score(a, b); }
extern "C" int host_seed_key(int a, int b, int c, int d) { return prot_seed_key(a, b, c, d); }
extern "C" int host_ungapped(const uint8_t *x, int lx, int i, const uint8_t *y, int ly, int j, int *seg) {
    return prot_ungapped(x, lx, i, y, ly, j, host_tab(), seg, seg + 1);
}
extern "C" int host_const(int k) {
    const int v[] = {PROT_XDROP, PROT_UNGAPPED_MIN, PROT_DIAG_JOIN, PROT_SPLIT, PROT_BAND_LO, PROT_BAND_HI, PROT_GAP_OPEN, PROT_GAP_EXT,
                     PROT_BUCKETS, PROT_MAX_AA};
    return v[k];
}
"""


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    body = _block(os.path.join(ROOT, "hite_amd", "csrc", "hite_prot.hip"), "prot_tables")
    return _build(tmp_path_factory.mktemp("prot"), "prot", "#define PROT_TAB static const\n" + body, WRAPPER)


@pytest.fixture(scope="module")
def so():
    import __graft_entry__ as g

    g.build()
    return C.CDLL(os.path.join(ROOT, "hite_amd", "libhite_gpu.so"))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_constants_match_the_twin(host):
    assert [host.host_const(k) for k in range(10)] == [T.XDROP, T.UNGAPPED_MIN, T.DIAG_JOIN, T.SPLIT, T.BAND_LO, T.BAND_HI, 12, 1, 20 ** 4, T.MAX_AA]


def test_codons_all_64_and_N_both_strands(host):
    comp = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}
    n = 0
    for a in "ACGTN":
        for b in "ACGTN":
            for c in "ACGTN":
                cod = a + b + c
                want = T.CODON.get(cod, "X")
                for s in (cod, cod.lower()):
                    assert T.LETTERS[host.host_codon(ord(s[0]), ord(s[1]), ord(s[2]), 0)] == want, cod
                # the minus strand reads the complement of the bytes it is handed (the kernel hands them over back to front)
                rc = "".join(comp[x] for x in cod)
                assert T.LETTERS[host.host_codon(ord(a), ord(b), ord(c), 1)] == T.CODON.get(rc, "X")
                n += 1
    assert n == 125
    # by hand
    assert T.CODON["ATG"] == "M" and T.CODON["TGG"] == "W" and T.CODON["TAA"] == "*" and T.CODON["TAG"] == "*" and T.CODON["TGA"] == "*"
    assert T.CODON["GCC"] == "A" and T.CODON["AAA"] == "K" and T.CODON["CAT"] == "H"
    assert T.translate6("ATGGCCTGANN") == ["MA*", "WPX", "GLX", "XQA", "XRP", "SGH"]
    assert T.translate6("atggcctga") == T.translate6("ATGGCCTGA")
    assert T.translate6("AC") == [""] * 6 and T.translate6("") == [""] * 6


def test_scores_all_25x25_letter_pairs(host):
    letters = "ARNDCQEGHILKMFPSTWYVBZX*U"
    assert len(letters) == 25
    for a in letters:
        ca = T.STOP if a == "*" else host.host_letter(ord(a))          # the frame side: '*' is a stop there
        assert ca == int(T.encode_frame(a)[0])
        for b in letters:
            cb = host.host_letter(ord(b))                                # the library side: everything non-standard is X
            assert cb == int(T.encode(b)[0]) and cb == host.host_letter(ord(b.lower()))
            assert host.host_score(ca, cb) == T.score(ca, cb), (a, b)
    code = {ch: k for k, ch in enumerate(T.LETTERS)}
    by_hand = {("W", "W"): 11, ("A", "A"): 4, ("C", "C"): 9, ("E", "K"): 1, ("D", "E"): 2, ("W", "C"): -2, ("G", "I"): -4, ("X", "A"): -1,
               ("X", "X"): -1, ("*", "A"): -4, ("*", "X"): -4, ("*", "*"): -4, ("F", "Y"): 3, ("H", "Y"): 2, ("L", "I"): 2, ("V", "I"): 3}
    for (a, b), v in by_hand.items():
        assert T.score(code[a], code[b]) == v and T.score(code[b], code[a]) == v


def test_seed_rule(host):
    rng = np.random.default_rng(3)
    for _ in range(3000):
        c = rng.integers(0, 22 if rng.random() < 0.3 else 4, 4)
        assert host.host_seed_key(*[int(v) for v in c]) == T.seed_key(c)
    assert T.seed_key([0, 0, 0, 0]) == -1 and T.seed_key([0, 1, 0, 1]) == -1 and T.seed_key([0, 1, 2, 0]) == 440
    assert T.seed_key([19, 19, 18, 17]) == 19 * 8000 + 19 * 400 + 18 * 20 + 17 and T.seed_key([0, 1, 2, 20]) == -1


def test_ungapped_random_diagonals(host):
    rng = np.random.default_rng(5)
    n_surv = 0
    for case in range(4000):
        lx, ly = int(rng.integers(4, 120)), int(rng.integers(4, 120))
        x = rng.integers(0, 22, lx).astype(np.uint8)
        y = rng.integers(0, 20, ly).astype(np.uint8)
        i, j = int(rng.integers(0, lx - 3)), int(rng.integers(0, ly - 3))
        # a diverged copy of y's neighbourhood on the diagonal, so that extensions are long, short and cut by the ends
        div = (0.0, 0.2, 0.5, 0.9)[case % 4]
        for k in range(-min(i, j), min(lx - i, ly - j)):
            if rng.random() >= div:
                x[i + k] = y[j + k]
        x[i:i + 4] = y[j:j + 4]
        seg = np.zeros(2, dtype=np.int32)
        s = host.host_ungapped(_p(x), lx, i, _p(y), ly, j, _p(seg))
        want = T.ungapped(x, i, y, j)
        assert (s, int(seg[0]), int(seg[1])) == want
        n_surv += s >= T.UNGAPPED_MIN
    assert 500 < n_surv < 3500


def _codes(s):
    return T.encode_frame(s)


def test_ungapped_by_hand():
    # W W W W seed (44) + A/A (4) to the right, then sixteen times -1 (X) and W W: a drop of exactly 16 goes on and the two W lift the
    # running sum to 4 - 16 + 22 = 10
    x = _codes("WWWWA" + "X" * 16 + "WW")
    y = _codes("WWWWA" + "A" * 16 + "WW")
    assert T.ungapped(x, 0, y, 0) == (44 + 10, 0, 22)
    # seventeen: the extension stops before the W; the segment ends at the A
    x = _codes("WWWWA" + "X" * 17 + "WW")
    y = _codes("WWWWA" + "A" * 17 + "WW")
    assert T.ungapped(x, 0, y, 0) == (48, 0, 4)
    # the same to the left
    assert T.ungapped(_codes("WW" + "X" * 16 + "AWWWW"), 19, _codes("WW" + "A" * 16 + "AWWWW"), 19) == (54, 0, 22)
    assert T.ungapped(_codes("WW" + "X" * 17 + "AWWWW"), 20, _codes("WW" + "A" * 17 + "AWWWW"), 20) == (48, 19, 23)
    # to the left, cut by the protein's start: frame position 2 is protein position 0
    x, y = _codes("GGCWWWW"), _codes("CWWWW")
    assert T.ungapped(x, 3, y, 1) == (53, 2, 6)
    # scores 40 and 41: A A A A C L (4 * 4 + 9 + 4 = 29) ... by seeds of standard residues: ARND = 4 + 5 + 6 + 6 = 21
    assert T.ungapped(_codes("ARNDCCA"), 0, _codes("ARNDCCA"), 0)[0] == 21 + 9 + 9 + 4
    assert T.ungapped(_codes("ARNDCCAS"), 0, _codes("ARNDCCAT"), 0) == (43 + 1, 0, 7)


def test_gapped_by_hand():
    big = 1 << 40
    # (three columns around one gap can never be the best alignment: 11 - 12 + 11 < 11; seven columns are the smallest that is)
    # one gap in the frame (F): W W W - C H P against W W W A C H P: 33 - 12 + (9 + 8 + 7); the diagonal after W W W only loses
    x, y = _codes("WWWCHP"), _codes("WWWACHP")
    assert T.gapped(x, 0, 5, y, -big, big) == (45, 0, 0, 5, 6, 6, 7)
    # one gap in the protein (E)
    assert T.gapped(y, 0, 6, x, -big, big) == (45, 0, 0, 6, 5, 6, 7)
    # the same inside the band's diagonals 0 .. 1; a band of diagonal 0 alone: the W run (33) is the first maximum (C/A = 0 ties it later)
    assert T.gapped(x, 0, 5, y, 0, 1) == (45, 0, 0, 5, 6, 6, 7)
    assert T.gapped(x, 0, 5, y, 0, 0) == (33, 0, 0, 2, 2, 3, 3)
    # rows 3 .. 5 only: C H P on diagonal 1
    assert T.gapped(x, 3, 5, y, -big, big) == (24, 3, 4, 5, 6, 3, 3)
    # best cell: the first maximum in row-major order ((0,0) and (2,0) both score 11; then (0,0) and (0,2))
    assert T.gapped(_codes("WAW"), 0, 2, _codes("W"), -big, big) == (11, 0, 0, 0, 0, 1, 1)
    assert T.gapped(_codes("W"), 0, 0, _codes("WAW"), -big, big) == (11, 0, 0, 0, 0, 1, 1)
    # H prefers the gap in the protein (E) to the gap in the frame (F) on a tie.  x = W W C W W, y = W W W W: the two W pairs (22 each
    # side) are joined either by skipping C in the frame (E, one column, -12) = 22 - 12 + 22 = 32 ... the diagonal through C (W/C = -2)
    # does better on the main diagonal: W W C W against W W W W = 11 + 11 - 2 + 11 = 31 < 32.  Columns: W W C(gap) W W = 5, identical 4
    assert T.gapped(_codes("WWCWW"), 0, 4, _codes("WWWW"), -big, big) == (32, 0, 0, 4, 3, 4, 5)
    # stops and X inside: * scores -4, X scores -1, neither is identical to anything
    assert T.gapped(_codes("WW*WW"), 0, 4, _codes("WWAWW"), -big, big) == (40, 0, 0, 4, 4, 4, 5)
    assert T.gapped(_codes("WWXWW"), 0, 4, _codes("WWXWW".replace("X", "B")), -big, big) == (43, 0, 0, 4, 4, 4, 5)
    # nothing positive
    assert T.gapped(_codes("G"), 0, 0, _codes("I"), -big, big) == (0, 0, 0, 0, 0, 0, 0)


def test_gapped_longer_by_hand():
    big = 1 << 40
    # three P in the frame: the diagonal through them (W/P = -4 each: 44 - 12 + 55) beats the gap of three (44 - 14 + 55)
    assert T.gapped(_codes("WWWWPPPWWWWW"), 0, 11, _codes("WWWWWWWWWWWW"), -big, big) == (87, 0, 0, 11, 11, 9, 12)
    # two A in the frame and a protein two shorter: a gap of two in the protein, 44 - 13 + 66
    assert T.gapped(_codes("WWWWAAWWWWWW"), 0, 11, _codes("WWWWWWWWWW"), -big, big) == (97, 0, 0, 11, 9, 10, 12)


def test_smin_rounding_boundary(so):
    so.hite_protein_smin.argtypes = [C.c_int64, C.c_int64, C.c_double, C.c_void_p]
    s = C.c_int32(0)
    # by hand: m = n = 1: E(S) = 0.041 exp(-0.267 S); E(10) is exactly representable as the threshold
    e10 = 0.041 * math.exp(-2.67)
    assert T.smin(1, 1, e10) == 10 and T.smin(1, 1, math.nextafter(e10, 0.0)) == 11 and T.smin(1, 1, math.nextafter(e10, math.inf)) == 10
    # 1 000 residues against 2.9 M at 1e-20: ln(1000 * 2.9e6 * 0.041 / 1e-20) / 0.267 = (ln 1.189e28) / 0.267 = 64.646 / 0.267 = 242.1
    assert T.smin(1000, 2_900_000, 1e-20) == 243
    rng = np.random.default_rng(11)
    for k in range(400):
        m, n = int(rng.integers(1, 70000)), int(rng.integers(1, 5_000_000))
        S = int(rng.integers(1, 400))
        e = T.evalue_of(m, n, S)
        for ev, want in ((e, S), (math.nextafter(e, 0.0), S + 1), (math.nextafter(e, math.inf), S)):
            assert so.hite_protein_smin(m, n, ev, C.byref(s)) == 0
            assert s.value == T.smin(m, n, ev) == want
    assert so.hite_protein_smin(0, 5, 1e-20, C.byref(s)) == 0 and s.value == 1
    assert so.hite_protein_smin(5, 5, 0.0, C.byref(s)) == -1


def _tasks(so, surv, frame_len, cap=None):
    n = len(surv)
    col = lambda k: np.ascontiguousarray([s[k] for s in surv], dtype=np.int32)  # noqa: E731
    fl = np.ascontiguousarray(frame_len, dtype=np.int32)
    cap = 2 * n + 1 if cap is None else cap
    out = [np.full(cap + 1, -7, dtype=np.int32) for _ in range(5)]
    n_out = C.c_int64(0)
    rc = so.hite_protein_tasks(C.c_int64(n), _p(col(0)), _p(col(1)), _p(col(2)), _p(col(3)), _p(col(4)), C.c_int64(len(fl)), _p(fl), C.c_int64(cap),
                               *[_p(o) for o in out], C.byref(n_out))
    return rc, n_out.value, out


def test_task_formation_host_entry(so):
    # by hand: one frame of 1000 residues, protein 0.  Diagonals 5 and 21 (= 5 + 16) share a cluster, 22 opens the next; segments 129
    # apart split, 128 apart do not; rows are clipped at 0 and at L_f - 1
    surv = [(0, 0, 5, 100, 120), (0, 0, 21, 248, 260), (0, 0, 21, 389, 400), (0, 0, 22, 900, 950)]
    want = [(0, 0, 5, 0, 388), (0, 0, 5, 261, 528), (0, 0, 22, 772, 999)]
    assert T.form_tasks(surv, [1000]) == want
    rc, n, out = _tasks(so, surv, [1000])
    assert rc == 0 and [tuple(int(o[k]) for o in out) for k in range(n)] == want
    rng = np.random.default_rng(21)
    for case in range(60):
        fl = [int(v) for v in rng.integers(50, 3000, 6)]
        surv = set()
        for _ in range(int(rng.integers(0, 80))):
            gf, p = int(rng.integers(0, 6)), int(rng.integers(0, 3))
            i0 = int(rng.integers(0, fl[gf] - 8))
            surv.add((gf, p, int(rng.integers(-40, 40)), i0, min(fl[gf] - 1, i0 + int(rng.integers(4, 200)))))
        surv = sorted(surv)
        want = T.form_tasks(surv, fl)
        rc, n, out = _tasks(so, surv, fl)
        assert rc == 0 and [tuple(int(o[k]) for o in out) for k in range(n)] == want
        if len(want) > 1:
            rc, n, out = _tasks(so, surv, fl, cap=len(want) - 1)
            assert rc == -4 and n == len(want) and all(int(o[len(want) - 1]) == -7 for o in out)


def test_hsp_filter_host_entry(so):
    def run(hs):
        col = lambda k: np.ascontiguousarray([h[k] for h in hs], dtype=np.int32)  # noqa: E731
        keep = np.zeros(len(hs) + 1, dtype=np.uint8)
        assert so.hite_protein_hsp_filter(C.c_int64(len(hs)), _p(col(0)), _p(col(1)), _p(col(2)), _p(col(3)), _p(col(4)), _p(keep)) == 0
        return [h for h, k in zip(hs, keep) if k]

    # by hand: (score, si, sj, ei, ej).  b shares a's start, c shares a's end, d lies inside a, e overlaps a without lying inside: stays
    a, b, c, d, e = (100, 10, 20, 60, 70), (90, 10, 20, 40, 50), (80, 30, 35, 60, 70), (70, 20, 30, 50, 60), (60, 50, 60, 90, 100)
    assert T.filter_hsps([e, d, c, b, a]) == [a, e]
    assert run([e, d, c, b, a]) == [e, a]
    rng = np.random.default_rng(2)
    for case in range(200):
        hs = []
        for _ in range(int(rng.integers(0, 12))):
            si, sj = int(rng.integers(0, 30)), int(rng.integers(0, 30))
            hs.append((int(rng.integers(40, 60)), si, sj, si + int(rng.integers(0, 30)), sj + int(rng.integers(0, 30))))
        hs = sorted(set(hs))
        assert sorted(run(hs)) == sorted(T.filter_hsps(hs))


def test_twin_search_and_exhaustive_mode_agree_on_a_planted_domain():
    rng = np.random.default_rng(9)
    import protein_cases as PC

    prots = [PC.rand_protein(rng, 150) for _ in range(3)]
    q = PC.rand_dna(rng, 200) + PC.back_translate(rng, prots[1]) + PC.rand_dna(rng, 100)
    for query in (q, PC.revcomp(q)):
        a = T.search([query], prots)
        b = T.search([query], prots, exhaustive=True)
        assert len(a) == 1 and a == b
        assert a[0][1] == 1 and a[0][5:7] == (1, 150) and a[0][8] == 150 and a[0][9] == 150
    assert T.search([q], prots)[0][2] == 3 and T.search([q], prots)[0][3:5] == (201, 650)
    assert T.search([PC.revcomp(q)], prots)[0][3:5] == (len(q) - 200, len(q) - 649)


def _dp(x, y, h_order="DEF", open_first=True):
    """the gapped definition once more, cell by cell in Python over the whole matrix, with the preferences as arguments"""
    n, m, Z = len(x), len(y), (0, 0, 0, 0, 0)          # (score, start i, start j, identical, columns)
    H = [[Z] * (m + 1) for _ in range(n + 1)]
    E = [[Z] * (m + 1) for _ in range(n + 1)]
    F = [[Z] * (m + 1) for _ in range(n + 1)]
    best, cell = Z, (0, 0)

    def gap(h, g):
        o, e = h[0] - 12, g[0] - 1
        r = (o,) + h[1:4] + (h[4] + 1,) if ((o >= e) if open_first else (o > e)) else (e,) + g[1:4] + (g[4] + 1,)
        return r if r[0] > 0 else Z

    for i in range(1, n + 1):
        for j in range(1, m + 1):
            a, b, hd = int(x[i - 1]), int(y[j - 1]), H[i - 1][j - 1]
            st = (hd[1], hd[2], hd[3], hd[4]) if hd[0] > 0 else (i - 1, j - 1, 0, 0)
            c = {"D": (hd[0] + T.score(a, b), st[0], st[1], st[2] + (a == b and a < 20), st[3] + 1),
                 "E": gap(H[i - 1][j], E[i - 1][j]), "F": gap(H[i][j - 1], F[i][j - 1])}
            h = max((c[k] for k in h_order), key=lambda t: t[0])      # the first maximum in the order of preference
            H[i][j], E[i][j], F[i][j] = (h if h[0] > 0 else Z), c["E"], c["F"]
            if h[0] > best[0]:
                best, cell = h, (i - 1, j - 1)
    return (best[0], best[1], best[2], cell[0], cell[1], best[3], best[4]) if best[0] > 0 else (0,) * 7


def test_gap_tie_rules():
    big = 1 << 40
    run = lambda x, y: T.gapped(_codes(x), 0, len(x) - 1, _codes(y), -big, big)  # noqa: E731
    # H prefers the diagonal.  Both paths score 18: A/A C/A G/C H/H C/C = 4 + 0 - 3 + 8 + 9 from (0,0) with three identical columns,
    # and A/A C/C, the G skipped (-12), H/H C/C from (0,1) with four; they meet where the diagonal move ties the gap
    assert run("ACGHC", "AACHCW") == (18, 0, 0, 4, 4, 3, 5)
    assert _dp(_codes("ACGHC"), _codes("AACHCW"), h_order="EFD") == (18, 0, 1, 4, 4, 4, 5)
    # H prefers the gap in the protein (E) to the gap in the frame (F).  Both paths score 34 = 15 - 12 + 31: S/S W/W, the frame's S
    # skipped, C/C W/W W/W from (0,3); and W/W S/S, the protein's W skipped, C/C W/W W/W from (1,2)
    assert run("SWSCWW", "SWWSWCWW") == (34, 0, 3, 5, 7, 5, 6)
    assert _dp(_codes("SWSCWW"), _codes("SWWSWCWW"), h_order="DFE") == (34, 1, 2, 5, 7, 5, 6)
    # a gap prefers opening to extending (the other preference reports another path for this pair)
    assert run("AWWWSCW", "SWWCASAW") == (24, 0, 0, 6, 7, 4, 8)
    assert _dp(_codes("AWWWSCW"), _codes("SWWCASAW"), open_first=False) == (24, 2, 1, 6, 7, 4, 7)
    # the C loops against the Python form of the definition
    rng = np.random.default_rng(4)
    for case in range(300):
        al = "WWCAS" if case % 2 else T.LETTERS
        x = "".join(al[k] for k in rng.integers(0, len(al), int(rng.integers(1, 14))))
        y = "".join(al[k] for k in rng.integers(0, len(al) - 1 if al is T.LETTERS else len(al), int(rng.integers(1, 14))))
        assert run(x, y) == _dp(_codes(x), T.encode(y)), (x, y)
