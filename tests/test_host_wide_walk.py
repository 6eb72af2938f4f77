"""The lane predicate of the wide fall-back's traceback by runs (hite_amd/csrc/hite_align.hip, block `wide_walk_probe`) compiled for
the HOST: a loop over 64 "lanes" drives it the way align_wide_tb_runs_kernel does -- fullt kept in two arrays of 64 and shifted
along the "lanes" by the columns the last trip moved by, lane q gathers three words of column j - q, a "ballot" of the flags and a
count of trailing ones give the diagonal or the left run, anything else at lane 0 takes the general step -- and the steps (i, j, op)
it takes are compared one by one with the column-by-column rule of align_wide_tb_kernel, restated here
in scalar code:
   * random fullt / bit matrices of 2, 4 and 64 words a column, with sparse gaps (the diagonal bit set in 99 % of the cells) and dense
     ones (50 %, 10 %), bands that move by 0 / 4 / 8 rows every fourth column, walks that fail because they leave the band or find no
     stop bit;
   * hand-made matrices: an up run directly behind a left run and the reverse (which no pair of sequences produces, see
     wide_walk_cases.py), runs of exactly 63 / 64 / 65 / 128 / 129 steps, runs that end because i or j reaches 0 inside a trip.
A part of them goes through a stand-alone program of the same code built with -fsanitize=address,undefined that keeps every array in
a heap buffer of exactly its size."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_host_compiled import PRELUDE, _block, _build  # noqa: E402

D, U, L = 0, 1, 2

DRIVER = r"""
#include <string.h>
#include <stdio.h>
#include <stdlib.h>
// one column's words: nw of diagonal bits, then nw of up bits; fullt[j] = row of the band's first bit; columns 1 .. n (column 0 exists
// and is never read)
struct Steps {
    int32_t *out; long cap, n;
    void put(int i, int j, int op) { if (n < cap) { out[3 * n] = i; out[3 * n + 1] = j; out[3 * n + 2] = op; } n++; }
};
// the general step of both kernels at column j; -> false: the walk fails
static bool general_step(int &i, int &j, int nw, const int32_t *ft, const uint32_t *fb, Steps &S) {
    const uint32_t *col = fb + (size_t)j * 2 * nw;
    const int kb = i - ft[j] - 1;
    if ((unsigned)kb >= (unsigned)(32 * nw)) return false;
    int ps = kb;
    while (ps >= 0 && !(((col[ps >> 5] | ~col[nw + (ps >> 5)]) >> (ps & 31)) & 1u)) ps--;
    if (ps < 0) return false;
    int nup = kb - ps;
    if (nup > i) nup = i;
    for (int x = 0; x < nup; x++) S.put(i - x, j, 1);
    i -= nup;
    if (i > 0) {
        if ((col[ps >> 5] >> (ps & 31)) & 1u) { S.put(i, j, 0); i--; j--; }
        else { S.put(i, j, 2); j--; }
    }
    return true;
}
// the column-by-column rule (align_wide_tb_kernel): diagonal where the cell's diagonal bit is set, else the general step
static bool walk_columns(int m, int n, int nw, const int32_t *ft, const uint32_t *fb, Steps &S) {
    int i = m, j = n;
    while (i > 0 && j > 0) {
        const int kb = i - ft[j] - 1;
        if ((unsigned)kb >= (unsigned)(32 * nw)) return false;
        if ((fb[(size_t)j * 2 * nw + (kb >> 5)] >> (kb & 31)) & 1u) { S.put(i, j, 0); i--; j--; }
        else if (!general_step(i, j, nw, ft, fb, S)) return false;
    }
    return true;
}
// by runs (align_wide_tb_runs_kernel): 64 lanes over the probe
static bool walk_runs(int m, int n, int nw, const int32_t *ft, const uint32_t *fb, Steps &S, long *trips) {
    int i = m, j = n;
    // fullt in two "registers" of 64 lanes, as the kernel keeps it: loaded once, then shifted along the lanes by the columns the last
    // trip moved by, the new tb read from memory; fullt is read nowhere else
    int ta[64], tb[64], xa[64], moved = 0;
    for (int q = 0; q < 64; q++) { ta[q] = ft[wide_walk_col(j, q)]; tb[q] = ft[wide_walk_col(j - 64, q)]; }
    while (i > 0 && j > 0) {
        for (int q = 0; q < 64; q++) {
            const int src = wide_walk_shift_lane(q, moved);
            xa[q] = wide_walk_shift_from_a(q, moved) ? ta[src] : tb[src];
        }
        for (int q = 0; q < 64; q++) { ta[q] = xa[q]; tb[q] = ft[wide_walk_col(j - 64, q)]; }
        moved = 0;
        unsigned long long bd = 0, bl = 0;
        for (int q = 0; q < 64; q++) {
            const int jq = wide_walk_col(j, q);
            const int t = ta[q];
            if (j - q > 0 && t != ft[jq]) { S.put(-1, -1, -1); return false; }      // a shift gone wrong: a step no walk takes
            const uint32_t *col = fb + (size_t)jq * 2 * nw;
            const int wd = wide_walk_word(i - q - t - 1, nw), wr = wide_walk_word(i - t - 1, nw);
            const uint32_t f = wide_walk_lane(i, j, q, t, col[wd], col[wr], col[nw + wr], nw);
            if (f & WALK_DIAG) bd |= 1ull << q;
            if (f & WALK_LEFT) bl |= 1ull << q;
        }
        ++*trips;
        int r = wide_walk_run(bd);
        if (r > 0) { for (int x = 0; x < r; x++) S.put(i - x, j - x, 0); i -= r; j -= r; moved = r; continue; }
        r = wide_walk_run(bl);
        if (r > 0) { for (int x = 0; x < r; x++) S.put(i, j - x, 2); j -= r; moved = r; continue; }
        const int j0 = j;
        if (!general_step(i, j, nw, ft, fb, S)) return false;
        moved = j0 - j;
    }
    return true;
}
// -> steps taken, or -(steps + 1) when the walk fails; the first `cap` steps are written to out
extern "C" long host_walk(int runs, int m, int n, int nw, const int32_t *ft, const uint32_t *fb, int32_t *out, long cap, long *trips) {
    Steps S = {out, cap, 0};
    *trips = 0;
    const bool ok = runs ? walk_runs(m, n, nw, ft, fb, S, trips) : walk_columns(m, n, nw, ft, fb, S);
    return ok ? S.n : -(S.n + 1);
}
"""
MAIN = r"""
// records: int32 m, n, nw; fullt (n + 1 words); the columns ((n + 1) * 2 nw words)
int main(int argc, char **argv) {
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    long cases = 0;
    for (;;) {
        int32_t h[3];
        if (fread(h, 4, 3, f) != 3) break;
        const int m = h[0], n = h[1], nw = h[2];
        const size_t nt = (size_t)n + 1, nb = nt * 2 * nw, cap = (size_t)m + n + 1;
        int32_t *ft = (int32_t *)malloc(nt * 4);
        uint32_t *fb = (uint32_t *)malloc(nb * 4);
        int32_t *a = (int32_t *)malloc(cap * 12), *b = (int32_t *)malloc(cap * 12);
        if (fread(ft, 4, nt, f) != nt || fread(fb, 4, nb, f) != nb) return 3;
        long trips;
        const long ra = host_walk(0, m, n, nw, ft, fb, a, (long)cap, &trips), rb = host_walk(1, m, n, nw, ft, fb, b, (long)cap, &trips);
        const long k = ra < 0 ? -ra - 1 : ra;
        if (ra != rb || (size_t)k > cap || memcmp(a, b, (size_t)k * 12)) { fprintf(stderr, "record %ld differs\n", cases); return 1; }
        free(ft); free(fb); free(a); free(b);
        cases++;
    }
    fclose(f);
    printf("%ld cases\n", cases);
    return 0;
}
"""


def _body():
    return _block(os.path.join(ROOT, "hite_amd", "csrc", "hite_align.hip"), "wide_walk_probe")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    lib = _build(tmp_path_factory.mktemp("wide_walk"), "wide_walk", _body(), DRIVER)
    lib.host_walk.restype = C.c_long
    lib.host_walk.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_void_p]
    return lib


class Matrix:
    """fullt and the columns of a pair of m rows and n columns, nw words a column"""

    def __init__(self, m, n, nw, ft, dg, up):
        self.m, self.n, self.nw = m, n, nw
        self.ft = np.ascontiguousarray(ft, np.int32)
        assert self.ft.shape == (n + 1,) and dg.shape == up.shape == (n + 1, 32 * nw)
        self.fb = np.ascontiguousarray(np.concatenate([self.pack(dg), self.pack(up)], axis=1))
        assert self.fb.shape == (n + 1, 2 * nw)

    @staticmethod
    def pack(bits):
        b = bits.reshape(bits.shape[0], -1, 32).astype(np.uint32)
        return (b << np.arange(32, dtype=np.uint32)).sum(axis=2, dtype=np.uint64).astype(np.uint32)

    def record(self):
        return struct.pack("<3i", self.m, self.n, self.nw) + self.ft.tobytes() + self.fb.tobytes()


def walk(lib, M, runs):
    cap = M.m + M.n + 1
    out = np.zeros((cap, 3), np.int32)
    trips = C.c_long(0)
    r = lib.host_walk(runs, M.m, M.n, M.nw, M.ft.ctypes.data_as(C.c_void_p), M.fb.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), cap,
                      C.byref(trips))
    k = -r - 1 if r < 0 else r
    assert k <= cap
    return r >= 0, out[:k], trips.value


def same(lib, M):
    """both walks take the same steps to the same end -> (completed, steps, trips of the walk by runs)"""
    ok0, s0, _ = walk(lib, M, 0)
    ok1, s1, trips = walk(lib, M, 1)
    if ok0 != ok1 or not np.array_equal(s0, s1):
        k = next((x for x in range(min(len(s0), len(s1))) if not np.array_equal(s0[x], s1[x])), min(len(s0), len(s1)))
        raise AssertionError("m %d n %d nw %d: completed %s / %s, %d / %d steps, first difference at step %d: %s / %s" %
                             (M.m, M.n, M.nw, ok0, ok1, len(s0), len(s1), k, s0[k:k + 2].tolist(), s1[k:k + 2].tolist()))
    return ok0, s0, trips


def random_matrix(rng, nw, n, p_dg, p_up, shift):
    """the band starts half its height above row 1 and moves by 0 / 4 / 8 rows every fourth column (shift: their weights); the walk
    starts where the last column's band has its middle"""
    W = 32 * nw
    moves = rng.choice([0, 4, 8], size=(n + 4) // 4, p=shift)
    ft = np.zeros(n + 1, np.int64)
    ft[1:] = -(W // 2) + np.cumsum(moves)[(np.arange(1, n + 1) - 1) // 4]
    ft[0] = 1 << 20                                            # never read: a walk that did would leave the band
    m = int(ft[n] + W // 2 + rng.integers(-W // 4, W // 4))
    m = max(m, 1)
    dg = rng.random((n + 1, W)) < p_dg
    up = rng.random((n + 1, W)) < p_up
    return Matrix(m, n, nw, ft, dg, up)


def test_random_matrices(lib, tmp_path):
    rng = np.random.default_rng(20)
    records, done, failed, steps, trips, ops = [], 0, 0, 0, 0, np.zeros(3, np.int64)
    for nw, sizes in ((2, (1, 5, 63, 64, 65, 200)), (4, (17, 130, 400)), (64, (300, 1500))):
        for n in sizes:
            for p_dg in (0.99, 0.9, 0.5, 0.1):
                for p_up in (0.05, 0.5, 0.95):
                    for shift in ((0.1, 0.8, 0.1), (0.45, 0.1, 0.45)):
                        for rep in range(3 if nw < 64 else 1):
                            M = random_matrix(rng, nw, n, p_dg, p_up, shift)
                            ok, s, t = same(lib, M)
                            done += ok
                            failed += not ok
                            steps += len(s)
                            trips += t
                            ops += np.bincount(s[:, 2], minlength=3)
                            if rep == 0 and (nw < 64 or p_up == 0.5):
                                records.append(M.record())
    assert done > 100 and failed > 100 and (ops > 1000).all(), (done, failed, ops)
    assert trips < steps
    # the same comparison under the sanitizers, every array in a heap buffer of exactly its size
    cpp, exe, data = tmp_path / "walk_main.cpp", tmp_path / "walk_main", tmp_path / "cases.bin"
    cpp.write_text(PRELUDE + _body() + DRIVER + MAIN)
    data.write_bytes(b"".join(records))
    subprocess.run(["g++", "-O1", "-g", "-static-libasan", "-static-libubsan", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", str(exe), str(cpp)], check=True)
    res = subprocess.run([str(exe), str(data)], capture_output=True, text=True)
    assert res.returncode == 0 and not res.stderr.strip(), (res.returncode, res.stderr[-3000:])
    assert res.stdout.strip() == "%d cases" % len(records)


def path_matrix(m, n, nw, path, t0=None):
    """a matrix whose bits spell ONE path: path = ops from the last cell towards the first (D / U / L); every cell off the path has
    its diagonal bit clear and its up bit set (a walk that strays runs up to the band's first row); the band starts at row t0 + 1"""
    W = 32 * nw
    ft = np.full(n + 1, 0 if t0 is None else t0, np.int64)
    dg = np.zeros((n + 1, W), bool)
    up = np.ones((n + 1, W), bool)
    if ft[0] < 0:
        up[:, -ft[0] - 1] = False         # row 0, where the band holds it, stops every up run (as the forward pass leaves it)
    i, j = m, n
    for op in path:
        assert i > 0 and j > 0
        kb = i - ft[j] - 1
        assert 0 <= kb < W
        if op == D:
            dg[j, kb] = True
            i, j = i - 1, j - 1
        elif op == U:                 # (up allowed, diagonal clear: the run goes on to the cell where the next op sets its stop bit)
            i -= 1
        else:
            up[j, kb] = False
            j -= 1
    return Matrix(m, n, nw, ft, dg, up), (i, j)


def expect(lib, M, path):
    ok, s, trips = same(lib, M)
    assert ok and s[:, 2].tolist() == list(path), (s[:, 2].tolist()[:40], list(path)[:40])
    return trips


def test_hand_made_paths(lib):
    # an up run directly behind a left run, and the reverse; each between diagonal runs
    for first, second in ((L, U), (U, L)):
        for a in (1, 5, 64, 70):
            for b in (1, 3, 64):
                path = [D] * 10 + [first] * a + [second] * b + [D] * 20
                m = 30 + (a if first == U else b)
                n = 30 + (a if first == L else b)
                M, end = path_matrix(m, n, 16, path)
                assert end == (0, 0)
                expect(lib, M, path)
    # diagonal and left runs of exactly 1, 63, 64, 65, 127, 128, 129 steps between two gaps, and the trips they take
    for k in (1, 63, 64, 65, 127, 128, 129, 200):
        for gap in (U, L):
            path = [D] * 3 + [gap] * 2 + [D] * k + [gap] * 2 + [D] * 3
            ups, lefts = path.count(U), path.count(L)
            M, end = path_matrix(6 + k + ups, 6 + k + lefts, 16, path)
            assert end == (0, 0)
            trips = expect(lib, M, path)
            assert trips <= 4 + (k + 63) // 64              # (the general step of an up run takes the step behind it along)
        path = [D] * 3 + [U] * 2 + [D] + [L] * k + [D] + [U] * 2 + [D] * 3
        M, end = path_matrix(8 + 4, 8 + k, 16, path)
        assert end == (0, 0)
        assert expect(lib, M, path) <= 6 + (k + 63) // 64
    # i reaches 0 inside a trip with columns to go; j reaches 0 with rows to go
    for k in (1, 30, 64, 100):
        path = [D] * k
        M, end = path_matrix(k, k + 37, 16, path)
        assert end == (0, 37)
        expect(lib, M, path)
        M, end = path_matrix(k + 37, k, 16, path)
        assert end == (37, 0)
        expect(lib, M, path)
    # a left run into column 0, an up run into row 0
    path = [D] * 5 + [L] * 70
    M, end = path_matrix(6, 75, 16, path)
    assert end == (1, 0)
    expect(lib, M, path)
    path = [D] * 5 + [U] * 70
    M, end = path_matrix(75, 6, 16, path, t0=-100)
    assert end == (0, 1)
    expect(lib, M, path)


def test_walks_that_fail(lib):
    # the diagonal run leaves the band in mid-trip: rows above the band's first
    M2 = Matrix(100, 100, 2, np.full(101, 68), np.ones((101, 64), bool), np.ones((101, 64), bool))      # band rows 69 .. 132
    ok, s, _ = same(lib, M2)
    assert not ok and s[:, 2].tolist() == [D] * 32 and s[-1].tolist()[:2] == [69, 69]
    # no stop bit below: diagonal clear and up allowed all the way to the band's first row
    dg = np.ones((101, 64), bool)
    dg[80, :] = False
    ok, s, _ = same(lib, Matrix(100, 100, 2, np.full(101, 60), dg, np.ones((101, 64), bool)))
    assert not ok and len(s) == 20
    # the band of a column on the way lies below the path
    ft = np.full(101, 40)
    ft[50] = 200
    ok, s, _ = same(lib, Matrix(100, 100, 2, ft, np.ones((101, 64), bool), np.ones((101, 64), bool)))
    assert not ok and len(s) == 50
