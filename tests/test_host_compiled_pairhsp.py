"""CPU-only: the cell update and the compares of ph_pair_kernel (hite_amd/csrc/hite_pairhsp.hip, the block between
`// >>> pairhsp_cell` and `// <<< pairhsp_cell`) compiled for the HOST as tests/test_host_compiled_framecluster.py does for the
clustering of frames, inside a host copy of the kernel's strip loop (strips of 64 lanes, lane l on row first + d - 1 - l at step d,
the value handed to the next lane, only the rows where the band meets the strip, the last column of a strip kept by its diagonal in
one of two buffers for the next one), and compared with the twin at the strip-edge lengths the GPU tests run.  What only the device
has -- the word table, the votes, the windows, the data-parallel moves, the batches -- is left to tests/test_gpu_pairhsp.py."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pairhsp_cases as PC  # noqa: E402
import pairhsp_twin as T  # noqa: E402

PRELUDE = r"""
#include <stdint.h>
#include <algorithm>
#define __device__
#define __forceinline__ inline
#include "hite_gpu.h"
#define PH_BAND (HITE_PAIRHSP_BAND_BELOW + HITE_PAIRHSP_BAND_ABOVE)
"""

WRAPPER = r"""
extern "C" int host_align(const uint8_t *q, int m, const uint8_t *s, int n, int dlo, int dhi, int r0, int r1, int c0, int c1, int32_t *out) {
    static int64_t bnd_a[2 * PH_BAND];
    static uint32_t bnd_b[2 * PH_BAND];
    PhBest best = {0, 0, 0};
    const int cs = std::max(c0, r0 + dlo), ce = std::min(c1, r1 + dhi);
    int buf = 0;
    for (int js = cs; js <= ce; js += 64, buf ^= 1) {
        const int nl = std::min(64, ce - js + 1);
        const bool more = js + 64 <= ce;
        const int first = std::max(r0, js - dhi), last = std::min(r1, js + nl - 1 - dlo);
        const int ib = first - 1;
        const int64_t *rd_a = bnd_a + (buf ^ 1) * PH_BAND;
        const uint32_t *rd_b = bnd_b + (buf ^ 1) * PH_BAND;
        auto edge = [&](int row) {
            PhVal v = {0, 0};
            const int dd = js - 1 - row;
            if (js > cs && row >= r0 && row <= r1 && dd >= dlo && dd <= dhi) { v.a = rd_a[dhi - dd]; v.b = rd_b[dhi - dd]; }
            return v;
        };
        PhVal cur[64], diag[64], left[64];
        int ca[64], cb[64];
        for (int lane = 0; lane < 64; lane++) {
            cur[lane] = diag[lane] = PhVal{0, 0};
            ca[lane] = 4;
            cb[lane] = lane < nl ? ph_code(s[js + lane - 1]) : 4;
        }
        diag[0] = edge(ib);
        const int steps = last - ib + nl - 1;
        for (int d = 1; d <= steps; d++) {
            for (int lane = 63; lane >= 1; lane--) { left[lane] = cur[lane - 1]; ca[lane] = ca[lane - 1]; }
            left[0] = edge(ib + d);
            ca[0] = ib + d <= m ? ph_code(q[ib + d - 1]) : 4;
            for (int lane = 0; lane < 64; lane++) {
                const int i = ib + d - lane, j = js + lane;
                const bool on = lane < nl && i >= r0 && i <= r1 && j - i >= dlo && j - i <= dhi;
                PhVal v = ph_cell(diag[lane], cur[lane], left[lane], ca[lane], cb[lane], i, j);
                diag[lane] = left[lane];
                if (!on) v = PhVal{0, 0};
                cur[lane] = v;
                if (on) {
                    const uint32_t e = (uint32_t)i << 16 | (uint32_t)j;
                    if (v.a > 0 && ph_best_better(v.a, v.b, e, best)) { best.a = v.a; best.b = v.b; best.e = e; }
                    if (more && lane == 63) { bnd_a[buf * PH_BAND + dhi - (j - i)] = v.a; bnd_b[buf * PH_BAND + dhi - (j - i)] = v.b; }
                }
            }
        }
    }
    if (best.a == 0) return 0;
    out[0] = (int32_t)(best.b >> 16); out[1] = (int32_t)(best.e >> 16); out[2] = (int32_t)(best.b & 0xFFFFu); out[3] = (int32_t)(best.e & 0xFFFFu);
    out[4] = (int32_t)(best.a >> 40); out[5] = (int32_t)((best.a >> 20) & 0xFFFFF); out[6] = (int32_t)(best.a & 0xFFFFF);
    return 1;
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    src = open(os.path.join(ROOT, "hite_amd", "csrc", "hite_pairhsp.hip")).read()
    m = re.search(r"// >>> pairhsp_cell.*?\n(.*?)// <<< pairhsp_cell", src, re.S)
    assert m
    d = tmp_path_factory.mktemp("pairhsp_cell")
    cpp, so = d / "ph.cpp", d / "ph.so"
    cpp.write_text(PRELUDE + m.group(1) + WRAPPER)
    extra = os.environ.get("HITE_HOST_CXXFLAGS", "").split()
    subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include")] + extra + ["-o", str(so), str(cpp)], check=True)
    return C.CDLL(str(so))


def _align(lib):
    def align(q, s, dlo, dhi, r0, r1, c0, c1):
        q, s = T.as_bytes(q), T.as_bytes(s)
        out = np.zeros(7, dtype=np.int32)
        ok = lib.host_align(q, len(q), s, len(s), dlo, dhi, r0, r1, c0, c1, out.ctypes.data_as(C.c_void_p))
        return tuple(int(x) for x in out) if ok else None
    return align


def _bands(q, s, dm):
    """the bands the definition gives the pair, and one at each end of the diagonals"""
    qc, sc = T.codes(q), T.codes(s)
    lo = T.NO_DIAG_MIN if dm is None else dm
    bands = [T.band_of(b, len(qc), lo) for b in T.windows(T.votes(qc, sc, lo))]
    return bands + [(-(len(qc) - 1) - 5, -(len(qc) - 1) + 186), (len(sc) - 1 - 186, len(sc) + 5), (-3, 0)]


def test_strip_loop_vs_twin_at_the_strip_edges(lib):
    """random and related pairs at lengths around the 64 columns of a strip, in their own bands and in bands at the corners"""
    align = _align(lib)
    grid = [c for c in PC.length_grid() if "unrelated" not in c[0]]
    n = 0
    for label, q, s, dm in grid:
        for dlo, dhi in _bands(q, s, dm):
            assert align(q, s, dlo, dhi, 1, len(q), 1, len(s)) == T.align_c(q, s, dlo, dhi, 1, len(q), 1, len(s)), (label, dlo, dhi)
            n += 1
    assert n >= 3 * len(grid)


def test_rectangles_and_band_edges(lib):
    """sub-rectangles, alignments that run along and across the band's edges, diag_min through a band"""
    align = _align(lib)
    rng = np.random.default_rng(4)
    n_hsp = 0
    for label, q, s, dm in PC.rectangles() + PC.band_edges()[::3] + PC.diag_min_cases()[:6] + PC.ties() + PC.bytes_cases():
        m, n = len(q), len(s)
        for dlo, dhi in _bands(q, s, dm)[:-2]:
            rects = [(1, m, 1, n)]
            for _ in range(3):
                r0, c0 = int(rng.integers(1, m + 1)), int(rng.integers(1, n + 1))
                rects.append((r0, int(rng.integers(r0, m + 1)), c0, int(rng.integers(c0, n + 1))))
            for r in rects:
                got = align(q, s, dlo, dhi, *r)
                assert got == T.align_c(q, s, dlo, dhi, *r), (label, dlo, dhi, r)
                n_hsp += got is not None
    assert n_hsp > 100
