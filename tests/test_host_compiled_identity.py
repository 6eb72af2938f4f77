"""CPU-only: the cell update of ident_pair_kernel (hite_amd/csrc/hite_ident.hip, the block between `// >>> ident_cell` and
`// <<< ident_cell`) compiled for the HOST as tests/test_host_compiled.py does for other kernels, inside a host copy of the kernel's
row loop (strips of 64 lanes run one after the other, the six shift-and-add steps of the in-row chain, the carry between strips),
and compared with the twin on the cases the GPU tests run.  What only the device has -- LDS, the shuffles, the launch geometry, the
batches -- is left to tests/test_gpu_identity.py."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import identity_cases as IC  # noqa: E402
import identity_twin as T  # noqa: E402

PRELUDE = r"""
#include <stdint.h>
#include <vector>
#include <algorithm>
#define __device__
#define __forceinline__ inline
"""

WRAPPER = r"""
extern "C" void host_ident_pair(const uint8_t *a, int m, const uint8_t *b, int n, int strand, int band, int32_t *out) {
    const int lo = std::min(0, n - m) - band, hi = std::max(0, n - m) + band, W = hi - lo + 1, ns = (W + 63) >> 6;
    const bool rev = strand != 0;
    std::vector<uint32_t> row((size_t)ns * 64 + 64);
    for (int x = 0; x < ns * 64 + 64; x++) {
        const int j = lo + x;
        row[x] = (x < W && j >= 0 && j <= n) ? IDENT_ZERO + (uint32_t)j * IDENT_ONE : IDENT_INF;
    }
    for (int i = 1; i <= m; i++) {
        const int ca = ident_code(a[i - 1], false);
        uint32_t carry = IDENT_INF;
        for (int s = 0; s < ns; s++) {
            uint32_t t[64], y[64];
            bool exists[64];
            for (int lane = 0; lane < 64; lane++) {
                const int x = s * 64 + lane, j = i + lo + x;
                exists[lane] = x < W && j >= 0 && j <= n;
                t[lane] = IDENT_INF;
                if (exists[lane]) {
                    const int cb = j >= 1 ? ident_code(rev ? b[n - j] : b[j - 1], rev) : 4;
                    t[lane] = ident_cell(j >= 1 ? row[x] : IDENT_INF, row[x + 1], ca, cb);
                }
            }
            t[0] = ident_chain(t[0], carry, 1);
            for (int d = 1; d < 64; d <<= 1) {
                for (int lane = 0; lane < 64; lane++) y[lane] = lane >= d ? t[lane - d] : 0;
                for (int lane = d; lane < 64; lane++) t[lane] = ident_chain(t[lane], y[lane], d);
            }
            for (int lane = 0; lane < 64; lane++) {
                if (!exists[lane]) t[lane] = IDENT_INF;
                row[s * 64 + lane] = t[lane];
            }
            carry = t[63];
        }
    }
    const uint32_t v = row[n - m - lo];
    out[0] = (int32_t)(v >> 16);
    out[1] = (int32_t)(0xFFFFu - (v & 0xFFFFu));
}
"""


def _lib(tmp_path):
    src = open(os.path.join(ROOT, "hite_amd", "csrc", "hite_ident.hip")).read()
    m = re.search(r"// >>> ident_cell.*?\n(.*?)// <<< ident_cell", src, re.S)
    assert m
    cpp, so = tmp_path / "ident.cpp", tmp_path / "ident.so"
    cpp.write_text(PRELUDE + m.group(1) + WRAPPER)
    extra = os.environ.get("HITE_HOST_CXXFLAGS", "").split()
    subprocess.run(["g++", "-O2", "-shared", "-fPIC"] + extra + ["-o", str(so), str(cpp)], check=True)
    return C.CDLL(str(so))


def _run(lib, seqs, pairs, band):
    got = np.zeros((len(pairs), 2), dtype=np.int32)
    u8p = C.POINTER(C.c_uint8)
    for k, (ai, a0, a1, bi, b0, b1, st) in enumerate(pairs):
        a = np.frombuffer(bytes(seqs[ai][a0:a1]) + b"\0", dtype=np.uint8)
        b = np.frombuffer(bytes(seqs[bi][b0:b1]) + b"\0", dtype=np.uint8)
        out = np.zeros(2, dtype=np.int32)
        lib.host_ident_pair(a.ctypes.data_as(u8p), a1 - a0, b.ctypes.data_as(u8p), b1 - b0, int(st), int(band), out.ctypes.data_as(C.c_void_p))
        got[k] = out
    return got


def test_ident_cell_update_vs_twin(tmp_path):
    lib = _lib(tmp_path)
    n = 0
    for label, seqs, pairs, band in IC.small_cases() + IC.batch(n_pair=400, max_len=300, seed=9):
        exp = T.pair_identity(seqs, pairs, band)
        ok = [k for k in range(len(pairs)) if exp[k, 0] >= 0]        # (refusing a pair is the entry point's part)
        assert ok, label
        got = _run(lib, seqs, [pairs[k] for k in ok], band)
        bad = [(ok[q], got[q].tolist(), exp[ok[q]].tolist()) for q in range(len(ok)) if (got[q] != exp[ok[q]]).any()]
        assert not bad, (label, bad[:5])
        n += len(ok)
    assert n > 900


def test_ident_saturating_states(tmp_path):
    """costs near the top of the 16-bit half: two sequences of 32 767 bases without a base in common, on one diagonal"""
    lib = _lib(tmp_path)
    a, b = b"A" * IC.MAX_LEN, b"C" * IC.MAX_LEN
    seqs = [a, b, a[:IC.MAX_LEN - 40]]
    pairs = [IC.whole(seqs, 0, 1), IC.whole(seqs, 2, 1), IC.whole(seqs, 0, 0)]
    exp = T.pair_identity(seqs, pairs, 1)
    assert exp.tolist() == [[IC.MAX_LEN, 0], [IC.MAX_LEN, 0], [0, IC.MAX_LEN]]
    assert (_run(lib, seqs, pairs, 1) == exp).all()
