"""CPU-only: the cell update and the pair test of fc_unit_kernel (hite_amd/csrc/hite_framecluster.hip, the block between
`// >>> framecluster_cell` and `// <<< framecluster_cell`) compiled for the HOST as tests/test_host_compiled_identity.py does for
the identity kernel, inside a host copy of the kernel's pair loop (strips of 64 lanes, lane l on row d - l at step d, the value
handed to the next lane, the last column of a strip kept for the next one), and compared with the twin on the cases the GPU tests
run.  What only the device has -- LDS, the shuffles, the units, the leader pass, the batches -- is left to
tests/test_gpu_framecluster.py."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import framecluster_cases as FC  # noqa: E402
import framecluster_twin as T  # noqa: E402

PRELUDE = r"""
#include <stdint.h>
#include <algorithm>
#define __device__
#define __forceinline__ inline
"""

WRAPPER = r"""
static int64_t host_pair_one(const uint8_t *a, int m, const uint8_t *b, int n, bool rev) {
    int64_t bnd[257] = {0}, best = 0;
    uint8_t ac[256], bc[256];
    for (int i = 0; i < m; i++) ac[i] = (uint8_t)fc_code(a[i], false);
    for (int j = 0; j < n; j++) bc[j] = (uint8_t)fc_code(b[j], false);
    for (int s0 = 0; s0 < n; s0 += 64) {
        const int nl = std::min(64, n - s0);
        const bool more = s0 + 64 < n;
        int cb[64], ca[64];
        int64_t cur[64], diag[64], left[64];
        for (int lane = 0; lane < 64; lane++) {
            cb[lane] = lane < nl ? (rev ? fc_comp(bc[n - 1 - (s0 + lane)]) : bc[s0 + lane]) : 4;
            cur[lane] = diag[lane] = 0;
            ca[lane] = 4;
        }
        for (int d = 1; d <= m + nl - 1; d++) {
            for (int lane = 63; lane >= 1; lane--) { left[lane] = cur[lane - 1]; ca[lane] = ca[lane - 1]; }
            left[0] = (s0 > 0 && d <= m) ? bnd[d] : 0;
            ca[0] = d <= m ? ac[d - 1] : 4;
            for (int lane = 0; lane < 64; lane++) {
                const int i = d - lane;
                const bool on = lane < nl && i >= 1 && i <= m;
                const int64_t v = fc_cell(diag[lane], cur[lane], left[lane], ca[lane], cb[lane]);
                diag[lane] = left[lane];
                if (on) {
                    cur[lane] = v;
                    if (v > best) best = v;
                    if (more && lane == 63) bnd[i] = v;
                }
            }
        }
    }
    return best;
}
extern "C" int64_t host_pair(const uint8_t *a, int m, const uint8_t *b, int n, int both) {
    int64_t r = 0;
    if (m > 0 && n > 0) {
        r = host_pair_one(a, m, b, n, false);
        if (both) r = std::max(r, host_pair_one(a, m, b, n, true));
    }
    return r;
}
extern "C" int host_similar(int64_t r, int la, int lb, double ident, double cov_short, double cov_long, int min_cov) {
    return fc_similar(r, la, lb, ident, cov_short, cov_long, min_cov) ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    src = open(os.path.join(ROOT, "hite_amd", "csrc", "hite_framecluster.hip")).read()
    m = re.search(r"// >>> framecluster_cell.*?\n(.*?)// <<< framecluster_cell", src, re.S)
    assert m
    d = tmp_path_factory.mktemp("framecluster_cell")
    cpp, so = d / "fc.cpp", d / "fc.so"
    cpp.write_text(PRELUDE + m.group(1) + WRAPPER)
    extra = os.environ.get("HITE_HOST_CXXFLAGS", "").split()
    subprocess.run(["g++", "-O2", "-shared", "-fPIC"] + extra + ["-o", str(so), str(cpp)], check=True)
    lib = C.CDLL(str(so))
    lib.host_pair.restype = C.c_int64
    lib.host_pair.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.c_int]
    lib.host_similar.argtypes = [C.c_int64, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int]
    return lib


def _value(lib):
    def value(a, b, both):
        a, b = T.as_bytes(a), T.as_bytes(b)
        return T.unpack(lib.host_pair(a, len(a), b, len(b), int(bool(both))))
    return value


def test_pairs_with_a_known_value(lib):
    value = _value(lib)
    for label, a, b, both, exp in FC.pair_values():
        assert value(a, b, both) == T.pair_value_c(a, b, both), label
        if exp is not None:
            assert value(a, b, both) == exp, label


def test_pair_loop_vs_twin_at_the_strip_edges(lib):
    """random and related pairs at lengths around the 64 columns of a strip and at the length limit, both strands"""
    value = _value(lib)
    rng = np.random.default_rng(21)
    n = 0
    for la in (1, 11, 63, 64, 65, 127, 128, 129, 200, 255, 256):
        for lb in (1, 12, 63, 64, 65, 128, 129, 192, 193, 256):
            a = FC.dna(rng, la)
            for b in (FC.dna(rng, lb), (FC.mutate(rng, a, 0.08) + FC.dna(rng, lb))[:lb], FC.revcomp(FC.mutate(rng, a + FC.dna(rng, lb), 0.1))[:lb]):
                assert value(a, b, True) == T.pair_value_c(a, b, True), (la, lb, a, b)
                n += 1
    assert n == 330


def test_clusters_through_the_host_compiled_cell(lib):
    """the ordered pass of the twin over the host-compiled pair value and pair test == the twin, on every small case"""
    value = _value(lib)
    for label, groups, kw in FC.small_cases():
        def sim(r, la, lb, ident, cov_short, cov_long, min_cov):
            packed = (r[0] << 37) + (r[1] << 28) + (r[2] << 18) + (r[3] << 9) + r[4]
            return bool(lib.host_similar(packed, la, lb, ident, cov_short, cov_long, min_cov))
        old = T.similar
        T.similar = sim
        try:
            got = [T.cluster_group(g, value=value, **kw) for g in groups]
        finally:
            T.similar = old
        assert got == T.frame_cluster(groups, **kw), label
        if label in FC.EXPECT:
            assert got == FC.EXPECT[label], label
