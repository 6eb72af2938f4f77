"""What the host-compiled tests of the banded HSP aligner share (tests/test_host_compiled_pairhsp.py, _ltrscan.py, _annotate.py): the
prelude that lets a `// >>> name` .. `// <<< name` block of hite_amd/csrc compile for the host, the lane-by-lane host copy of the strip
loop of hsp_align (hite_amd/csrc/hite_hsp.h) and the build of a test's source into a library."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PRELUDE = r"""
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#define __device__
#define __host__
#define __forceinline__ inline
#include "hite_gpu.h"
"""

# the strip loop of hsp_align, lane by lane: strips of 64 lanes, lane l on row first + d - 1 - l at step d, the value handed to the next
# lane, only the rows where the band meets the strip, the last column of a strip kept by its diagonal in one of two buffers for the next
HOST_ALIGN = r"""
static HspBest host_align(const uint8_t *q, int m, const uint8_t *s, int dlo, int dhi, int r0, int r1, int c0, int c1) {
    static int64_t bnd_a[2 * HSP_BAND];
    static uint32_t bnd_b[2 * HSP_BAND];
    HspBest best = {0, 0, 0};
    const int cs = std::max(c0, r0 + dlo), ce = std::min(c1, r1 + dhi);
    int buf = 0;
    for (int js = cs; js <= ce; js += 64, buf ^= 1) {
        const int nl = std::min(64, ce - js + 1);
        const bool more = js + 64 <= ce;
        const int first = std::max(r0, js - dhi), last = std::min(r1, js + nl - 1 - dlo);
        const int ib = first - 1;
        const int64_t *rd_a = bnd_a + (buf ^ 1) * HSP_BAND;
        const uint32_t *rd_b = bnd_b + (buf ^ 1) * HSP_BAND;
        auto edge = [&](int row) {
            HspVal v = {0, 0};
            const int dd = js - 1 - row;
            if (js > cs && row >= r0 && row <= r1 && dd >= dlo && dd <= dhi) { v.a = rd_a[dhi - dd]; v.b = rd_b[dhi - dd]; }
            return v;
        };
        HspVal cur[64], diag[64], left[64];
        int ca[64], cb[64];
        for (int lane = 0; lane < 64; lane++) {
            cur[lane] = diag[lane] = HspVal{0, 0};
            ca[lane] = 4;
            cb[lane] = lane < nl ? hsp_code(s[js + lane - 1]) : 4;
        }
        diag[0] = edge(ib);
        const int steps = last - ib + nl - 1;
        for (int d = 1; d <= steps; d++) {
            for (int lane = 63; lane >= 1; lane--) { left[lane] = cur[lane - 1]; ca[lane] = ca[lane - 1]; }
            left[0] = edge(ib + d);
            ca[0] = ib + d <= m ? hsp_code(q[ib + d - 1]) : 4;
            for (int lane = 0; lane < 64; lane++) {
                const int i = ib + d - lane, j = js + lane;
                const bool on = lane < nl && i >= r0 && i <= r1 && j - i >= dlo && j - i <= dhi;
                HspVal v = hsp_cell(diag[lane], cur[lane], left[lane], ca[lane], cb[lane], i, j);
                diag[lane] = left[lane];
                if (!on) v = HspVal{0, 0};
                cur[lane] = v;
                if (on) {
                    const uint32_t e = (uint32_t)i << 16 | (uint32_t)j;
                    if (v.a > 0 && hsp_best_better(v.a, v.b, e, best)) { best.a = v.a; best.b = v.b; best.e = e; }
                    if (more && lane == 63) { bnd_a[buf * HSP_BAND + dhi - (j - i)] = v.a; bnd_b[buf * HSP_BAND + dhi - (j - i)] = v.b; }
                }
            }
        }
    }
    return best;
}
"""


def blocks(path, *names):
    """the text between `// >>> name` and `// <<< name` of a file of hite_amd/csrc, for every name, in that order"""
    src = open(os.path.join(ROOT, "hite_amd", "csrc", path)).read()
    out = []
    for name in names:
        m = re.search(r"// >>> %s.*?\n(.*?)// <<< %s" % (name, name), src, re.S)
        assert m, (path, name)
        out.append(m.group(1))
    return "".join(out)


def compile_host(d, stem, source):
    """PRELUDE + source, compiled in directory d ($HITE_HOST_CXXFLAGS adds flags), loaded"""
    cpp, so = d / (stem + ".cpp"), d / (stem + ".so")
    cpp.write_text(PRELUDE + source)
    extra = os.environ.get("HITE_HOST_CXXFLAGS", "").split()
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include")] + extra + ["-o", str(so), str(cpp)], check=True)
    return C.CDLL(str(so))
