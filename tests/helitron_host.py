"""The scoring code of hite_amd/csrc/hite_helitron.hip (the block between `// >>> helitron_score` and `// <<< helitron_score`:
base codes, the plane shift, the pattern test, the anchor literals on the forward text, the windows of the four anchor kinds, the
compiled pattern) built for the HOST, as tests/test_host_compiled_identity.py does for the identity kernel, inside a host loop
that walks the bytes, fills the window planes bit by bit and pairs per sequence and strand.  What only the device has -- the
ballots, LDS, the scans and the placement of the records -- is left to tests/test_gpu_helitron.py.  tests/test_helitron_cases.py
holds this form against the twin; the GPU volume case and tools/helitron_bench.py use it where the Python twin would take minutes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PRELUDE = r"""
#include <stdint.h>
#include <vector>
#include <algorithm>
#include <thread>
#include <stdlib.h>
#include "hite_gpu.h"
#define __device__
#define __forceinline__ inline
"""

WRAPPER = r"""
struct Planes { uint64_t lo[2], hi[2], nn[2]; int avail; };
static void planes_of(const uint8_t *s, int kind, int64_t i, int64_t b, int64_t e, Planes *W) {
    int64_t w0, av; int dir;
    heli_window(kind, i, b, e, &w0, &dir, &av);
    W->avail = av > 95 ? 95 : (int)av;
    W->lo[0] = W->lo[1] = W->hi[0] = W->hi[1] = W->nn[0] = W->nn[1] = 0;
    for (int k = 0; k < W->avail; k++) {
        const int c = heli_code(s[w0 + (int64_t)dir * k], kind == 1 || kind == 3);
        W->lo[k >> 6] |= (uint64_t)(c & 1) << (k & 63);
        W->hi[k >> 6] |= (uint64_t)((c >> 1) & 1) << (k & 63);
        W->nn[k >> 6] |= (uint64_t)((c >> 2) & 1) << (k & 63);
    }
}
// dense: four rows of nb entries (plus heads, plus tails, minus heads, minus tails, the minus rows in the coordinates of the reverse
// complement).  -> the number of anchors, -1 for a pattern beyond a limit
extern "C" int64_t host_helitron_scores(int64_t n, const uint8_t *s, const int64_t *off, int32_t n_head, const hite_lcv *head,
                                        int32_t n_tail, const hite_lcv *tail, int32_t *dense) {
    std::vector<HeliPat> hp(n_head), tp(n_tail);
    for (int k = 0; k < n_head; k++) if (!heli_compile(head[k], false, &hp[k])) return -1;
    for (int k = 0; k < n_tail; k++) if (!heli_compile(tail[k], true, &tp[k])) return -1;
    const int64_t nb = off[n];
    std::fill(dense, dense + 4 * nb, 0);
    // the sequences in strides over a few threads (every sequence writes its own columns)
    const char *env = getenv("HITE_HOST_THREADS");
    int nt = env ? atoi(env) : (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    if (nt < 1) nt = 1;
    std::vector<int64_t> count(nt, 0);
    auto work = [&](int t) {
        for (int64_t q = t; q < n; q += nt) {
            const int64_t b = off[q], e = off[q + 1], L = e - b;
            for (int64_t i = b; i < e; i++) {
                const int kinds = heli_anchor_kinds(s, i, b, e);
                for (int kind = 0; kind < 4; kind++) {
                    if (!(kinds >> kind & 1)) continue;
                    count[t]++;
                    Planes W;
                    planes_of(s, kind, i, b, e, &W);
                    const std::vector<HeliPat> &tab = kind < 2 ? hp : tp;
                    int sc = 0;
                    for (const HeliPat &P : tab) sc += heli_match(W.lo[0], W.lo[1], W.hi[0], W.hi[1], W.nn[0], W.nn[1], W.avail, P) ? 1 : 0;
                    const int64_t x = i - b;
                    const int64_t at = kind == 0 ? i : kind == 2 ? nb + i : kind == 1 ? 2 * nb + b + (L - 2 - x) : 3 * nb + b + (L - 1 - x);
                    dense[at] = sc;
                }
            }
        }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < nt; t++) pool.emplace_back(work, t);
    work(0);
    for (std::thread &th : pool) th.join();
    int64_t anchors = 0;
    for (int64_t c : count) anchors += c;
    return anchors;
}
// the whole stage: out = rows of 6 (seq, start, end, strand, head score, tail score), the first cap of them; stats[4]; -> records
extern "C" int64_t host_helitron_scan(int64_t n, const uint8_t *s, const int64_t *off, int32_t n_head, const hite_lcv *head, int32_t n_tail,
                                      const hite_lcv *tail, int32_t hthr, int32_t tthr, int32_t len_min, int32_t len_max, int64_t cap,
                                      int32_t *out, int64_t *stats) {
    const int64_t nb = off[n];
    std::vector<int32_t> dense((size_t)(4 * nb) + 1);
    stats[0] = host_helitron_scores(n, s, off, n_head, head, n_tail, tail, dense.data());
    if (stats[0] < 0) return -1;
    stats[1] = stats[2] = 0;
    int64_t total = 0;
    std::vector<int32_t> rec, tails;
    for (int64_t q = 0; q < n; q++) {
        const int64_t b = off[q], L = off[q + 1] - b;
        for (int strand = 0; strand < 2; strand++) {
            const int32_t *hs = dense.data() + (2 * strand) * nb + b, *ts = dense.data() + (2 * strand + 1) * nb + b;
            tails.clear(); rec.clear();
            for (int64_t x = 0; x < L; x++) if (ts[x] >= tthr) tails.push_back((int32_t)x);
            stats[2] += (int64_t)tails.size();
            for (int64_t p = 0; p < L; p++) {
                if (hs[p] < hthr) continue;
                stats[1]++;
                auto it = std::lower_bound(tails.begin(), tails.end(), (int32_t)std::min<int64_t>(p + len_min - 1, INT32_MAX));
                if (it == tails.end() || *it - p + 1 > len_max) continue;
                const int32_t t = *it;
                if (strand == 0) { rec.insert(rec.end(), {(int32_t)q, (int32_t)p, t + 1, 0, hs[p], ts[t]}); }
                else { rec.insert(rec.end(), {(int32_t)q, (int32_t)(L - 1 - t), (int32_t)(L - p), 1, hs[p], ts[t]}); }
            }
            const int64_t nr = (int64_t)rec.size() / 6;
            for (int64_t k = 0; k < nr; k++) {        // minus strand: ascending p' is descending (start, end)
                const int32_t *r = &rec[6 * (strand ? nr - 1 - k : k)];
                if (total < cap) std::copy(r, r + 6, out + 6 * total);
                total++;
            }
        }
    }
    stats[3] = total;
    return total;
}
"""

_LIBS = {}


def build(workdir):
    """-> the ctypes library, compiled once per directory"""
    workdir = str(workdir)
    if workdir not in _LIBS:
        src = open(os.path.join(ROOT, "hite_amd", "csrc", "hite_helitron.hip")).read()
        m = re.search(r"// >>> helitron_score.*?\n(.*?)// <<< helitron_score", src, re.S)
        assert m
        cpp, so = os.path.join(workdir, "helitron_host.cpp"), os.path.join(workdir, "helitron_host.so")
        with open(cpp, "w") as f:
            f.write(PRELUDE + m.group(1) + WRAPPER)
        extra = os.environ.get("HITE_HOST_CXXFLAGS", "").split()
        subprocess.run(["g++", "-O2", "-pthread", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include")] + extra + ["-o", so, cpp], check=True)
        lib = C.CDLL(so)
        lib.host_helitron_scores.restype = C.c_int64
        lib.host_helitron_scan.restype = C.c_int64
        _LIBS[workdir] = lib
    return _LIBS[workdir]


def _args(seqs, head, tail):
    from hite_amd._lib import LCV_DTYPE

    sb = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
    off = np.zeros(len(sb) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in sb], out=off[1:])
    buf = np.frombuffer(b"".join(sb) + b"\0" * 16, dtype=np.uint8)
    hp, tp = np.ascontiguousarray(head, dtype=LCV_DTYPE).reshape(-1), np.ascontiguousarray(tail, dtype=LCV_DTYPE).reshape(-1)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    return (buf, off, hp, tp), [C.c_int64(len(sb)), p(buf), p(off), C.c_int32(len(hp)), p(hp), C.c_int32(len(tp)), p(tp)]


def scores(lib, seqs, head, tail):
    """head / tail: LCV_DTYPE records -> int32 [4, total bytes]"""
    keep, args = _args(seqs, head, tail)
    out = np.zeros((4, int(keep[1][-1])), dtype=np.int32)
    assert lib.host_helitron_scores(*args, out.ctypes.data_as(C.c_void_p)) >= 0
    return out


def scan(lib, seqs, head, tail, head_threshold=1, tail_threshold=1, len_range=(200, 20000), stats=None):
    """-> int32 [n, 6], as Context.helitron_scan"""
    keep, args = _args(seqs, head, tail)
    st = np.zeros(4, dtype=np.int64)
    cap = 1 << 12
    while True:
        out = np.zeros((cap, 6), dtype=np.int32)
        n = lib.host_helitron_scan(*args, C.c_int32(head_threshold), C.c_int32(tail_threshold), C.c_int32(len_range[0]), C.c_int32(len_range[1]),
                                   C.c_int64(cap), out.ctypes.data_as(C.c_void_p), st.ctypes.data_as(C.c_void_p))
        assert n >= 0
        if n <= cap:
            break
        cap = n
    if stats is not None:
        stats.update(zip(("anchors", "heads", "tails", "pairs"), (int(v) for v in st)))
    return out[:n].copy()
