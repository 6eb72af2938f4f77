"""The `host_plan` block of hite_amd/csrc/hite_hostbuf.h (the layout of a block carved from the context's scratch, the check of an
offset table, the check of a pair of intervals) is plain host C++: it is cut out between its markers, compiled with g++ and called
here.  No GPU needed; the GPU tests of the four stages that carve their scratch with it cover what the kernels then do there."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PRELUDE = r"""
#include <stddef.h>
#include <stdint.h>
#include <initializer_list>
#include <vector>
"""

WRAPPER = r"""
// spec: n x (element size, count, extra bytes) -> off[n], ptr[n] (as integers, from `base`); returns the total
extern "C" uint64_t host_plan(const uint64_t *spec, int n, uint64_t base, uint64_t *off, uint64_t *ptr) {
    std::vector<BufSpec> bufs;
    for (int i = 0; i < n; i++) bufs.push_back(BufSpec{(size_t)spec[3 * i], (size_t)spec[3 * i + 1], (size_t)spec[3 * i + 2]});
    const ScratchPlan plan(bufs.data(), bufs.size());
    for (int i = 0; i < n; i++) { off[i] = plan.off[i]; ptr[i] = (uint64_t)(uintptr_t)plan.at<uint8_t>((void *)(uintptr_t)base, i); }
    return plan.total;
}
extern "C" int host_csr_ok(const int64_t *off, int64_t n) { return csr_ok(off, n) ? 1 : 0; }
extern "C" int host_interval_pair(int64_t n_seq, const int64_t *seq_off, int64_t a_id, int64_t a_start, int64_t a_end, int64_t b_id,
                                  int64_t b_start, int64_t b_end, int64_t min_len, int64_t max_len, int64_t *m, int64_t *n) {
    return interval_pair_ok(n_seq, seq_off, a_id, a_start, a_end, b_id, b_start, b_end, min_len, max_len, m, n) ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    src = open(os.path.join(ROOT, "hite_amd", "csrc", "hite_hostbuf.h")).read()
    m = re.search(r"// >>> host_plan.*?\n(.*?)// <<< host_plan", src, re.S)
    assert m
    d = tmp_path_factory.mktemp("host_plan")
    cpp, so = d / "host_plan.cpp", d / "host_plan.so"
    cpp.write_text(PRELUDE + m.group(1) + WRAPPER)
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", str(so), str(cpp)], check=True)
    L = C.CDLL(str(so))
    L.host_plan.restype = C.c_uint64
    return L


def _plan(lib, bufs, base=0):
    spec = np.array(bufs, dtype=np.uint64).reshape(-1)
    off, ptr = np.zeros(len(bufs), np.uint64), np.zeros(len(bufs), np.uint64)
    u64p = C.POINTER(C.c_uint64)
    total = lib.host_plan(spec.ctypes.data_as(u64p), len(bufs), C.c_uint64(base), off.ctypes.data_as(u64p), ptr.ctypes.data_as(u64p))
    return [int(x) for x in off], int(total), [int(x) for x in ptr]


def test_layout_random_lists(lib):
    """every buffer starts at a multiple of 256 behind the one before it, owns at least what it asked for and at least 256 bytes; the
    total is the sum of the rounded sizes; a pointer is the base plus the offset"""
    rng = np.random.default_rng(41)
    n_zero = n_extra = 0
    for case in range(400):
        n = int(rng.integers(1, 13))
        bufs = []
        for _ in range(n):
            count = int(rng.choice([0, 1, int(rng.integers(0, 300)), int(rng.integers(0, (1 << 20) + 1)), 1 << 20]))
            extra = int(rng.choice([0, 0, 4, 16, 32]))
            bufs.append((int(rng.choice([1, 4, 8, 12, 24, 28])), count, extra))
        base = int(rng.integers(1, 1 << 40)) * 256
        off, total, ptr = _plan(lib, bufs, base)
        asked = [e * c + x for e, c, x in bufs]
        rounded = [max(256, (a + 255) // 256 * 256) for a in asked]
        ends = off[1:] + [total]
        assert off[0] == 0 and all(o % 256 == 0 for o in off), (case, off)
        assert all(b > a for a, b in zip(off, ends)), (case, off)                         # strictly increasing
        assert all(e - o >= a for o, e, a in zip(off, ends, asked)), (case, off, asked)
        assert all(e - o == 256 for o, e, a in zip(off, ends, asked) if a == 0), (case, off, asked)
        assert [e - o for o, e in zip(off, ends)] == rounded and total == sum(rounded), (case, off, total)
        assert [p - base for p in ptr] == off, case
        n_zero += sum(a == 0 for a in asked)
        n_extra += sum(x > 0 for _, _, x in bufs)
    assert n_zero > 50 and n_extra > 500


# One list per stage that carves its scratch with the helper, as the stage writes it, at a batch of one and at a batch of three with
# odd byte counts.  The expected offsets are worked out by hand from the formulas the stages had before the helper:
# up(x) = (x + 255) & ~255, each buffer behind the one before it.
STAGE_CASES = [
    # hite_pair_identity: up(bytes + 16), up(batch * sizeof(IdentTask) = 32), batch * 8
    ("ident-1", [(1, 241, 16), (32, 1, 0), (8, 1, 0)], [0, 512, 768], 1024),              # 257 -> 512 (the + 16 tail), 32 -> 256, 8 -> 256
    ("ident-3", [(1, 1001, 16), (32, 3, 0), (8, 3, 0)], [0, 1024, 1280], 1536),           # 1017 -> 1024, 96 -> 256, 24 -> 256
    # hite_pair_hsps: up(bytes + 16), up(nt * sizeof(PhTask) = 24), up(nt * 84 * 4), up(blocks * table_words * 4)
    ("pairhsp-1", [(1, 11, 16), (24, 1, 0), (4, 84, 0), (4, 256, 0)], [0, 256, 512, 1024], 2048),             # 27, 24, 336 -> 512, 1024
    ("pairhsp-3", [(1, 245, 16), (24, 3, 0), (4, 252, 0), (4, 2688, 0)], [0, 512, 768, 1792], 12544),         # 261 -> 512, 72, 1008 -> 1024, 10752
    # hite_frame_cluster: up(bytes + 16), up(units * sizeof(FcUnit) = 24), up(rows * sizeof(FcRow) = 12), up(rows * 4)
    ("framecluster-1", [(1, 250, 16), (24, 1, 0), (12, 3, 0), (4, 3, 0)], [0, 512, 768, 1024], 1280),         # 266 -> 512, 24, 36, 12
    ("framecluster-3", [(1, 1013, 16), (24, 3, 0), (12, 23, 0), (4, 23, 0)], [0, 1280, 1536, 2048], 2304),    # 1029 -> 1280, 72, 276 -> 512, 92
    # hite_msa_subcluster: up(bytes + 32), up(n * sizeof(SubTask) = 32), up(rows * 4 + 4), up(n * 4), up(max_rows * 4 + 4), up(64 * 4), up(64 * 8)
    ("subcluster-1", [(1, 230, 32), (32, 1, 0), (4, 5, 4), (4, 1, 0), (4, 0, 4), (4, 64, 0), (8, 64, 0)],
     [0, 512, 768, 1024, 1280, 1536, 1792], 2304),                                        # 262 -> 512, 32, 24, 4, 4, 256, 512
    ("subcluster-3", [(1, 999, 32), (32, 3, 0), (4, 127, 4), (4, 3, 0), (4, 70, 4), (4, 64, 0), (8, 64, 0)],
     [0, 1280, 1536, 2048, 2304, 2816, 3072], 3584),                                      # 1031 -> 1280, 96, 512 -> 512, 12, 284 -> 512, 256, 512
]


@pytest.mark.parametrize("label,bufs,want_off,want_total", STAGE_CASES, ids=[c[0] for c in STAGE_CASES])
def test_layout_of_the_stages(lib, label, bufs, want_off, want_total):
    off, total, _ptr = _plan(lib, bufs)
    assert (off, total) == (want_off, want_total)


def _csr(lib, off, n):
    a = np.array(off, dtype=np.int64)
    return bool(lib.host_csr_ok(a.ctypes.data_as(C.POINTER(C.c_int64)), C.c_int64(n)))


def test_csr_ok(lib):
    assert bool(lib.host_csr_ok(None, C.c_int64(0)))              # no piece: nothing is read
    assert _csr(lib, [7, 7, 7, 7], 3)                             # empty pieces
    assert _csr(lib, [0, 3, 3, 10], 3)
    assert not _csr(lib, [-1, 3, 3, 10], 3)                       # negative first offset
    assert not _csr(lib, [5, 4, 6, 10], 3)                        # a step down at the first position
    assert not _csr(lib, [0, 3, 10, 9], 3)                        # ... at the last


def _pair(lib, seq_off, a, b, min_len, max_len):
    so = np.array(seq_off, dtype=np.int64)
    m, n = C.c_int64(-7), C.c_int64(-7)
    ok = lib.host_interval_pair(C.c_int64(len(seq_off) - 1), so.ctypes.data_as(C.POINTER(C.c_int64)), *[C.c_int64(v) for v in a + b],
                                C.c_int64(min_len), C.c_int64(max_len), C.byref(m), C.byref(n))
    return (m.value, n.value) if ok else None


def test_interval_pair(lib):
    seq_off = [100, 140, 140, 200]          # lengths 40, 0, 60
    good = (0, 3, 30)
    assert _pair(lib, seq_off, good, (2, 0, 60), 0, 100) == (27, 60)
    assert _pair(lib, seq_off, (2, 10, 60), good, 0, 100) == (50, 27)
    for bad in [(-1, 0, 1), (3, 0, 1), (0, -1, 5), (0, 6, 5), (0, 0, 41), (2, 0, 61)]:          # id = -1, id = n_seq, start < 0, end < start, end = len + 1
        assert _pair(lib, seq_off, bad, good, 0, 100) is None, bad
        assert _pair(lib, seq_off, good, bad, 0, 100) is None, bad
    assert _pair(lib, seq_off, (0, 0, 40), (2, 60, 60), 0, 100) == (40, 0)                      # end = len; an empty interval at the end
    assert _pair(lib, seq_off, (2, 5, 35), good, 0, 30) == (30, 27)                             # length = max_len
    assert _pair(lib, seq_off, (2, 5, 36), good, 0, 30) is None                                 # max_len + 1
    assert _pair(lib, seq_off, good, (2, 5, 36), 0, 30) is None
    assert _pair(lib, seq_off, (1, 0, 0), (0, 9, 9), 0, 30) == (0, 0)                           # length 0 with min_len 0
    assert _pair(lib, seq_off, (1, 0, 0), good, 1, 30) is None                                  # ... and with min_len 1
    assert _pair(lib, seq_off, good, (0, 9, 9), 1, 30) is None
