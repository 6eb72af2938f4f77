"""The `host_arena` block of hite_amd/csrc/hite_arena.h (the grow-only device arenas of the drivers: arena_alloc, the typed
arena_get, the soft and the hard reset) is plain host C++: it is cut out between its markers, compiled with g++ against stand-ins
of the three HIP calls it makes, and called here.  The stand-in hipMalloc hands out distinct fake addresses, counts its calls and
can be told to fail; nothing is dereferenced.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIB = 1 << 20
CHUNK = 256 * MIB          # the smallest chunk
HITE_OK, HITE_EHIP = 0, -3

PRELUDE = r"""
#include <stddef.h>
#include <stdint.h>
#include <vector>
#define HITE_OK 0
#define HITE_EHIP (-3)
struct hite_ctx { int errors; };
typedef int hipError_t;
static const hipError_t hipSuccess = 0;
static uint64_t g_next = 1ull << 40;
static int g_mallocs = 0, g_frees = 0, g_syncs = 0, g_fail_at = 0;
// distinct fake addresses, 4096-aligned with a gap behind every block; the g_fail_at-th call (counted from 1; 0: none) fails
static hipError_t hipMalloc(void **p, size_t n) {
    g_mallocs++;
    if (g_fail_at && g_mallocs == g_fail_at) return 2;
    *p = (void *)(uintptr_t)g_next;
    g_next += ((uint64_t)n + 4095) / 4096 * 4096 + 4096;
    return hipSuccess;
}
static hipError_t hipFree(void *) { g_frees++; return hipSuccess; }
static hipError_t hipDeviceSynchronize() { g_syncs++; return hipSuccess; }
#define HITE_CHECK(ctx, call) do { if ((call) != hipSuccess) { if (ctx) (ctx)->errors++; return HITE_EHIP; } } while (0)
"""

WRAPPER = r"""
struct E12 { uint32_t w[3]; };
struct E24 { uint64_t w[3]; };
static hite_ctx g_ctx = {0};
extern "C" void *h_new() { return new Arena(); }
extern "C" void h_del(void *a) { arena_free(*(Arena *)a); delete (Arena *)a; }
extern "C" int h_alloc(void *a, uint64_t bytes, uint64_t *ptr) {
    void *p = nullptr;
    const int rc = arena_alloc(&g_ctx, *(Arena *)a, (size_t)bytes, &p);
    *ptr = (uint64_t)(uintptr_t)p;
    return rc;
}
template <class T> static int get_as(Arena &a, uint64_t count, uint64_t *ptr) {
    T *p = nullptr;
    const int rc = arena_get(&g_ctx, a, (size_t)count, &p);
    *ptr = (uint64_t)(uintptr_t)p;
    return rc;
}
extern "C" int h_get(void *a, int elem, uint64_t count, uint64_t *ptr) {
    Arena &A = *(Arena *)a;
    switch (elem) {
        case 1: return get_as<uint8_t>(A, count, ptr);
        case 4: return get_as<uint32_t>(A, count, ptr);
        case 8: return get_as<uint64_t>(A, count, ptr);
        case 12: return get_as<E12>(A, count, ptr);
        case 24: return get_as<E24>(A, count, ptr);
    }
    return -100;
}
// the several-arrays form: four arrays of `count` elements of 4, 12, 1 and 8 bytes
extern "C" int h_get4(void *a, uint64_t count, uint64_t *ptr) {
    uint32_t *p0 = nullptr; E12 *p1 = nullptr; uint8_t *p2 = nullptr; uint64_t *p3 = nullptr;
    const int rc = arena_get(&g_ctx, *(Arena *)a, (size_t)count, &p0, &p1, &p2, &p3);
    ptr[0] = (uint64_t)(uintptr_t)p0; ptr[1] = (uint64_t)(uintptr_t)p1; ptr[2] = (uint64_t)(uintptr_t)p2; ptr[3] = (uint64_t)(uintptr_t)p3;
    return rc;
}
extern "C" int h_reset(void *a, int hard) { return arena_reset(&g_ctx, *(Arena *)a, hard != 0); }
extern "C" int h_chunks(void *a, uint64_t *base, uint64_t *caps, int max) {
    const Arena &A = *(Arena *)a;
    for (size_t i = 0; i < A.chunks.size() && (int)i < max; i++) { base[i] = (uint64_t)(uintptr_t)A.chunks[i]; caps[i] = A.caps[i]; }
    return (int)A.chunks.size();
}
// counters of the stand-ins: mallocs, frees, synchronisations, errors noted in the context
extern "C" void fake_counts(int *out) { out[0] = g_mallocs; out[1] = g_frees; out[2] = g_syncs; out[3] = g_ctx.errors; }
extern "C" void fake_fail_at(int k) { g_fail_at = k ? g_mallocs + k : 0; }     // the k-th hipMalloc from now fails
extern "C" void fake_rewind() { g_next = 1ull << 40; }                          // the next arena gets the addresses of the first again
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    src = open(os.path.join(ROOT, "hite_amd", "csrc", "hite_arena.h")).read()
    m = re.search(r"// >>> host_arena.*?\n(.*?)// <<< host_arena", src, re.S)
    assert m
    d = tmp_path_factory.mktemp("host_arena")
    cpp, so = d / "host_arena.cpp", d / "host_arena.so"
    cpp.write_text(PRELUDE + m.group(1) + WRAPPER)
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", str(so), str(cpp)], check=True)
    L = C.CDLL(str(so))
    L.h_new.restype = C.c_void_p
    return L


class Arena:
    def __init__(self, lib):
        self.lib, self.h = lib, C.c_void_p(lib.h_new())

    def close(self):
        self.lib.h_del(self.h)

    def alloc(self, nbytes):
        p = C.c_uint64(0)
        return self.lib.h_alloc(self.h, C.c_uint64(nbytes), C.byref(p)), p.value

    def get(self, elem, count):
        p = C.c_uint64(0)
        return self.lib.h_get(self.h, elem, C.c_uint64(count), C.byref(p)), p.value

    def reset(self, hard):
        return self.lib.h_reset(self.h, 1 if hard else 0)

    def chunks(self):
        base, caps = (C.c_uint64 * 64)(), (C.c_uint64 * 64)()
        n = self.lib.h_chunks(self.h, base, caps, 64)
        assert n <= 64
        return [(int(base[i]), int(caps[i])) for i in range(n)]


@pytest.fixture
def arena(lib):
    lib.fake_fail_at(0)
    a = Arena(lib)
    yield a
    lib.fake_fail_at(0)
    a.close()


def _counts(lib):
    out = (C.c_int * 4)()
    lib.fake_counts(out)
    return dict(mallocs=out[0], frees=out[1], syncs=out[2], errors=out[3])


def _delta(lib, before):
    now = _counts(lib)
    return {k: now[k] - before[k] for k in now}


def _rounded(nbytes):
    return max(256, (nbytes + 255) // 256 * 256)


def _chunk_of(chunks, p):
    hit = [(b, c) for b, c in chunks if b <= p < b + c]
    assert len(hit) == 1, (p, chunks)
    return hit[0]


def _random_sizes(rng, n, big):
    """byte counts: zeros, ones, sizes around the 256-byte grain, and a few large enough (`big`) to leave the chunk"""
    out = []
    for _ in range(n):
        kind = int(rng.integers(0, 6))
        out.append([0, 1, int(rng.integers(1, 1024)), 256 * int(rng.integers(1, 9)), int(rng.integers(1, 5 * MIB)),
                    int(rng.integers(MIB, big))][kind])
    return out


def test_rounding(lib, arena):
    """every allocation starts at a multiple of 256 and owns max(256, the request rounded up to 256) bytes of ONE chunk: inside a
    chunk the next allocation starts exactly behind it, and none overlaps another"""
    rng = np.random.default_rng(7)
    sizes = _random_sizes(rng, 300, 90 * MIB)
    got = []
    for s in sizes:
        rc, p = arena.alloc(s)
        assert rc == HITE_OK and p % 256 == 0, (s, p)
        got.append(p)
    chunks = arena.chunks()
    assert len(chunks) > 1                                        # (the list leaves the first chunk)
    assert sizes.count(0) > 10
    for i, (s, p) in enumerate(zip(sizes, got)):
        b, c = _chunk_of(chunks, p)
        assert p + _rounded(s) <= b + c, (i, s)                   # owns its bytes inside the chunk
        if i + 1 < len(got) and _chunk_of(chunks, got[i + 1]) == (b, c):
            assert got[i + 1] == p + _rounded(s), (i, s)          # 0 bytes: 256
        elif i + 1 < len(got):
            assert got[i + 1] == _chunk_of(chunks, got[i + 1])[0], i          # a new chunk is filled from its start
    spans = sorted((p, p + _rounded(s)) for s, p in zip(sizes, got))
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))


def test_typed_helper_matches_byte_allocator(lib):
    """arena_get<T>(count) yields the pointers arena_alloc yields for count * sizeof(T), over random lists of element sizes 1, 4,
    8, 12 and 24 (the fake addresses start over for the second arena, so equal requests give equal pointers)"""
    rng = np.random.default_rng(11)
    for case in range(40):
        n = int(rng.integers(1, 40))
        reqs = []
        for _ in range(n):
            elem = int(rng.choice([1, 4, 8, 12, 24]))
            count = int(rng.choice([0, 1, int(rng.integers(0, 700)), int(rng.integers(0, 1 << 16)), int(rng.integers(0, 1 << 23))]))
            reqs.append((elem, count))
        lib.fake_rewind()
        a = Arena(lib)
        want = [a.alloc(e * c) for e, c in reqs]
        want_chunks = a.chunks()
        a.close()
        lib.fake_rewind()
        b = Arena(lib)
        got = [b.get(e, c) for e, c in reqs]
        got_chunks = b.chunks()
        b.close()
        assert all(rc == HITE_OK for rc, _ in want)
        assert got == want and got_chunks == want_chunks, (case, reqs)
    lib.fake_rewind()
    a = Arena(lib)
    assert a.get(3, 1)[0] == -100           # (the wrapper knows the five sizes only)
    a.close()


def test_several_arrays_of_one_count(lib):
    """arena_get(count, &a, &b, &c, &d) allocates count elements for each, in the order named: the pointers of four single requests"""
    for count in (0, 1, 85, 4097, (1 << 24) + 5):
        lib.fake_rewind()
        a = Arena(lib)
        assert a.alloc(40)[0] == HITE_OK
        want = [a.alloc(e * count)[1] for e in (4, 12, 1, 8)]
        a.close()
        lib.fake_rewind()
        b = Arena(lib)
        assert b.alloc(40)[0] == HITE_OK
        got = (C.c_uint64 * 4)()
        assert lib.h_get4(b.h, C.c_uint64(count), got) == HITE_OK
        b.close()
        assert [int(x) for x in got] == want, count


def test_growth(lib, arena):
    """the first chunk holds 256 MiB; a request beyond the room left opens a chunk at least as large as the request, as 256 MiB and
    as everything held so far"""
    c0 = _counts(lib)
    assert arena.alloc(100)[0] == HITE_OK
    assert [c for _, c in arena.chunks()] == [CHUNK]
    assert arena.alloc(CHUNK - 256)[0] == HITE_OK                                  # exactly the room left: no new chunk
    assert len(arena.chunks()) == 1
    assert arena.alloc(1)[0] == HITE_OK                                            # full: a second chunk, of everything held so far
    assert [c for _, c in arena.chunks()] == [CHUNK, CHUNK]
    assert arena.alloc(300 * MIB)[0] == HITE_OK                                    # 512 MiB held > the request
    assert [c for _, c in arena.chunks()] == [CHUNK, CHUNK, 2 * CHUNK]
    rc, p = arena.alloc(2000 * MIB + 3)                                            # the request > the 1024 MiB held
    assert rc == HITE_OK
    caps = [c for _, c in arena.chunks()]
    assert caps[:3] == [CHUNK, CHUNK, 2 * CHUNK] and caps[3] >= 2000 * MIB + 3 and len(caps) == 4
    assert p == arena.chunks()[3][0]
    held = sum(caps)
    assert arena.alloc(10 * MIB)[0] == HITE_OK                                     # chunk 4 is full to the last byte
    caps = [c for _, c in arena.chunks()]
    assert len(caps) == 5 and caps[4] >= held
    assert _delta(lib, c0) == dict(mallocs=5, frees=0, syncs=0, errors=0)


def test_soft_reset_hands_the_same_memory_out(lib, arena):
    rng = np.random.default_rng(23)
    sizes = _random_sizes(rng, 200, 120 * MIB)
    first = [arena.alloc(s) for s in sizes]
    assert len(arena.chunks()) > 1
    c0 = _counts(lib)
    for _ in range(2):
        assert arena.reset(False) == HITE_OK
        assert [arena.alloc(s) for s in sizes] == first
    assert _delta(lib, c0) == dict(mallocs=0, frees=0, syncs=0, errors=0)


def test_hard_reset_merges_the_chunks(lib, arena):
    """with more than one chunk: one synchronisation, every chunk freed, ONE chunk of the summed capacity; the same requests then
    fit without a further hipMalloc.  With one chunk a hard reset is a soft one"""
    rng = np.random.default_rng(29)
    sizes = _random_sizes(rng, 200, 120 * MIB)
    for s in sizes:
        assert arena.alloc(s)[0] == HITE_OK
    before = arena.chunks()
    assert len(before) > 1
    c0 = _counts(lib)
    assert arena.reset(True) == HITE_OK
    assert _delta(lib, c0) == dict(mallocs=1, frees=len(before), syncs=1, errors=0)
    after = arena.chunks()
    assert len(after) == 1 and after[0][1] == sum(c for _, c in before)
    assert after[0][0] not in [b for b, _ in before]
    c1 = _counts(lib)
    got = [arena.alloc(s) for s in sizes]
    assert all(rc == HITE_OK for rc, _ in got)
    assert got[0][1] == after[0][0]
    assert arena.chunks() == after
    assert arena.reset(True) == HITE_OK                       # one chunk: nothing to merge
    assert arena.chunks() == after and arena.alloc(5)[1] == after[0][0]
    assert _delta(lib, c1) == dict(mallocs=0, frees=0, syncs=0, errors=0)


def test_failing_hipmalloc_leaves_the_arena_usable(lib, arena):
    c0 = _counts(lib)
    lib.fake_fail_at(1)                                       # an empty arena's first chunk
    assert arena.alloc(100)[0] == HITE_EHIP and arena.chunks() == []
    lib.fake_fail_at(0)
    rc, p0 = arena.alloc(100)
    assert rc == HITE_OK and arena.chunks() == [(p0, CHUNK)]
    lib.fake_fail_at(1)                                       # growth
    assert arena.alloc(CHUNK)[0] == HITE_EHIP
    assert arena.chunks() == [(p0, CHUNK)]                    # what it held stays
    assert _delta(lib, c0) == dict(mallocs=3, frees=0, syncs=0, errors=2)
    lib.fake_fail_at(0)
    rc, p1 = arena.alloc(CHUNK)
    assert rc == HITE_OK and len(arena.chunks()) == 2 and p1 == arena.chunks()[1][0]
    lib.fake_fail_at(1)                                       # the hard reset's one chunk: the old chunks are gone, the arena is empty
    c1 = _counts(lib)
    assert arena.reset(True) == HITE_EHIP
    assert _delta(lib, c1) == dict(mallocs=1, frees=2, syncs=1, errors=1)
    assert arena.chunks() == []
    lib.fake_fail_at(0)
    rc, p2 = arena.alloc(3 * CHUNK)
    assert rc == HITE_OK and arena.chunks() == [(p2, 3 * CHUNK)]
    assert arena.reset(True) == HITE_OK and arena.alloc(1)[1] == p2
