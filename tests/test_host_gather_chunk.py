"""The window gather's chunk -> source function (hite_amd/csrc/hite_genome.h, block `gather_chunk`, behind the `genome_decode` block it
calls) compiled for the HOST and run chunk by chunk, against plain slicing + pads built here: a row is `a` pad bytes (the centre's base
they face in lower case, HITE_ROW_PAD where it has none), the window on its strand, `b` pad bytes, or the first 500 + last 500 bytes of
that; every chunk is 16 bytes of the row's slot, the bytes behind the row's length are zero and nothing outside the slot is touched.
   * every window length 100 .. 1100 on both strands, in both forms where the window is longer than 1000;
   * pads 0 / 1 / 15 / 16 / 17 / 31 / 32 / 33 in front and behind, on all four strand combinations of row and centre;
   * pads 499 / 500 / 501 / 520 / 1200 under the first500 + last500 form (chunk 31 holds the seam);
   * centres with clips of their own (the pads are what pad_lengths leaves of the clip words), shorter than the pad, all N;
   * runs of N of 1 .. 33 bases at every offset of a 32-base mask word;
   * windows and centres at genome position 0 and on the last base.
A thinned set goes through a stand-alone program of the same block built with -fsanitize=address,undefined that keeps every array in a
heap buffer of exactly its size (the packed genome: the word of the last base and one more, which is as far as the per-row form of the
gather reads)."""
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

ROW_PAD = 0x2e
GR_MINUS, GR_TRUNC, GR_CMINUS = 1, 2, 4
DESC = np.dtype([("g_lo", "<i8"), ("c_g_lo", "<i8"), ("len", "<i4"), ("c_len", "<i4"), ("a", "<u2"), ("b", "<u2"), ("flags", "<u4")])
assert DESC.itemsize == 32

SHIMS = r"""
#include <string.h>
#include <stdio.h>
#include <stdlib.h>
#define HITE_ROW_PAD 0x2e
struct uint4 { uint32_t x, y, z, w; };
// v_perm_b32 for selectors 0..3 (bytes of the second operand), which is all the decode uses
static inline uint32_t __builtin_amdgcn_perm(uint32_t a, uint32_t b, uint32_t sel) {
    uint32_t out = 0;
    for (int i = 0; i < 4; i++) { const uint32_t s = (sel >> (8 * i)) & 0xffu; out |= ((s < 4 ? b >> (8 * s) : a >> (8 * (s - 4))) & 0xffu) << (8 * i); }
    return out;
}
static inline uint32_t __builtin_bitreverse32(uint32_t x) { uint32_t r = 0; for (int i = 0; i < 32; i++) r |= ((x >> i) & 1u) << (31 - i); return r; }
"""
DRIVER = r"""
static_assert(sizeof(GatherRow) == 32, "the row descriptor is 32 bytes");
extern "C" int host_gather_row(const uint32_t *bases, const uint32_t *nmask, const GatherRow *R, uint8_t *dst) {
    const int nch = (gather_row_len(*R) + 15) >> 4;
    for (int q = 0; q < nch; q++) { const uint4 v = gather_chunk(bases, nmask, *R, q); memcpy(dst + 16 * q, &v, 16); }
    return nch;
}
"""
MAIN = r"""
// records: int64 words of bases, words of nmask, bytes of the slot; the descriptor; bases; nmask; the expected slot
int main(int argc, char **argv) {
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    long n = 0;
    for (;;) {
        int64_t h[3];
        if (fread(h, 8, 3, f) != 3) break;
        GatherRow *R = (GatherRow *)aligned_alloc(16, sizeof(GatherRow));
        uint32_t *bases = (uint32_t *)malloc(h[0] * 4), *nmask = (uint32_t *)malloc(h[1] * 4);
        uint8_t *exp = (uint8_t *)malloc(h[2]), *dst = (uint8_t *)aligned_alloc(16, h[2]);
        if (fread(R, sizeof(GatherRow), 1, f) != 1 || fread(bases, 4, h[0], f) != (size_t)h[0] || fread(nmask, 4, h[1], f) != (size_t)h[1] ||
            fread(exp, 1, h[2], f) != (size_t)h[2]) return 3;
        memset(dst, 0x5a, h[2]);
        if (host_gather_row(bases, nmask, R, dst) * 16 != h[2] || memcmp(dst, exp, h[2])) { fprintf(stderr, "record %ld differs\n", n); return 1; }
        free(R); free(bases); free(nmask); free(exp); free(dst);
        n++;
    }
    fclose(f);
    printf("%ld cases\n", n);
    return 0;
}
"""

_COMP = np.full(256, ord("N"), np.uint8)
_COMP[[65, 67, 71, 84]] = [84, 71, 67, 65]


def _body():
    h = os.path.join(ROOT, "hite_amd", "csrc", "hite_genome.h")
    return SHIMS + _block(h, "genome_decode") + _block(h, "gather_chunk")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("gather_chunk"), "gather_chunk", _body(), DRIVER)


class Genome:
    """a sequence and its packed form in arrays of exactly the words a gather may read: the word of the last base and one more"""

    def __init__(self, seq):
        self.seq = np.ascontiguousarray(seq, dtype=np.uint8)
        G = len(self.seq)
        lut = np.zeros(256, np.uint32)
        lut[[65, 67, 71, 84]] = [0, 1, 2, 3]
        nb, nm = (G + 15) // 16 + 1, (G + 31) // 32 + 1
        codes = np.zeros(nb * 16, np.uint32)
        codes[:G] = lut[self.seq]
        isn = np.zeros(nm * 32, np.uint32)
        isn[:G] = ~np.isin(self.seq, [65, 67, 71, 84])
        self.bases = np.zeros(nb, np.uint32)
        for k in range(16):
            self.bases |= codes[k::16] << np.uint32(2 * k)
        self.nm = np.zeros(nm, np.uint32)
        for k in range(32):
            self.nm |= isn[k::32] << np.uint32(k)

    def window(self, lo, n, minus):
        w = self.seq[lo:lo + n]
        assert len(w) == n and lo >= 0
        return _COMP[w[::-1]] if minus else w


def pad_lengths(clip, minus, clip0, minus0):
    """hite_pipeline.hip: pad_lengths -- the clip words (left | right << 16, in the genome's orientation) of a row and of its centre"""
    ar, br = (clip >> 16, clip & 0xffff) if minus else (clip & 0xffff, clip >> 16)
    a0, b0 = (clip0 >> 16, clip0 & 0xffff) if minus0 else (clip0 & 0xffff, clip0 >> 16)
    return max(0, ar - a0), max(0, br - b0)


def expected(gen, lo, n, minus, a=0, b=0, trunc=False, centre=None):
    w = gen.window(lo, n, minus)
    if a or b:
        c_lo, c_n, c_minus = centre
        cw = gen.window(c_lo, c_n, c_minus) | 0x20
        front = np.array([cw[i] if i < c_n else ROW_PAD for i in range(a)], np.uint8)
        back = np.array([cw[c_n - b + j] if 0 <= c_n - b + j < c_n else ROW_PAD for j in range(b)], np.uint8)
        w = np.concatenate([front, w, back])
    if trunc:
        assert len(w) > 1000
        w = np.concatenate([w[:500], w[-500:]])
    return w


class Runner:
    def __init__(self, lib):
        self.lib, self.n, self.records, self.seam, self.slow_tail = lib, 0, [], 0, 0

    def run(self, gen, lo, n, minus, a=0, b=0, trunc=False, centre=None, keep=False):
        exp = expected(gen, lo, n, minus, a, b, trunc, centre)
        d = np.zeros(1, DESC)
        c_lo, c_n, c_minus = centre if (a or b) else (0, 0, 0)
        d[0] = (lo, c_lo, n, c_n, a, b, (GR_MINUS if minus else 0) | (GR_TRUNC if trunc else 0) | (GR_CMINUS if c_minus else 0))
        L = len(exp)
        slot = (L + 15) & ~15
        buf = np.full(slot + 96, 0x5a, np.uint8)
        start = (-buf.ctypes.data) % 16 + 32
        nch = self.lib.host_gather_row(gen.bases.ctypes.data_as(C.c_void_p), gen.nm.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p),
                                       C.c_void_p(buf.ctypes.data + start))
        what = (lo, n, minus, a, b, trunc, centre)
        assert nch * 16 == slot, what
        got = buf[start:start + L]
        if not np.array_equal(got, exp):
            bad = np.flatnonzero(got != exp)
            raise AssertionError("%r: %d bytes differ, first at %d: %r != %r" % (what, len(bad), bad[0], got[bad[0]:bad[0] + 8].tobytes(), exp[bad[0]:bad[0] + 8].tobytes()))
        assert not buf[start + L:start + slot].any(), (what, "the tail of the last chunk is not zero")
        assert (buf[:start] == 0x5a).all() and (buf[start + slot:] == 0x5a).all(), (what, "wrote outside the slot")
        self.n += 1
        self.seam += trunc
        self.slow_tail += L % 16 != 0
        if keep:
            full = np.zeros(slot, np.uint8)
            full[:L] = exp
            self.records.append(struct.pack("<3q", len(gen.bases), len(gen.nm), slot) + d.tobytes() + gen.bases.tobytes() + gen.nm.tobytes() + full.tobytes())


PADS = (0, 1, 15, 16, 17, 31, 32, 33)
TRUNC_PADS = (499, 500, 501, 520, 1200)


def _all_cases(R):
    rng = np.random.default_rng(19)
    G = 5000 + 7                                          # (the last genome and mask words are partly used)
    seq = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=G)
    seq[rng.integers(0, G, size=40)] = ord("N")
    gen = Genome(seq)
    # every length on both strands, anywhere, at position 0 and on the last base; both forms where the window is longer than 1000
    for n in range(100, 1101):
        for minus in (0, 1):
            for lo in (int(rng.integers(1, G - n)), 0, G - n):
                keep = n in (100, 111, 112, 113, 1000, 1001, 1016, 1100) and lo in (0, G - n)
                R.run(gen, lo, n, minus, keep=keep)
                if n > 1000:
                    R.run(gen, lo, n, minus, trunc=True, keep=keep)
    # pads on all four strand combinations; the row's first base at every offset of a chunk
    for cm in (0, 1):
        centre = (2100, 140, cm)
        for j, (a, b) in enumerate((a, b) for a in PADS for b in PADS):
            for minus in (0, 1):
                R.run(gen, 300 + 37 * j, 100 + j % 16, minus, a, b, centre=centre, keep=(a in (1, 16, 33) and b in (0, 15, 32)))
        for a in range(0, 18):
            R.run(gen, 900, 101, cm, a, 17 - a, centre=centre)
    # ... at genome position 0 and on the last base, rows and centres
    for minus in (0, 1):
        for cm in (0, 1):
            for a, b in ((1, 1), (17, 33), (33, 16), (150, 150)):
                R.run(gen, 0, 100 + a, minus, a, b, centre=(G - 120, 120, cm), keep=True)
                R.run(gen, G - 100 - b, 100 + b, minus, a, b, centre=(0, 120, cm), keep=True)
    # the first500 + last500 form cut from the padded window: a pad that ends before / on / behind the seam, a pad cut by the form
    ab = [(a, 0) for a in (1, 3, 4, 12) + TRUNC_PADS] + [(0, b) for b in (1, 3, 4, 12) + TRUNC_PADS] + [(a, b) for a in TRUNC_PADS for b in TRUNC_PADS] + \
         [(495, 498), (498, 495), (4, 12)]
    for cm in (0, 1):
        for j, (a, b) in enumerate(ab):
            for minus in (0, 1):
                for n in (1001, 1016, 1100):
                    centre = (1500 + j, 1100, cm)
                    R.run(gen, 20 + 3 * j, n, minus, a, b, trunc=True, centre=centre, keep=(n in (1001, 1016) and (a in (0, 499, 1200)) and (b in (0, 501, 1200))))
                    R.run(gen, 20 + 3 * j, n, minus, a, b, centre=centre)
    # centres with clips of their own: the pads are what pad_lengths leaves of the clip words
    for cm in (0, 1):
        clip0 = 5 | (7 << 16)
        for minus in (0, 1):
            for left in (0, 4, 5, 6, 17, 33):
                for right in (0, 6, 7, 8, 17, 33):
                    a, b = pad_lengths(left | (right << 16), minus, clip0, cm)
                    R.run(gen, 600 + left, 100 + right, minus, a, b, centre=(2400, 140, cm), keep=(left == 17 and right in (0, 8)))
    # a centre shorter than the pad: HITE_ROW_PAD where it has no base
    for cm in (0, 1):
        for minus in (0, 1):
            for a in (0, 99, 100, 101, 150):
                for b in (0, 99, 100, 101, 150):
                    R.run(gen, 1300, 107, minus, a, b, centre=(2700, 100, cm), keep=(a == 101 and b in (0, 150)))
    # a centre of N
    nseq = seq.copy()
    nseq[3000:3200] = ord("N")
    ngen = Genome(nseq)
    for cm in (0, 1):
        for minus in (0, 1):
            for a, b in ((0, 1), (1, 0), (16, 33), (33, 16), (40, 40)):
                R.run(ngen, 700, 109, minus, a, b, centre=(3010, 120, cm), keep=(a == 16))
                R.run(ngen, 700, 109, minus, a, b, centre=(2950, 120, cm))
    # runs of N of 1 .. 33 bases at every offset of a 32-base mask word: in front of, inside and at the end of a window
    for Lr in range(1, 34):
        s = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=32 * 192 + 300)
        at = [192 * k + 128 + k for k in range(32)]                  # offsets 0 .. 31 of a mask word (192 = 6 words)
        assert sorted(p % 32 for p in at) == list(range(32))
        for p in at:
            s[p:p + Lr] = ord("N")
        g2 = Genome(s)
        for p in at:
            for minus in (0, 1):
                R.run(g2, p, 100 + p % 16, minus, keep=(Lr in (1, 16, 17, 32, 33) and p % 32 in (0, 1, 15, 16, 31)))
                R.run(g2, p - 30, 110 + Lr, minus)
                R.run(g2, p + Lr - 104, 104, minus)


def test_gather_chunk_vs_slicing(lib, tmp_path):
    R = Runner(lib)
    _all_cases(R)
    assert R.n > 14000 and R.seam > 1000 and R.slow_tail > 10000, (R.n, R.seam, R.slow_tail)
    assert 200 <= len(R.records) <= 900, len(R.records)
    cpp, exe, data = tmp_path / "gather_main.cpp", tmp_path / "gather_main", tmp_path / "cases.bin"
    cpp.write_text(PRELUDE + _body() + DRIVER + MAIN)
    data.write_bytes(b"".join(R.records))
    # (the sanitizer runtimes linked statically: the program does not depend on what else the process has loaded before it)
    subprocess.run(["g++", "-O1", "-g", "-static-libasan", "-static-libubsan", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", str(exe), str(cpp)], check=True)
    res = subprocess.run([str(exe), str(data)], capture_output=True, text=True)
    assert res.returncode == 0 and not res.stderr.strip(), (res.returncode, res.stderr[-3000:])
    assert res.stdout.strip() == "%d cases" % len(R.records)
