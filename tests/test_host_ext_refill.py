"""The copy finder's end extension (hite_ext.h, copy mode) takes its bases from per-lane windows that are refilled 16 bases at a
time.  The block is compiled for the host as tests/test_host_compiled.py does it and driven in three ways that must agree with the
twin (oracle/hite_oracle_copies.c: ext_align) and with each other on (best_i, best_t):
  - ext_align_dev (refills every 16 columns itself),
  - ext_step alone (the windows run empty and ext_step refills them on the spot),
  - ext_step with ext_refill at the columns k with (k + phase) % 16 == 0, for every phase 0..15 (chain_extend_kernel's schedule as a
    lane sees it that took its task `phase` columns into a period).
Cases: both directions, both byte orders, both strands, the query starting at every byte offset of 16, the genome at several offsets
of a mask word, lengths around every multiple of 16, N runs and non-ACGT bytes on both sides of a chunk edge, the contig end at every
offset of a chunk, genome word 0, byte 0 of the candidate buffer and the last candidate of a buffer with 16 bytes behind it.
A subset of the cases goes to a stand-alone program of the same block, built with -fsanitize=address,undefined, that holds every
array in a heap buffer of exactly its size (packed genome: the words that hold bases; candidates: 16 bytes behind the last one)."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle_lib as O  # noqa: E402
from test_host_compiled import PRELUDE, _block, _build  # noqa: E402

SLACK = 16              # include/hite_gpu.h: d_cand is readable for 16 bytes beyond cand_bytes
NS = (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 300)
G0MOD = (0, 1, 15, 16, 17, 31)
COMP = np.full(256, ord("N"), np.uint8)
COMP[[65, 67, 71, 84]] = [84, 71, 67, 65]

DRIVER = r"""
static uint32_t g_lut[EXT_LUT_WORDS];
static bool g_lut_ready = false;
static const uint32_t *host_lut() {
    if (!g_lut_ready) { for (int t = 0; t < EXT_LUT_WORDS; t++) g_lut[t] = ext_lut_entry(t >> 8, t & 255); g_lut_ready = true; }
    return g_lut;
}
// mode 0: ext_align_dev; 1: ext_step alone; 2: ext_step + ext_refill at the columns k with (k + phase) % 16 == 0
static void drive(int mode, int phase, const uint8_t *q, int64_t p0, int step, int comp, int n, const uint32_t *bases, const uint32_t *nmask,
                  int64_t g0, int dir, int64_t jmax, int *io, int *to) {
    if (mode == 0) {
        int s;
        ext_align_dev<ExtCopyMode>(q, p0, step, comp != 0, n, bases, nmask, g0, dir, jmax, -EXT_B, EXT_B, io, to, &s, host_lut());
        return;
    }
    ExtStateT<ExtCopyMode> E;
    ext_init(E, q, p0, step, comp != 0, n, bases, nmask, g0, dir, jmax);
    if (n >= 1) for (int k = 0;; k++) {
        if (mode == 2 && (k + phase) % 16 == 0) ext_refill(E, q, bases, nmask);
        if (ext_step(E, bases, nmask, host_lut())) break;
    }
    *io = E.best_i; *to = E.best_t;
}
// all 18 ways; 0 if they agree (result in *io / *to), else 1 + the number of the first way that differs from ext_align_dev
extern "C" int host_ext_all(const uint8_t *q, int64_t p0, int step, int comp, int n, const uint32_t *bases, const uint32_t *nmask,
                            int64_t g0, int dir, int64_t jmax, int *io, int *to) {
    drive(0, 0, q, p0, step, comp, n, bases, nmask, g0, dir, jmax, io, to);
    for (int w = 1; w < 18; w++) {
        int i2 = -1, t2 = -1;
        drive(w == 1 ? 1 : 2, w - 2, q, p0, step, comp, n, bases, nmask, g0, dir, jmax, &i2, &t2);
        if (i2 != *io || t2 != *to) return 1 + w;
    }
    return 0;
}
"""

# the stand-alone program: records of 12 int64 (p0, step, comp, n, g0, dir, jmax, genome words, mask words, candidate bytes, expected
# i, expected t) followed by the three arrays; every array is copied into a heap buffer of exactly its size
MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
int main(int argc, char **argv) {
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t h[12];
    long n_cases = 0;
    while (fread(h, 8, 12, f) == 12) {
        uint32_t *bases = (uint32_t *)malloc((size_t)h[7] * 4), *nmask = (uint32_t *)malloc((size_t)h[8] * 4);
        uint8_t *q = (uint8_t *)malloc((size_t)h[9]);
        if (fread(bases, 4, (size_t)h[7], f) != (size_t)h[7] || fread(nmask, 4, (size_t)h[8], f) != (size_t)h[8] || fread(q, 1, (size_t)h[9], f) != (size_t)h[9]) return 3;
        int io = -1, to = -1;
        const int bad = host_ext_all(q, h[0], (int)h[1], (int)h[2], (int)h[3], bases, nmask, h[4], (int)h[5], h[6], &io, &to);
        if (bad || io != (int)h[10] || to != (int)h[11]) { fprintf(stderr, "case %ld: way %d, got %d %d, expected %ld %ld\n", n_cases, bad, io, to, (long)h[10], (long)h[11]); return 1; }
        free(bases); free(nmask); free(q);
        n_cases++;
    }
    fclose(f);
    printf("%ld cases\n", n_cases);
    return n_cases > 0 ? 0 : 4;
}
"""


def _body():
    return "#define EXT_LUT_PTR const uint32_t *\n" + _block(os.path.join(ROOT, "hite_amd", "csrc", "hite_ext.h"), "ext_align_dev")


def _pack_exact(genome):
    """the packed genome with no word beyond the last one that holds a base"""
    G = len(genome)
    lut = np.zeros(256, np.uint32)
    lut[[65, 67, 71, 84]] = [0, 1, 2, 3]
    codes = np.zeros((G + 15) // 16 * 16, np.uint32)
    codes[:G] = lut[genome]
    bases = np.zeros((G + 15) // 16, np.uint32)
    for k in range(16):
        bases |= codes[k::16] << np.uint32(2 * k)
    isn = np.zeros((G + 31) // 32 * 32, np.uint32)
    isn[:G] = ~np.isin(genome, [65, 67, 71, 84])
    nm = np.zeros((G + 31) // 32, np.uint32)
    for k in range(32):
        nm |= isn[k::32] << np.uint32(k)
    return bases, nm


class Genome:
    def __init__(self, genome):
        self.bytes = np.ascontiguousarray(genome)
        self.bases, self.nm = _pack_exact(self.bytes)


def _walk(genome, g0, d, n):
    return genome[g0:g0 + n] if d > 0 else genome[max(0, g0 - n):g0][::-1]


def _diverged(rng, walk, n):
    """n query bases in walking order: the genome walked over with a substitution every ~17 bases, one base left out, one put in"""
    seg = [int(b) if b in (65, 67, 71, 84) else 65 for b in walk]
    for k in range(5, len(seg), 17):
        seg[k] = int(rng.choice([65, 67, 71, 84]))
    if len(seg) > 60:
        del seg[41]
        seg.insert(23, 71)
    while len(seg) < n:
        seg.append(int(rng.choice([65, 67, 71, 84])))
    return np.array(seg[:n], np.uint8)


def _layout(seg, step, strand, before, behind=SLACK):
    """the candidate buffer that holds the segment as the kernel reads it: `before` bytes, the stored bases, `behind` bytes -> (q, p0)"""
    stored = COMP[seg] if strand else seg.copy()
    if step < 0:
        stored = stored[::-1]
    q = np.concatenate([np.full(before, ord("T"), np.uint8), stored, np.full(behind, ord("G"), np.uint8)])
    p0 = before if step > 0 else before + len(seg) - 1
    return np.ascontiguousarray(q), p0


class Runner:
    """runs a case through the 18 ways of the host build and the twin; keeps the cases marked for the stand-alone program"""

    def __init__(self, lib):
        self.lib = lib
        self.L = O.lib()
        self.L.orc_ext_align.restype = C.c_int64
        self.n = self.n_cut = self.n_full = 0
        self.records = []

    def run(self, gen, seg, d, g0, jmax, step, strand, before, behind=SLACK, keep=False, tag=None):
        n = len(seg)
        G = len(gen.bytes)
        gmin, gmax = (0, min(G, g0 + jmax)) if d > 0 else (max(0, g0 - jmax), G)
        jm = (gmax - g0) if d > 0 else (g0 - gmin)
        t_ref = C.c_int64(0)
        segb = np.ascontiguousarray(np.concatenate([seg, np.zeros(1, np.uint8)]))
        i_ref = int(self.L.orc_ext_align(segb.ctypes.data_as(O.u8p), C.c_int64(n), d, gen.bytes.ctypes.data_as(O.u8p), C.c_int64(g0),
                                         C.c_int64(gmin), C.c_int64(gmax), C.byref(t_ref)))
        q, p0 = _layout(seg, step, strand, before, behind)
        io, to = C.c_int(-1), C.c_int(-1)
        bad = self.lib.host_ext_all(q.ctypes.data_as(O.u8p), C.c_int64(p0), step, int(strand), n, gen.bases.ctypes.data_as(C.POINTER(C.c_uint32)),
                                    gen.nm.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_int64(g0), d, C.c_int64(jm), C.byref(io), C.byref(to))
        what = (tag, "dir", d, "step", step, "comp", strand, "n", n, "g0", g0, "jmax", jm, "p0", p0)
        assert bad == 0, what + ("way %d differs from ext_align_dev" % (bad - 1),)
        assert (io.value, to.value) == (i_ref, int(t_ref.value)), what + ("got", io.value, to.value, "twin", i_ref, int(t_ref.value))
        self.n += 1
        self.n_cut += 0 < i_ref < n
        self.n_full += i_ref == n
        if keep:
            self.records.append(struct.pack("<12q", p0, step, int(strand), n, g0, d, jm, len(gen.bases), len(gen.nm), len(q), i_ref, int(t_ref.value))
                                + gen.bases.tobytes() + gen.nm.tobytes() + q.tobytes())


@pytest.fixture(scope="module")
def ext_all(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("extrefill"), "extall", _body(), DRIVER)


ORIENT = [(d, step, strand) for d in (+1, -1) for step in (+1, -1) for strand in (False, True)]


def _all_cases(R):
    rng = np.random.default_rng(18)
    G = 2000 + 13                                # (the last genome and mask words are partly used)
    plain = Genome(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=G))
    segs = {}

    def seg_of(gen_key, gen, d, g0, n):
        key = (gen_key, d, g0)
        if key not in segs:
            segs[key] = _diverged(rng, _walk(gen.bytes, g0, d, 300), 300)
        return segs[key][:n].copy()

    # the crossed cases: direction, byte order, strand x query start mod 16 x genome start mod 32 x length
    for d, step, strand in ORIENT:
        for qoff in range(16):
            for gm in G0MOD:
                g0 = 640 + gm
                for n in NS:
                    keep = (qoff in (0, 5, 15)) and gm in (1, 16, 31) and n in (1, 16, 17, 33, 49, 300)
                    R.run(plain, seg_of("plain", plain, d, g0, n), d, g0, G, step, strand, 64 + qoff if step > 0 else 64 + (qoff - n + 1) % 16,
                          keep=keep, tag="crossed")
    # the same with a query that is unrelated behind its first bases: the extension is abandoned (x-drop) in a later chunk
    for d, step, strand in ORIENT:
        for qoff in range(16):
            for hom in (10, 30, 100):
                seg = seg_of("plain", plain, d, 641, 300)
                seg[hom:] = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=300 - hom)
                R.run(plain, seg, d, 641, G, step, strand, 64 + qoff, keep=(qoff in (2, 9)), tag="unrelated tail")
    # a run of N in the genome across a chunk edge (chunks of the genome stream end at base number 16 k + 8)
    for d in (+1, -1):
        for gm in G0MOD:
            g0 = 640 + gm
            gb = plain.bytes.copy()
            for j in (22, 23, 24, 25, 26, 27, 40, 41):          # base numbers, 1-based in walking order
                gb[g0 + j - 1 if d > 0 else g0 - j] = ord("N")
            gen = Genome(gb)
            for step in (+1, -1):
                for strand in (False, True):
                    for n in (47, 300):
                        R.run(gen, seg_of(("nrun", d, gm), gen, d, g0, n), d, g0, G, step, strand, 64 + 3, keep=(gm == 17), tag="N run")
    # a non-ACGT query byte on each side of a chunk edge
    for d, step, strand in ORIENT:
        for pos in (15, 16, 31, 32, 47, 48):
            for n in (49, 300):
                seg = seg_of("plain", plain, d, 641, n)
                seg[pos] = ord("N") if pos % 2 else ord("a")
                R.run(plain, seg, d, 641, G, step, strand, 64 + 7, keep=(n == 49), tag="query N")
    # the contig end inside the extension (jmax < n: the band reaches it and ext_expand takes over) at every offset of a chunk
    for d, step, strand in ORIENT:
        for jmax in list(range(1, 19)) + list(range(40, 57)) + [100, 291, 299]:
            R.run(plain, seg_of("plain", plain, d, 656, 300), d, 656, jmax, step, strand, 64 + 11, keep=(jmax in (1, 8, 9, 24, 25, 41)), tag="contig end")
    # dir = -1 down to genome word 0, dir = +1 up to the last genome word
    for step in (+1, -1):
        for strand in (False, True):
            for g0 in (1, 5, 9, 16, 17, 33, 40, 100):
                R.run(plain, seg_of("plain", plain, -1, g0, min(g0 + 30, 300))[:100], -1, g0, g0, step, strand, 64, keep=True, tag="genome word 0")
            for back in (1, 5, 9, 16, 17, 33, 40, 100):
                g0 = G - back
                R.run(plain, seg_of("plain", plain, +1, g0, 300)[:100], +1, g0, back, step, strand, 64, keep=True, tag="last genome word")
    # step = -1 down to byte 0 of the buffer; step = +1 in the last candidate of a buffer with exactly the slack behind it
    for d in (+1, -1):
        for strand in (False, True):
            for n in NS:
                R.run(plain, seg_of("plain", plain, d, 672, n), d, 672, G, -1, strand, 0, keep=True, tag="byte 0")
                R.run(plain, seg_of("plain", plain, d, 672, n), d, 672, G, +1, strand, 0, keep=True, tag="last candidate")
                R.run(plain, seg_of("plain", plain, d, 672, n), d, 672, G, +1, strand, 5, keep=True, tag="last candidate")


def test_refill_schedules_vs_twin(ext_all, tmp_path):
    """ext_align_dev, ext_step alone and ext_step + ext_refill at every phase == the twin, on every case; then the kept cases through the
    stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer: exit 0, nothing reported"""
    R = Runner(ext_all)
    _all_cases(R)
    assert R.n > 9000 and R.n_cut > 500 and R.n_full > 2000, (R.n, R.n_cut, R.n_full)
    assert len(R.records) > 500
    cpp, exe, data = tmp_path / "ext_main.cpp", tmp_path / "ext_main", tmp_path / "cases.bin"
    cpp.write_text(PRELUDE + _body() + DRIVER + MAIN)
    data.write_bytes(b"".join(R.records))
    # (the sanitizer runtimes linked statically: the program does not depend on what else the process has loaded before it)
    subprocess.run(["g++", "-O1", "-g", "-static-libasan", "-static-libubsan", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", str(exe), str(cpp)], check=True)
    res = subprocess.run([str(exe), str(data)], capture_output=True, text=True)
    assert res.returncode == 0 and not res.stderr.strip(), (res.returncode, res.stderr[-3000:])
    assert res.stdout.strip() == "%d cases" % len(R.records)
