"""CPU-only: the integer-only parts of the genome annotation (hite_amd/csrc/hite_annotate.hip, the blocks between `// >>> annotate_key`,
`// >>> annotate_resolve` and their `// <<<` lines, with the `hsp_cell` and `hsp_key` blocks of hite_hsp.h) compiled for the HOST, as
tests/test_host_compiled_ltrscan.py does for the LTR scan: the cell inside the host copy of the strip loop (tests/hsp_host.py) and of
the kernel's redo loop against the twin's step 4 on the runs of the small cases, the word code, the packed hit and the sort key
against the twin's words and its order of the hits, the chain walk against the twin's runs, the resolve against the twin's.  What only
the device has -- the sort, the compaction, the look-up, the data-parallel moves, the batches -- is left to tests/test_gpu_annotate.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import annotate_cases as AC
import annotate_twin as AT
import hsp_host as H
import pairhsp_twin as PT

ROOT = H.ROOT

WRAPPER = r"""
// the redo loop of an_extend_kernel on one run: q the text of L bytes, s the sequence of len bytes;
// out = found, gs, ge, qs, qe, score, matches, columns, alignments
extern "C" void host_extend(const uint8_t *q, int64_t L, const uint8_t *s, int64_t len, int g_lo, int g_hi, int d_lo, int d_hi, int32_t *out) {
    const int64_t dc = ((int64_t)d_lo + d_hi) >> 1;
    int pl = 0, pr = 0, n_align = 0, found = 0;
    int64_t qs = 0, qe = 0, gs = 0, ge = 0;
    HspBest h = {0, 0, 0};
    for (;;) {
        const AnWin W = an_window(L, len, g_lo, g_hi, dc, pl, pr);
        const int m = (int)(W.qe - W.qb), n = (int)(W.se - W.sb);
        n_align++;
        found = 0;
        if (m < 1 || n < 1 || m >= HITE_PAIRHSP_MAX_LEN || n >= HITE_PAIRHSP_MAX_LEN) break;
        h = host_align(q + W.qb, m, s + W.sb, W.dlo, W.dlo + HSP_BAND - 1, 1, m, 1, n);
        if (hsp_score(h.a) < HITE_PAIRHSP_MIN_SCORE) break;
        found = 1;
        qs = W.qb + hsp_q_start(h.b) - 1; qe = W.qb + hsp_q_end(h.e);
        gs = W.sb + hsp_s_start(h.b) - 1; ge = W.sb + hsp_s_end(h.e);
        const int step = an_pad_steps(W, L, qs, qe, pl, pr);
        if (step == 0 || n_align > HITE_ANNOT_MAX_REDO) break;
        pl += step & 1;
        pr += step >> 1;
    }
    out[0] = found; out[1] = (int32_t)gs; out[2] = (int32_t)ge; out[3] = (int32_t)qs; out[4] = (int32_t)qe;
    out[5] = hsp_score(h.a); out[6] = hsp_matches(h.a); out[7] = hsp_columns(h.a); out[8] = n_align;
}

extern "C" uint64_t host_word_key(const uint8_t *p) {
    int codes[HITE_ANNOT_WORD];
    for (int k = 0; k < HITE_ANNOT_WORD; k++) codes[k] = hsp_code(p[k]);
    return hsp_word_key<HITE_ANNOT_WORD>(codes);
}
extern "C" void host_revcomp(const uint8_t *p, int64_t n, uint8_t *out) { for (int64_t k = 0; k < n; k++) out[k] = an_comp(p[n - 1 - k]); }
extern "C" uint64_t host_hit_pack(uint32_t t, uint32_t q, uint32_t gp) { return an_hit_pack(t, q, gp); }
extern "C" uint32_t host_hit_t(uint64_t h) { return an_hit_t(h); }
extern "C" uint32_t host_hit_q(uint64_t h) { return an_hit_q(h); }
extern "C" uint32_t host_hit_gp(uint64_t h) { return an_hit_gp(h); }
extern "C" uint32_t host_diag(int64_t g_rel, uint32_t q) { return an_diag(g_rel, q); }
extern "C" uint64_t host_run_key(uint32_t t, uint32_t diag, uint32_t gp, int lam, int bin_bits, int pos_bits) { return an_run_key(t, diag, gp, lam, bin_bits, pos_bits); }
extern "C" int64_t host_key_pos(uint64_t key, int pos_bits) { return an_key_pos(key, pos_bits); }
extern "C" uint64_t host_key_group(uint64_t key, int pos_bits) { return an_key_group(key, pos_bits); }
extern "C" int host_bits(uint64_t v) { return hsp_bits(v); }
extern "C" int host_pad(int k) { return an_pad(k); }

// the walk of an_run_kernel over n hits of one (piece, t, bin) in ascending g: out gets (g_first, g_last, d_lo, d_hi, hits) per run
extern "C" int64_t host_chains(int64_t n, const int64_t *g, const uint32_t *diag, int64_t *out) {
    int64_t runs = 0;
    AnChain c;
    auto emit = [&]() {
        if (c.n < HITE_ANNOT_MIN_HITS) return;
        int64_t *o = out + 5 * runs++;
        o[0] = c.g_first; o[1] = c.g_last; o[2] = c.d_lo; o[3] = c.d_hi; o[4] = c.n;
    };
    for (int64_t k = 0; k < n; k++) {
        if (k == 0) an_chain_start(c, g[k], diag[k]);
        else if (an_chain_breaks(c, g[k])) { emit(); an_chain_start(c, g[k], diag[k]); }
        else an_chain_add(c, g[k], diag[k]);
    }
    if (n > 0) emit();
    return runs;
}

// steps 5 and 6 as the entry point runs them: recs (n x 10) in any order -> the kept ones in recs; returns their number
extern "C" int64_t host_resolve(int64_t n, int32_t *recs, int64_t *dup, int64_t *dom) {
    std::vector<AnRec> v((size_t)n);
    if (n) memcpy(v.data(), recs, (size_t)n * sizeof(AnRec));
    std::sort(v.begin(), v.end(), [](const AnRec &x, const AnRec &y) { return an_rec_less(x.f, y.f); });
    an_resolve(v, dup, dom);
    if (!v.empty()) memcpy(recs, v.data(), v.size() * sizeof(AnRec));
    return (int64_t)v.size();
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    src = H.blocks("hite_hsp.h", "hsp_cell", "hsp_key") + H.blocks("hite_annotate.hip", "annotate_key", "annotate_resolve")
    lb = H.compile_host(tmp_path_factory.mktemp("annotate_host"), "an", src + H.HOST_ALIGN + WRAPPER)
    for f in ("host_word_key", "host_hit_pack", "host_run_key", "host_key_group"):
        getattr(lb, f).restype = C.c_uint64
    for f in ("host_key_pos", "host_chains", "host_resolve"):
        getattr(lb, f).restype = C.c_int64
    for f in ("host_hit_t", "host_hit_q", "host_hit_gp", "host_diag"):
        getattr(lb, f).restype = C.c_uint32
    return lb


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_header_constants_are_the_twin_s():
    txt = open(os.path.join(ROOT, "include", "hite_gpu.h")).read()
    val = lambda name: eval(re.search(r"#define HITE_ANNOT_%s\s+(.+)" % name, txt).group(1))  # noqa: E731
    assert [val(n) for n in ("WORD", "MAX_OCC", "BIN_SHIFT", "GAP", "MIN_HITS", "MAX_SPAN", "EDGE", "MAX_REDO", "PIECE", "MIN_PIECE", "OVERLAP",
                             "MAX_LIB_LEN", "MAX_LIB")] == \
        [AT.WORD, AT.MAX_OCC, AT.BIN_SHIFT, AT.GAP, AT.MIN_HITS, AT.MAX_SPAN, AT.EDGE, AT.MAX_REDO, AT.PIECE, AT.MIN_PIECE, AT.OVERLAP, AT.MAX_LIB_LEN,
         AT.MAX_LIB]
    assert (0, val("LATTICE")) == AT.LATTICES and (val("BAND_BELOW"), val("BAND_ABOVE")) == (AT.BAND_BELOW, AT.BAND_ABOVE)
    assert tuple(val("PAD_%d" % k) for k in range(4)) == AT.PADS and val("STATS") == len(AT.STATS) and val("REC") == 10
    # a window stays under what the packed start coordinates hold
    assert AT.MAX_SPAN + AT.WORD + 2 * AT.PADS[-1] + AT.BAND_BELOW + AT.BAND_ABOVE < PT.MAX_LEN


def test_strip_and_redo_loops_vs_twin_on_the_runs_of_the_small_cases(lib):
    n_run = n_redo = n_none = n_minus = 0
    for c in AC.small_cases():
        st = dict.fromkeys(AT.STATS, 0)
        texts, tab = AT.table(c["lib"], st)
        for s in c["seqs"]:
            s = PT.as_bytes(s)
            if len(s) > 16000:
                continue
            codes = PT.codes(s)
            for begin, end in AT.pieces(len(s), c["piece_len"]):
                hits = AT.hits_of(codes, begin, end, tab)
                for lam in AT.LATTICES:
                    for run in AT.runs(hits, begin, lam):
                        if run[5] < AT.MIN_HITS:
                            continue
                        st = dict.fromkeys(AT.STATS, 0)
                        exp = AT.extend(s, texts[run[0]], run, PT.align_c, st)
                        tb = bytes(b"ACGTN"[x] for x in texts[run[0]])
                        out = np.zeros(9, dtype=np.int32)
                        lib.host_extend(tb, C.c_int64(len(tb)), s, C.c_int64(len(s)), run[1], run[2], run[3], run[4], _p(out))
                        got = tuple(int(x) for x in out[1:8]) if out[0] else None
                        assert got == exp and out[8] == st["alignments"], (c["label"], run, got, exp)
                        n_run += 1
                        n_redo += st["redos"]
                        n_none += exp is None
                        n_minus += run[0] & 1
    assert n_run >= 60 and n_redo >= 12 and n_none >= 6 and n_minus >= 8


def test_word_keys_and_the_reverse_complement(lib):
    s = b"ACGTTGCAAGCTAnACGTacgtTTGACCAGTNNACGTGTGTGCACACGTTTAGC-ACGATCGATTAGCAGCTAGCTAGCTAGGATC"
    wd = AT.words(PT.codes(s))
    for i in range(len(s) - AT.WORD + 1):
        assert lib.host_word_key(s[i:i + AT.WORD]) == wd.get(i, 1 << 26), i
    assert 10 < len(wd) < len(s) - AT.WORD + 1
    assert lib.host_word_key(b"T" * 13) == (1 << 26) - 1 and lib.host_word_key(b"A" * 12 + b"C") == 1
    out = C.create_string_buffer(len(s))
    lib.host_revcomp(s, C.c_int64(len(s)), out)
    assert PT.codes(out.raw) == AT.revcomp_codes(PT.codes(s))


def test_packed_hits_and_sort_keys_order_as_the_definition(lib):
    rng = np.random.default_rng(3)
    for t, q, gp in [(0, 0, 0), (65535, AT.MAX_LIB_LEN - 13, (1 << 26) - 1), (1, 24563, 5), (40000, 7, 1 << 25)]:
        h = lib.host_hit_pack(C.c_uint32(t), C.c_uint32(q), C.c_uint32(gp))
        assert (lib.host_hit_t(C.c_uint64(h)), lib.host_hit_q(C.c_uint64(h)), lib.host_hit_gp(C.c_uint64(h))) == (t, q, gp)
    assert lib.host_bits(C.c_uint64(0)) == 1 and lib.host_bits(C.c_uint64(255)) == 8 and lib.host_bits(C.c_uint64(256)) == 9
    assert lib.host_bits(C.c_uint64((1 << 26) - 1)) == 26 and [lib.host_pad(k) for k in range(4)] == list(AT.PADS)
    # two pieces in one batch: piece 0 = bases [0, 5000) of its sequence at 0, piece 1 = bases [4096, 9000) with a lead of 100 at 5000
    pieces = [(0, 0, 0, 5000), (4096, 5000, 100, 4904)]         # (begin, at, lead, bases)
    nb = 5000 + 100 + 4904
    pos_bits, bin_bits = lib.host_bits(C.c_uint64(nb - 1)), lib.host_bits(C.c_uint64((5000 + AT.MAX_LIB_LEN + 32) >> 6))
    hits = set()
    for p, (begin, at, lead, n) in enumerate(pieces):
        for _ in range(400):
            q = int(rng.choice([0, 1, 63, 64, 100, 1000, AT.MAX_LIB_LEN - 13]))
            hits.add((p, int(rng.integers(0, 3)), q, begin + int(rng.integers(0, min(n, 2500)))))
    hits = sorted(hits)
    for lam in AT.LATTICES:
        keyed = []
        for p, t, q, g in hits:
            begin, at, lead, _n = pieces[p]
            gp = at + lead + g - begin
            diag = lib.host_diag(C.c_int64(g - begin), C.c_uint32(q))
            assert diag == g - q - begin + AT.MAX_LIB_LEN
            key = lib.host_run_key(C.c_uint32(t), C.c_uint32(diag), C.c_uint32(gp), lam, bin_bits, pos_bits)
            assert lib.host_key_pos(C.c_uint64(key), pos_bits) == gp
            assert lib.host_key_group(C.c_uint64(key), pos_bits) == t << bin_bits | (g - q - begin + lam + AT.MAX_LIB_LEN) >> 6
            keyed.append((key, p, t, g, g - q, diag))
        keyed.sort()
        # by the packed order, the groups of equal (key group, piece) are the twin's (piece, t, bin) in ascending g; the walk gives its runs
        got, exp = [], []
        k = 0
        while k < len(keyed):
            e = k
            grp = lib.host_key_group(C.c_uint64(keyed[k][0]), pos_bits)
            while e < len(keyed) and lib.host_key_group(C.c_uint64(keyed[e][0]), pos_bits) == grp and keyed[e][1] == keyed[k][1]:
                e += 1
            p, t = keyed[k][1], keyed[k][2]
            g = np.array([x[3] for x in keyed[k:e]], dtype=np.int64)
            assert (np.diff(g) >= 0).all()
            diag = np.array([x[5] for x in keyed[k:e]], dtype=np.uint32)
            out = np.zeros((e - k, 5), dtype=np.int64)
            n = lib.host_chains(C.c_int64(e - k), _p(g), _p(diag), _p(out))
            to_d = pieces[p][0] - AT.MAX_LIB_LEN
            got += [(p, t, int(o[0]), int(o[1]), int(o[2]) + to_d, int(o[3]) + to_d, int(o[4])) for o in out[:n]]
            k = e
        for p in range(2):
            exp += [(p,) + r for r in AT.runs([(t, g, d) for _k, pp, t, g, d, _dg in keyed if pp == p], pieces[p][0], lam) if r[5] >= AT.MIN_HITS]
        assert sorted(got) == sorted(exp) and len(exp) >= 5


def test_chains_close_at_the_gap_and_at_the_span(lib):
    def chains(g):
        g = np.array(g, dtype=np.int64)
        diag = np.arange(len(g), dtype=np.uint32) % 7 + 100
        out = np.zeros((len(g) + 1, 5), dtype=np.int64)
        n = lib.host_chains(C.c_int64(len(g)), _p(g), _p(diag), _p(out))
        exp = [r[1:] for r in AT.runs([(0, int(x), int(x) - int(d)) for x, d in zip(g, 30000 - diag.astype(np.int64))], 0, 0)]
        return [tuple(int(x) for x in o) for o in out[:n]], exp

    got, _ = chains([0, 300, 600, 901, 902, 903])
    assert [(r[0], r[1], r[4]) for r in got] == [(0, 600, 3), (901, 903, 3)]
    got, _ = chains(list(range(0, 8400, 200)))
    assert [(r[0], r[1], r[4]) for r in got] == [(0, 8000, 41)]                   # 8 200 - 0 >= MAX_SPAN: the 42nd hit starts a chain of one
    got, _ = chains(list(range(0, 17000, 100)))
    assert [(r[0], r[1]) for r in got] == [(0, 8100), (8200, 16300), (16400, 16900)]
    assert chains([5, 5, 5])[0] == [(5, 5, 100, 102, 3)] and chains([5, 5])[0] == [] and chains([])[0] == []


def test_resolve_vs_twin(lib):
    rng = np.random.default_rng(5)
    for trial in range(30):
        n = int(rng.integers(0, 120))
        recs = []
        for _ in range(n):
            gs = int(rng.integers(0, 3000))
            ln = int(rng.choice([50, 100, 500, 1000, 30000]))
            recs.append((int(rng.integers(0, 2)), gs, gs + ln, int(rng.integers(0, 3)), int(rng.integers(0, 2)), 0, ln, int(rng.choice([100, 200, 200, 900])),
                         ln // 2, ln))
        recs += recs[:n // 4]                                                        # duplicates
        recs += [r[:7] + (r[7] + 1, r[8], r[9]) for r in recs[:n // 8]]                # the same place at another score
        order = rng.permutation(len(recs))
        arr = np.array([recs[k] for k in order], dtype=np.int32).reshape(-1, 10)
        dup, dom = C.c_int64(0), C.c_int64(0)
        m = lib.host_resolve(C.c_int64(len(arr)), _p(arr), C.byref(dup), C.byref(dom))
        st = dict.fromkeys(AT.STATS, 0)
        exp = AT.resolve(list(recs), st)
        assert [tuple(r) for r in arr[:m].tolist()] == exp and (dup.value, dom.value) == (st["duplicates"], st["dominated"]), trial
    for x, y in [((0, 0, 1000), (0, 200, 1200)), ((0, 0, 500), (0, 100, 5000)), ((0, 0, 500), (0, 101, 5000)), ((0, 0, 500), (1, 0, 500))]:
        a, b = x + (0, 0, 0, 10, 100, 50, 50), y + (1, 0, 0, 10, 200, 50, 50)
        arr = np.array([a, b], dtype=np.int32)
        dup, dom = C.c_int64(0), C.c_int64(0)
        m = lib.host_resolve(C.c_int64(2), _p(arr), C.byref(dup), C.byref(dom))
        assert [tuple(r) for r in arr[:m].tolist()] == AT.resolve([a, b], dict.fromkeys(AT.STATS, 0))
    assert dom.value == 0      # (the last pair: other sequences)
