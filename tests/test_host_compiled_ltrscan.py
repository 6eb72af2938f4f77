"""CPU-only: the integer-only parts of the LTR candidate scan (hite_amd/csrc/hite_ltrscan.hip, the blocks between `// >>> ltrscan_key`,
`// >>> ltrscan_filter` and their `// <<<` lines, with the `hsp_cell` and `hsp_key` blocks of hite_hsp.h) compiled for the HOST, as
tests/test_host_compiled_pairhsp.py does for the pair search: the cell inside the host copy of the strip loop (tests/hsp_host.py) and
of the kernel's redo loop against the twin's step 4 on the runs of the small cases, the word and hit keys against the twin's words and
its order of the hits, the filter and the record order against the twin's.  What only the device has -- the sort, the compaction, the
segmented scan, the data-parallel moves, the batches -- is left to tests/test_gpu_ltrscan.py."""
import ctypes as C

import numpy as np
import pytest

import hsp_host as H
import ltrscan_cases as LC
import ltrscan_twin as LT
import pairhsp_twin as PT

WRAPPER = r"""
// the redo loop of ls_extend_kernel on one run of a sequence of len bytes: out = found, ls, le, rs, re, score, matches, columns, alignments
extern "C" void host_extend(const uint8_t *s, int64_t len, int i_lo, int i_hi, int d_lo, int d_hi, int max_ltr, int32_t *out) {
    const int64_t dc = ((int64_t)d_lo + d_hi) >> 1;
    int pl = 0, pr = 0, n_align = 0, found = 0;
    int64_t ls = 0, le = 0, rs = 0, re = 0;
    HspBest h = {0, 0, 0};
    for (;;) {
        const LsWin W = ls_window(len, i_lo, i_hi, dc, pl, pr, max_ltr);
        const int m = (int)(W.qe - W.qb), n = (int)(W.se - W.sb);
        n_align++;
        found = 0;
        if (m < 1 || n < 1 || m >= HITE_PAIRHSP_MAX_LEN || n >= HITE_PAIRHSP_MAX_LEN) break;
        h = host_align(s + W.qb, m, s + W.sb, W.dlo, W.dlo + HSP_BAND - 1, 1, m, 1, n);
        if (hsp_score(h.a) < HITE_PAIRHSP_MIN_SCORE) break;
        found = 1;
        ls = W.qb + hsp_q_start(h.b) - 1; le = W.qb + hsp_q_end(h.e);
        rs = W.sb + hsp_s_start(h.b) - 1; re = W.sb + hsp_s_end(h.e);
        const int step = ls_pad_steps(W, len, ls, le, pl, pr);
        if (step == 0 || n_align > HITE_LTRSCAN_MAX_REDO) break;
        pl += step & 1;
        pr += step >> 1;
    }
    out[0] = found; out[1] = (int32_t)ls; out[2] = (int32_t)le; out[3] = (int32_t)rs; out[4] = (int32_t)re;
    out[5] = hsp_score(h.a); out[6] = hsp_matches(h.a); out[7] = hsp_columns(h.a); out[8] = n_align;
}

extern "C" uint64_t host_word_key(const uint8_t *p) {
    int codes[HITE_LTRSCAN_WORD];
    for (int k = 0; k < HITE_LTRSCAN_WORD; k++) codes[k] = hsp_code(p[k]);
    return hsp_word_key<HITE_LTRSCAN_WORD>(codes);
}
extern "C" uint64_t host_hit_key(uint32_t gp, uint32_t d, int lam, int pos_bits) { return ls_hit_key(gp, d, lam, pos_bits); }
extern "C" int64_t host_key_pos(uint64_t key, int pos_bits) { return ls_key_pos(key, pos_bits); }
extern "C" int64_t host_key_bin(uint64_t key, int pos_bits) { return ls_key_bin(key, pos_bits); }
extern "C" int host_bits(uint64_t v) { return hsp_bits(v); }
extern "C" int host_pad(int k, int max_ltr) { return ls_pad(k, max_ltr); }
extern "C" int host_filter(const int32_t *r, int min_len, int max_len, int min_ltr, int max_ltr, int identity) {
    return ls_filter(r, min_len, max_len, min_ltr, max_ltr, identity);
}
extern "C" int host_rec_less(const int32_t *x, const int32_t *y) { return ls_rec_less(x, y); }
extern "C" int host_rec_same_place(const int32_t *x, const int32_t *y) { return ls_rec_same_place(x, y); }
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    src = H.blocks("hite_hsp.h", "hsp_cell", "hsp_key") + H.blocks("hite_ltrscan.hip", "ltrscan_key", "ltrscan_filter")
    lb = H.compile_host(tmp_path_factory.mktemp("ltrscan_host"), "ls", src + H.HOST_ALIGN + WRAPPER)
    for f in ("host_word_key", "host_hit_key"):
        getattr(lb, f).restype = C.c_uint64
    for f in ("host_key_pos", "host_key_bin"):
        getattr(lb, f).restype = C.c_int64
    return lb


def test_strip_and_redo_loops_vs_twin_on_the_runs_of_the_small_cases(lib):
    n_run = n_redo = n_none = 0
    for c in LC.small_cases():
        kw = c["kw"]
        for s in c["seqs"]:
            s = PT.as_bytes(s)
            hits = LT.links(LT.words(PT.codes(s)), kw["min_ltr"], kw["max_len"] - kw["min_ltr"])
            for lam in LT.LATTICES[:1 if len(s) > 12000 else 2]:
                for run in LT.runs(hits, lam):
                    if run[4] < LT.MIN_HITS or run[1] - run[0] + LT.WORD > kw["max_ltr"]:
                        continue
                    st = dict.fromkeys(LT.STATS, 0)
                    exp = LT.extend(s, run, kw["max_ltr"], PT.align_c, st)
                    out = np.zeros(9, dtype=np.int32)
                    lib.host_extend(s, C.c_int64(len(s)), run[0], run[1], run[2], run[3], kw["max_ltr"], out.ctypes.data_as(C.c_void_p))
                    got = tuple(int(x) for x in out[1:8]) if out[0] else None
                    assert got == exp and out[8] == st["alignments"], (c["label"], run, got, exp)
                    n_run += 1
                    n_redo += st["redos"]
                    n_none += exp is None
    assert n_run >= 80 and n_redo >= 30 and n_none >= 4


def test_word_keys(lib):
    s = b"ACGTTGCAAGCTAnACGTacgtTTGACCAGTNNACGTGTGTGCACACGTTTAGC-ACGATCGATTAGCAGCTAGCTAGCTAGGATC"
    wd = LT.words(PT.codes(s))
    for i in range(len(s) - LT.WORD + 1):
        assert lib.host_word_key(s[i:i + LT.WORD]) == wd.get(i, 1 << 26), i
    assert 10 < len(wd) < len(s) - LT.WORD + 1
    assert lib.host_word_key(b"T" * 13) == (1 << 26) - 1 and lib.host_word_key(b"A" * 12 + b"C") == 1


def test_hit_keys_order_as_the_definition(lib):
    """sorted by the packed key, the hits of a batch of sequences fall into the runs of the definition's order (seq, bin, i)"""
    rng = np.random.default_rng(3)
    off = [0, 5000, 5000, 70000, 2 ** 31 - 5]
    nb = off[-1]
    pb = lib.host_bits(C.c_uint64(nb - 1))
    assert pb == 31 and lib.host_bits(C.c_uint64(0)) == 1 and lib.host_bits(C.c_uint64(255)) == 8 and lib.host_bits(C.c_uint64(256)) == 9
    hits = set()
    for q in range(4):
        for _ in range(300 if off[q + 1] > off[q] else 0):
            i = int(rng.integers(0, min(off[q + 1] - off[q], 3000)))
            hits.add((q, i, int(rng.choice([100, 127, 128, 160, 191, 192, 2 ** 31 - 40]))))
    hits = sorted(hits)
    for lam in LT.LATTICES:
        keyed = sorted((lib.host_hit_key(C.c_uint32(off[q] + i), C.c_uint32(d), lam, pb), q, i, d) for q, i, d in hits)
        for key, q, i, d in keyed:
            assert lib.host_key_pos(C.c_uint64(key), pb) == off[q] + i and lib.host_key_bin(C.c_uint64(key), pb) == (d + lam) >> LT.BIN_SHIFT
        # runs by the packed order: same bin, same sequence, gap <= GAP
        got, cur = [], None
        for key, q, i, d in keyed:
            b = (d + lam) >> LT.BIN_SHIFT
            if cur is not None and cur[0] == (q, b) and i - cur[2] <= LT.GAP:
                cur = [cur[0], cur[1], i, min(cur[3], d), max(cur[4], d), cur[5] + 1]
            else:
                if cur is not None:
                    got.append((cur[0][0],) + tuple(cur[1:]))
                cur = [(q, b), i, i, d, d, 1]
        got.append((cur[0][0],) + tuple(cur[1:]))
        exp = [(q,) + r for q in range(4) for r in LT.runs([(i, d) for qq, i, d in hits if qq == q], lam)]
        assert sorted(got) == sorted(exp) and max(r[5] for r in exp) >= 3


def test_pads(lib):
    for max_ltr in (1, 100, 256, 257, 1024, 5000, 8192):
        assert [lib.host_pad(k, max_ltr) for k in range(4)] == [min(p, max_ltr) for p in LT.PADS] + [max_ltr]


def test_filter_and_order(lib):
    rng = np.random.default_rng(5)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    kw = dict(min_len=400, max_len=1000, min_ltr=100, max_ltr=300, identity=87)
    names = {None: 0, "drop_ltr": 1, "drop_len": 2, "drop_overlap": 3, "drop_identity": 4}
    recs, seen = [], set()
    edge = [(0, 100, 300, 400, 0, 100, 100), (0, 99, 300, 400, 0, 100, 100), (0, 100, 300, 399, 0, 100, 100), (0, 300, 700, 1000, 0, 107, 123),
            (0, 301, 700, 1001, 0, 300, 301), (0, 300, 700, 1001, 0, 107, 123), (0, 200, 200, 400, 0, 87, 100), (0, 201, 200, 400, 0, 87, 100),
            (0, 200, 200, 400, 0, 8699, 10000), (0, 200, 200, 400, 0, 108, 123), (0, 100, 99, 399, 0, 100, 100)]
    for k in range(3000):
        if k < len(edge):
            r = edge[k]
        else:
            ls = int(rng.integers(0, 50))
            le = ls + int(rng.integers(95, 306))
            rs = le + int(rng.integers(-3, 500))
            r = (ls, le, rs, rs + int(rng.integers(95, 306)), int(rng.integers(0, 4)), int(rng.integers(80, 100)), int(rng.integers(95, 110)))
        rec = np.array((int(rng.integers(0, 3)),) + tuple(r), dtype=np.int32)
        why = LT.passes(tuple(int(x) for x in rec[1:]), **kw)
        assert lib.host_filter(p(rec), kw["min_len"], kw["max_len"], kw["min_ltr"], kw["max_ltr"], kw["identity"]) == names[why], rec
        seen.add(why)
        recs.append(tuple(int(x) for x in rec))
    assert seen == set(names)
    recs = recs[:400] + [r[:5] + (r[5] + 1, r[6], r[7]) for r in recs[:40]] + [r[:6] + (r[6] - 1, r[7] + 1) for r in recs[:40]]
    key = lambda r: (r[0], r[1], r[4], r[2], r[3], -r[5], -r[6], r[7])  # noqa: E731
    arr = [np.array(r, dtype=np.int32) for r in recs]
    for x in range(0, len(arr), 7):
        for y in range(len(arr)):
            assert bool(lib.host_rec_less(p(arr[x]), p(arr[y]))) == (key(recs[x]) < key(recs[y]))
            assert bool(lib.host_rec_same_place(p(arr[x]), p(arr[y]))) == (recs[x][:5] == recs[y][:5])
