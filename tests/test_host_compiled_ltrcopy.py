"""CPU-only: the rules of the full-length copy support (hite_amd/csrc/hite_ltrcopy.h, what the kernels of hite_ltrcopy.hip run per
record and per element) compiled for the HOST and held against tests/ltrcopy_twin.py: the crafted tables of tests/ltrcopy_cases.py
through a serial driver made of the same routines, and every binary64 compare on the full sweep of (overlap, length) for lengths 1
to 400 at both thresholds -- every place where the device's division or multiplication could round differently from Python's.  What
only the device has -- the compaction, the atomics, the rank and the redundancy rule spread over a wavefront -- is left to
tests/test_gpu_ltrcopy.py."""
import ctypes as C
import os

import numpy as np
import pytest

import hsp_host as H
import ltrcopy_cases as LC
import ltrcopy_twin as LT

WRAPPER = r"""
extern "C" int64_t host_map_fragment(int64_t s, int64_t e, int64_t chunk) { return lc_map_fragment(s, e, chunk); }
extern "C" int host_cover_ok(int64_t L, uint32_t clip, int64_t s, int64_t e, double c) { return lc_cover_ok(L, clip, s, e, c); }
extern "C" int host_overlap_ok(int64_t ps, int64_t pe, int64_t s, int64_t e, double thr) { return lc_overlap_ok(ps, pe, s, e, thr); }
extern "C" int host_redundant(int i, int m, const int64_t *s, const int64_t *e, const int32_t *c) { return lc_redundant(i, m, s, e, c); }

// the two kernels of hite_ltrcopy.hip, record after record and element after element; -1: bad input, else the number of copies kept
extern "C" int64_t host_support_records(int64_t n_el, const int64_t *el_len, const int32_t *copy_first, const int32_t *contig,
                                        const int64_t *start1, const int64_t *end1, const uint32_t *clip, int64_t n_std,
                                        const int32_t *std_contig, const int64_t *std_start, const int64_t *std_end, int32_t n_contig,
                                        const int64_t *contig_len, double cover, double thr, int64_t segment_len, int32_t *out_first,
                                        int32_t *out_contig, int64_t *out_start1, int64_t *out_end1, int64_t *stats, int64_t *n_stored) {
    LcBuckets B;
    if (!lc_build_buckets(n_std, std_contig, std_start, std_end, n_contig, contig_len, thr, segment_len, &B)) return -1;
    *n_stored = (int64_t)B.fs.size();
    const int64_t n_rec = copy_first[n_el];
    std::vector<uint8_t> hit((size_t)n_rec, 0);
    std::vector<uint32_t> first((size_t)n_contig, 0xffffffffu);
    stats[0] = n_rec; stats[1] = stats[2] = stats[3] = 0;
    for (int64_t el = 0; el < n_el; el++)
        for (int64_t r = copy_first[el]; r < copy_first[el + 1]; r++) {
            if (contig[r] < 0 || contig[r] >= n_contig) return -1;
            if (!lc_cover_ok(el_len[el], clip[r], start1[r], end1[r], cover)) continue;
            stats[1]++;
            first[contig[r]] = std::min(first[contig[r]], (uint32_t)r);
            hit[r] = lc_match(B.keys.data(), B.first.data(), (int64_t)B.keys.size(), B.fs.data(), B.fe.data(), contig[r], start1[r], end1[r], thr, segment_len);
            stats[2] += hit[r];
        }
    int64_t at = 0;
    for (int64_t el = 0; el < n_el; el++) {
        out_first[el] = (int32_t)at;
        std::vector<int64_t> s, e, ts, te;
        std::vector<int32_t> c, tc;
        std::vector<uint32_t> cf;
        for (int64_t r = copy_first[el]; r < copy_first[el + 1]; r++)
            if (hit[r]) { s.push_back(start1[r]); e.push_back(end1[r]); c.push_back(contig[r]); cf.push_back(first[contig[r]]); }
        const int m = (int)s.size();
        if (m > LC_MAX_RECORDS) return -1;
        ts.resize(m); te.resize(m); tc.resize(m);
        for (int i = 0; i < m; i++) {
            const int rk = lc_rank(i, m, s.data(), e.data(), cf.data());
            ts[rk] = s[i]; te[rk] = e[i]; tc[rk] = c[i];
        }
        for (int i = 0; i < m; i++)
            if (!lc_redundant(i, m, ts.data(), te.data(), tc.data())) { out_contig[at] = tc[i]; out_start1[at] = ts[i]; out_end1[at] = te[i]; at++; }
    }
    out_first[n_el] = (int32_t)at;
    stats[3] = at;
    return at;
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    inc = '#include "%s"\n' % os.path.join(H.ROOT, "hite_amd", "csrc", "hite_ltrcopy.h")
    lb = H.compile_host(tmp_path_factory.mktemp("ltrcopy_host"), "lc", inc + WRAPPER)
    lb.host_map_fragment.restype = C.c_int64
    lb.host_support_records.restype = C.c_int64
    return lb


def run_host(lib, c):
    a = lambda x, t: np.ascontiguousarray(x, dtype=t)  # noqa: E731
    p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    n = len(c["el_len"])
    cf = np.zeros(n + 1, dtype=np.int32)
    np.cumsum([len(r) for r in c["records"]], out=cf[1:])
    flat = [t for r in c["records"] for t in r]
    ct, s1, e1, cl = (a([t[k] for t in flat], t_) for k, t_ in ((0, np.int32), (1, np.int64), (2, np.int64), (3, np.uint32)))
    sc, ss, se = (a([t[k] for t in c["std"]], t_) for k, t_ in ((0, np.int32), (1, np.int64), (2, np.int64)))
    clen = a(c["contig_len"], np.int64)
    kw = dict(dict(full_length_coverage=0.985, overlap_threshold=0.95, segment_len=LT.SEGMENT_LEN), **c["kw"])
    of = np.zeros(n + 1, dtype=np.int32)
    oc, os_, oe = np.zeros(len(flat) + 1, dtype=np.int32), np.zeros(len(flat) + 1, dtype=np.int64), np.zeros(len(flat) + 1, dtype=np.int64)
    st, stored = np.zeros(4, dtype=np.int64), C.c_int64(0)
    rc = lib.host_support_records(C.c_int64(n), p(a(c["el_len"], np.int64)), p(cf), p(ct), p(s1), p(e1), p(cl), C.c_int64(len(sc)), p(sc), p(ss), p(se),
                                  C.c_int32(len(clen)), p(clen), C.c_double(kw["full_length_coverage"]), C.c_double(kw["overlap_threshold"]),
                                  C.c_int64(kw["segment_len"]), p(of), p(oc), p(os_), p(oe), p(st), C.byref(stored))
    if rc < 0:
        return None, None, None
    rows = list(zip(oc.tolist(), os_.tolist(), oe.tolist()))
    return [rows[of[k]:of[k + 1]] for k in range(n)], dict(zip(LT.STATS, (int(x) for x in st))), stored.value


@pytest.mark.parametrize("case", LC.crafted(), ids=lambda c: c["label"])
def test_crafted_tables_vs_twin(lib, case):
    st = {}
    exp = LT.support_records(case["el_len"], case["records"], case["std"], case["contig_len"], stats=st, **case["kw"])
    got, gst, stored = run_host(lib, case)
    assert got == exp and gst == st
    assert case["stats"] is None or st == case["stats"]
    assert stored == sum(len(v) for v in LT.buckets(case["std"], case["contig_len"], 0.95).values())
    for s, e, seg in case.get("segments", ()):
        assert lib.host_map_fragment(C.c_int64(s), C.c_int64(e), C.c_int64(LT.SEGMENT_LEN)) == seg == LT.map_fragment(s, e, LT.SEGMENT_LEN)


def test_the_crafted_tables_reach_every_rule():
    st = {}
    c = LC.record_counts()
    out = LT.support_records(c["el_len"], c["records"], c["std"], c["contig_len"], stats=st)
    assert [len(r) for r in c["records"]] == list(LC.COUNTS)
    assert st["records"] > st["covered"] > st["matched"] > st["kept"] > 0 and max(len(o) for o in out) > 64 and all(0 < len(o) < 64 for o in out[2:5])
    stored = sum(len(v) for v in LT.buckets(c["std"], c["contig_len"], 0.95).values())
    assert len(c["std"]) > stored > len(c["std"]) - len(c["std"]) // 7 - 2          # the covered lines are left out, the others are not
    c = LC.order_and_nesting()
    out = LT.support_records(c["el_len"], c["records"], c["std"], c["contig_len"])
    assert [r[0] for r in out[0]] == [2, 2, 0, 0, 1] and [len(o) for o in out] == [5, 3, 1, 3]
    assert out[3] == [(2, 90_251, 95_250), (0, 90_001, 95_000), (0, 90_252, 95_251)]


def test_301_records_are_refused_by_the_twin():
    c = LC.too_many()
    with pytest.raises(ValueError):
        LT.support_records(c["el_len"], c["records"], c["std"], c["contig_len"])


def test_map_fragment(lib):
    rng = np.random.default_rng(2)
    for chunk in (1, 7, 1000, 100000):
        for _ in range(2000):
            s = int(rng.integers(0, 5 * chunk + 3))
            e = s + int(rng.integers(0, 3 * chunk + 2))
            assert lib.host_map_fragment(C.c_int64(s), C.c_int64(e), C.c_int64(chunk)) == LT.map_fragment(s, e, chunk)
    for s, e in ((99_999, 100_000), (100_000, 100_000), (50_000, 150_000), (50_001, 150_000), (49_999, 150_000), (0, 299_999), (2 ** 32 - 5, 2 ** 32 + 9)):
        assert lib.host_map_fragment(C.c_int64(s), C.c_int64(e), C.c_int64(100000)) == LT.map_fragment(s, e, 100000)


def test_every_binary64_compare_on_the_full_sweep(lib):
    """overlap 0 .. length for lengths 1 .. 400: the quotient against 0.95 and 0.985 in the coverage rule and in the two-sided test,
    the product 0.95 * length in the redundancy rule"""
    n_true = n_edge = 0
    for ln in range(1, 401):
        s = np.array([1, 0], dtype=np.int64)
        e = np.array([ln, 0], dtype=np.int64)
        ct = np.zeros(2, dtype=np.int32)
        for ov in range(0, ln + 1):
            for thr in (0.95, 0.985):
                exp = ov / ln >= thr
                # the coverage rule: once the element, once the target decides
                assert bool(lib.host_cover_ok(C.c_int64(ln), C.c_uint32(ln - ov), C.c_int64(1), C.c_int64(ov), C.c_double(thr))) == (exp and ov > 0)
                assert bool(lib.host_cover_ok(C.c_int64(ov), C.c_uint32(0), C.c_int64(1), C.c_int64(ln), C.c_double(thr))) == (exp and ov > 0)
                assert LT.cover_ok(ln, ln - ov, 1, ov, thr) == (exp and ov > 0) and LT.cover_ok(ov, 0, 1, ln, thr) == (exp and ov > 0)
                # the two-sided test: both fragments ln long, ov in common; then the stored one longer, so that the other decides
                assert bool(lib.host_overlap_ok(C.c_int64(0), C.c_int64(ln), C.c_int64(ln - ov), C.c_int64(2 * ln - ov), C.c_double(thr))) == exp
                assert bool(lib.host_overlap_ok(C.c_int64(ln - ov), C.c_int64(2 * ln - ov), C.c_int64(0), C.c_int64(ln), C.c_double(thr))) == exp
                assert LT.overlap_ok((0, ln), (ln - ov, 2 * ln - ov), thr) == exp
                n_true += exp
                n_edge += ov / ln == thr
            # the redundancy rule: copy 0 of ln bases, copy 1 later in the order (longer) with ov bases in common
            s[1], e[1] = ln - ov + 1, 2 * ln + 1
            exp = ov >= 0.95 * ln
            assert bool(lib.host_redundant(0, 2, s.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p), ct.ctypes.data_as(C.c_void_p))) == exp
            assert (LT.redundancy([(0, 1, ln), (0, ln - ov + 1, 2 * ln + 1)]) == [(0, ln - ov + 1, 2 * ln + 1)]) == exp
    assert n_true > 5000 and n_edge >= 20          # 19 / 20, 38 / 40, 197 / 200, ... sit exactly on a bound
