"""Crafted tables for the full-length copy support (hite_ltr_copy_support_records): what tests/test_host_compiled_ltrcopy.py and
tests/test_gpu_ltrcopy.py both run against tests/ltrcopy_twin.py.  A case: label, el_len, records (per element the list of
(contig, start1, end1, clip)), std ((contig, start, end) per candidate line), contig_len, and the statistics the twin must report
(None: only compared)."""
import numpy as np

FAMILIES = (3000, 5200, 8000)
COUNTS = (0, 1, 63, 64, 65, 300, 0, 2)


def _case(label, el_len, records, std, contig_len, stats=None, **kw):
    return dict(label=label, el_len=list(el_len), records=[list(r) for r in records], std=list(std), contig_len=list(contig_len), stats=stats, kw=kw)


def record_counts(seed=1):
    """elements of 0, 1, 63, 64, 65 and 300 records over three contigs: records on candidate lines (exact, shifted, clipped), records
    beside every line, copies of earlier records (redundant) and nested ones"""
    rng = np.random.default_rng(seed)
    contig_len = [2_000_000, 400_000, 250_001]
    lines = []
    for c, clen in enumerate(contig_len):
        at = 1000
        while at + 9000 < clen:
            ln = int(FAMILIES[(2, 2, 0, 1)[int(rng.integers(0, 4))]] + rng.integers(0, 30))
            s = at + int(rng.integers(0, 500))
            lines.append((c, s, s + ln))
            at += 9000
    std = []
    for k, (c, s, e) in enumerate(lines):
        std.append((c, s, e))
        if k % 7 == 0:        # a line that an earlier one covers by more than 95 %: not stored, and one just below: stored
            std.append((c, s + 20, e + 20))
        if k % 11 == 0:
            std.append((c, s + (e - s) // 10, e + (e - s) // 10))
    el_len, records = [], []
    for n in COUNTS:
        L = FAMILIES[len(el_len) % 3] + 10
        fam = [ln for ln in lines if abs((ln[2] - ln[1]) - L) <= 40]
        recs = []
        for j in range(n):
            kind = int(rng.integers(0, 10))
            if kind < 5 or not recs:
                c, s, e = fam[int(rng.integers(0, len(fam)))]
                d0, d1 = (int(x) for x in rng.integers(-60, 61, size=2)) if kind % 2 else (0, 0)
                recs.append((c, s + 1 + d0, e + d1, int(rng.integers(0, 40)) | int(rng.integers(0, 40)) << 16 if kind == 3 else 0))
            elif kind < 7:
                c = int(rng.integers(0, 3))
                s = int(rng.integers(1, contig_len[c] - L - 1))
                recs.append((c, s, s + L - 1, 0))
            elif kind < 9:
                c, s, e, cl = recs[int(rng.integers(0, len(recs)))]
                d = int(rng.integers(0, 4))
                recs.append((c, s + d, e + int(rng.integers(0, 4)) - d, cl))
            else:
                c, s, e, cl = recs[int(rng.integers(0, len(recs)))]
                cut = int(rng.integers(1, (e - s) // 30 + 2))
                recs.append((c, s + cut, e - cut, cl))
        el_len.append(L)
        records.append(recs)
    return _case("record counts 0 1 63 64 65 300", el_len, records, std, contig_len)


def coverage_bound():
    """L = 2000 at 0.985: clips that sum to 30 leave 1970 / 2000, exactly the bound, 31 fall below; a target of 2030 bases passes
    with the whole element aligned, one of 2031 does not (2000 / 2031 < 0.985)"""
    contig_len = [300_000]
    std = [(0, 10_000 + 20_000 * k, 12_000 + 20_000 * k) for k in range(8)]
    recs = [(0, 10_001, 11_970, 30), (0, 30_001, 31_970, 10 | 20 << 16), (0, 50_001, 51_969, 31), (0, 70_001, 71_969, 16 | 15 << 16),
            (0, 90_001, 92_030, 0), (0, 110_001, 112_031, 0), (0, 130_001, 132_000, 0), (0, 150_001, 151_970, 30 << 16)]
    return _case("coverage at the bound", [2000], [recs], std, contig_len, stats=dict(records=8, covered=5, matched=5, kept=5))


def bucket_edge():
    """a copy and a line that overlap by 99 % and fall into different buckets at 100 000, and the mirror pair that share one"""
    contig_len = [400_000, 400_000]
    std = [(0, 50_000, 149_000), (1, 50_000, 149_000)]
    assert_seg = [(50_000, 149_000, 0), (50_601, 149_800, 1), (50_101, 149_050, 0)]
    recs = [(0, 50_601, 149_800, 0), (1, 50_101, 149_050, 0)]
    c = _case("buckets at a multiple of 100 000", [99_000], [recs], std, contig_len, stats=dict(records=2, covered=2, matched=1, kept=1))
    c["segments"] = assert_seg
    return c


def order_and_nesting():
    """equally long copies (the order of the contigs' first appearance, then input order), nested copies on one contig against the same
    intervals on two contigs, a chain of overlaps, and an overlap of exactly 95 % beside one of a base less"""
    contig_len = [200_000, 200_000, 200_000]
    std = [(c, s, s + ln) for c in range(3) for s, ln in ((10_000, 5000), (30_000, 5000), (50_000, 5100), (70_000, 5000), (90_000, 5000), (90_251, 5000))]
    e0 = [(2, 10_001, 15_000, 0), (0, 30_001, 35_000, 0), (1, 10_001, 15_000, 0), (0, 10_001, 15_000, 0), (2, 30_001, 35_000, 0)]
    # nested on one contig: the shorter goes; the same two intervals on two contigs: both stay
    e1 = [(0, 50_001, 55_100, 0), (0, 50_041, 55_060, 0), (1, 50_001, 55_100, 0), (2, 50_041, 55_060, 0)]
    # a chain a < b < c by length, each 96 % inside the next: a and b go
    e2 = [(1, 70_001, 74_900, 0), (1, 70_001, 75_000, 0), (1, 70_001, 74_950, 0), (1, 70_101, 75_050, 0)]
    # overlap of exactly 95 % of the shorter (4750 of 5000) and one base less
    e3 = [(2, 90_001, 95_000, 0), (2, 90_251, 95_250, 0), (0, 90_001, 95_000, 0), (0, 90_252, 95_251, 0)]
    return _case("order and nesting", [5000, 5100, 4950, 5000], [e0, e1, e2, e3], std, contig_len)


def crafted():
    return [record_counts(), coverage_bound(), bucket_edge(), order_and_nesting()]


def too_many():
    """an element of 301 records: HITE_EINVAL"""
    return _case("301 records", [3000], [[(0, 1001 + k, 4000 + k, 0) for k in range(301)]], [(0, 1000, 4000)], [100_000])
