"""CPU twin of the full-length copy support (include/hite_gpu.h, hite_amd/csrc/hite_ltrcopy.hip): FiLTR's get_copies_minimap2
(bin/FiLTR-main/src/Util.py:6509-6556) and get_intact_ltr_copies (:11022-11147) on a copy table, written plainly with Python's own
integers and floats, independent of hite_amd.  A zero denominator, where the reference raises ZeroDivisionError, answers False."""
SEGMENT_LEN = 100000
STATS = ("records", "covered", "matched", "kept")


def map_fragment(start, end, chunk_size):
    start_chunk, end_chunk = start // chunk_size, end // chunk_size
    if start_chunk == end_chunk:
        return start_chunk
    if abs(end_chunk * chunk_size - start) < abs(end - end_chunk * chunk_size):
        return end_chunk
    return start_chunk


def cover_ok(L, clip, start1, end1, c):
    aligned = L - (clip & 0xffff) - (clip >> 16)
    target = end1 - start1 + 1
    if L <= 0 or target <= 0:
        return False
    return aligned / L >= c and aligned / target >= c


def overlap_ok(prev, cur, thr):
    ov = max(min(prev[1], cur[1]) - max(prev[0], cur[0]), 0)
    dp, dc = abs(prev[1] - prev[0]), abs(cur[1] - cur[0])
    if dp == 0 or dc == 0:
        return False
    return ov / dp >= thr and ov / dc >= thr


def buckets(std, contig_len, thr, segment_len=SEGMENT_LEN):
    """std: (contig, start, end) per candidate line, in the order of ltr_lines -> {(contig, segment): [(start, end), ...]}"""
    out = {}
    for c, s, e in std:
        seg = map_fragment(s, e, segment_len)
        if seg >= contig_len[c] // segment_len + (contig_len[c] % segment_len != 0):
            continue
        frs = out.setdefault((c, seg), [])
        if not any(overlap_ok(p, (s, e), thr) for p in frs):
            frs.append((s, e))
    return out


def redundancy(copies):
    """copies: (contig, start, end) in the order the reference holds them -> the kept ones, ascending by end - start"""
    copies = sorted(copies, key=lambda x: x[2] - x[1])
    out = []
    for i, (ci, si, ei) in enumerate(copies):
        if not any(cj == ci and min(ei, ej) - max(si, sj) + 1 >= 0.95 * (ei - si + 1) for cj, sj, ej in copies[i + 1:]):
            out.append((ci, si, ei))
    return out


def support_records(el_len, records, std, contig_len, full_length_coverage=0.985, overlap_threshold=0.95, segment_len=SEGMENT_LEN, stats=None):
    """el_len[k]: bases of element k; records[k]: its (contig, start1, end1, clip) in input order; std as buckets() takes it ->
    per element the list of (contig, start1, end1) kept.  stats: a dict that receives STATS."""
    table = buckets(std, contig_len, overlap_threshold, segment_len)
    st = dict.fromkeys(STATS, 0)
    covered = []
    for L, recs in zip(el_len, records):
        if len(recs) > 300:
            raise ValueError("an element of more than 300 records")
        st["records"] += len(recs)
        covered.append([r[:3] for r in recs if cover_ok(L, r[3], r[1], r[2], full_length_coverage)])
    # the reference collects the full-length records contig by contig, the contigs in the order of their first record (:11039-11049)
    order = {}
    for recs in covered:
        for c, _, _ in recs:
            order.setdefault(c, len(order))
    out = []
    for recs in covered:
        st["covered"] += len(recs)
        hit = [r for r in recs
               if any(overlap_ok(p, (r[1], r[2]), overlap_threshold) for p in table.get((r[0], map_fragment(r[1], r[2], segment_len)), ()))]
        st["matched"] += len(hit)
        hit.sort(key=lambda r: order[r[0]])
        out.append(redundancy(hit))
        st["kept"] += len(out[-1])
    if stats is not None:
        stats.update(st)
    return out


def support(contigs, elements, std, full_length_coverage=0.985, overlap_threshold=0.95, segment_len=SEGMENT_LEN, stats=None):
    """the copy finder's twin on the elements (aligned intervals, clip words), then support_records"""
    import oracle_lib as O

    tab = O.find_copies(contigs, elements, clips=True)
    records = [[(r[0], r[1], r[2], r[5]) for r in rows] for rows in tab]
    return support_records([len(e) for e in elements], records, std, [len(c) for c in contigs], full_length_coverage, overlap_threshold,
                           segment_len, stats)
