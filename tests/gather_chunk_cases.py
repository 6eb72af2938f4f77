"""Copy tables for tests/test_gpu_gather_chunks.py: the window gather in chunks of the destination (hite_amd/csrc/hite_pipeline.hip:
row_meta_kernel's row descriptors, gather_items_kernel, row_gather_chunks_kernel; hite_genome.h: the gather_chunk block) at the edges
of its items (runs of 256 chunks of 16 bytes) and chunks, on the genome and with the helpers of tests/fine_row_cases.py.  The expectation
is the twin (tests/oracle_pipeline.py: pass_rows), computed once per case and pass."""
import fine_row_cases as FR

ITEM_BYTES = 4096                      # GR_ITEM_CHUNKS chunks of 16 bytes
EDGE_LENS = (100, 111, 112, 113, 1000, 1001, 1016, 4080, 4095, 4096, 4097, 8191, 8192, 8193, 12300)
SEAM_PADS = (0, 1, 3, 4, 12, 499, 500, 501)

_cases = None
_twin = {}


def items_of(n):
    return (((n + 15) // 16) + 255) // 256


def cases():
    global _cases
    if _cases is None:
        out = []
        clen = FR.clen
        # item and chunk edges: rows of exactly 1, 2, 3 and 4 items; the short lengths also in a candidate of their own (full in pass A)
        for m in (0, 1):
            rows = [FR.win(0, 150 + 13 * j, n, m) for j, n in enumerate(EDGE_LENS)]
            out.append({"name": "item_edges_%s" % "+-"[m], "copies": [rows, [r for r, n in zip(rows, EDGE_LENS) if n <= 1000]]})
        # the seam of the first500 + last500 form in chunk 31, pads on both sides of it, all four strand combinations
        ab = [(a, 0) for a in SEAM_PADS] + [(0, b) for b in SEAM_PADS[1:]] + [(a, a) for a in (1, 499, 500, 501)] +[(499, 501), (501, 499), (4, 12)]
        for m0 in (0, 1):
            rows = [FR.padcopy(0, 2000 + 1100 * (j % 30), n, j & 1, a, b) for j, (a, b, n) in
                    enumerate((a, b, n) for (a, b) in ab for n in (1001, 1016) for _m in (0, 1))]
            out.append({"name": "seam_%s" % "+-"[m0], "copies": [[FR.win(2, 9000, 1100, m0)] + rows]})
        # the item search: rows of 1 and of 4 items in turn; candidates of 0, 1, 5 and 100 rows; an empty last candidate
        alt = [FR.win(0, 200 + 251 * j, 12300 if j & 1 else 100, (j >> 1) & 1) for j in range(100)]
        out.append({"name": "item_search", "copies": [[], alt[1:2], alt[:5], alt, []]})
        # genome position 0, the last base of the last contig, the first base of a later contig: one item and several
        ends = []
        for n in (100, 1001, 4097):
            ends.append([FR.win(0, 0, n, m) for m in (0, 1)] + [FR.win(3, clen(3) - n, n, m) for m in (0, 1)] +
                        [FR.win(ci, 0, n, m) for ci in (1, 2, 3) for m in (0, 1)])
        out.append({"name": "contig_ends_items", "copies": ends})
        for c in out:
            c["cands"] = [FR.DUMMY] * len(c["copies"])
        _cases = out
    return _cases


def names():
    return [c["name"] for c in cases()]


def case(name):
    return [c for c in cases() if c["name"] == name][0]


def twin(name, p):
    """(rows, totals) of pass p by the twin, computed once"""
    if (name, p) not in _twin:
        c = case(name)
        _twin[(name, p)] = FR.twin_rows(FR.genome()["contigs"], FR.NAMES, c["cands"], c["copies"], FR.FLANK, p)
    return _twin[(name, p)]


def selfcheck():
    """by the twin alone: every case reaches what it is named for"""
    for m in "+-":
        b = twin("item_edges_" + m, 1)[0]
        assert tuple(len(x[1]) for x in b[0]) == EDGE_LENS and b[1] == []
        assert {items_of(len(x[1])) for x in b[0]} == {1, 2, 3, 4} and items_of(4096) == 1 and items_of(4097) == 2 and items_of(12300) == 4
        a = twin("item_edges_" + m, 0)[0]
        assert all(x[2] and len(x[1]) == 1000 for x in a[0]) and tuple(len(x[1]) for x in a[1]) == EDGE_LENS[:5]
        s = twin("seam_" + m, 0)[0][0]
        assert len(s) == len(case("seam_" + m)["copies"][0]) and all(x[2] for x in s)
        pads = {FR.front_back(cp) for cp in case("seam_" + m)["copies"][0][1:]}
        assert {a for a, _b in pads} == set(SEAM_PADS) == {b for _a, b in pads}
    rows = twin("item_search", 1)[0]
    assert [len(r) for r in rows] == [0, 1, 5, 100, 0]
    assert [items_of(len(x[1])) for x in rows[3]] == [1, 4] * 50
    ends = case("contig_ends_items")["copies"]
    a, b = twin("contig_ends_items", 0)[0], twin("contig_ends_items", 1)[0]
    assert [len(r) for r in a] == [len(c) for c in ends] and [len(r) for r in b] == [0] + [len(c) for c in ends[1:]]
    assert not any(x[2] for x in a[0]) and all(x[2] for r in a[1:] for x in r)
    assert {items_of(len(x[1])) for x in b[2]} == {2}
