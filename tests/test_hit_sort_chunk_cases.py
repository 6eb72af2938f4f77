"""The cases of tests/hit_sort_chunk_cases.py on the CPU: every builder reaches the hit counts and contig counts it is named for (it
asserts so with the model of tests/copy_limit_cases.py), the case set names every place where the per-candidate sort changes shape
(test_coverage), and the twin (oracle/hite_oracle_copies.c: orc_find_copies), which is the definition of the copy table, gives the
rows the constructions are built for.  tests/test_gpu_hit_sort_chunks.py compares the device with the same tables."""
import pytest

import hit_sort_chunk_cases as HC
import oracle_lib as O


def twin_table(case, cands=None):
    O.find_copies_config(case["aligned"])
    try:
        return O.find_copies(case["contigs"], case["cands"] if cands is None else cands, clips=True)
    finally:
        O.find_copies_config(None)


_tables = {}


def table_of(name):
    if name not in _tables:
        _tables[name] = twin_table(HC.get(name))
    return _tables[name]


@pytest.mark.parametrize("name", HC.names())
def test_case_against_twin(name):
    """the builder's own assertions, then the twin's table: rows per candidate as the construction gives them; the sort keys (anchors
    capped at 4095, global start, strand) of a candidate's rows are unique: the order of the table is defined"""
    c = HC.get(name)
    t = table_of(name)
    HC.check_closed_forms(name, t)
    coff = [0]
    for s in c["contigs"]:
        coff.append(coff[-1] + len(s))
    for rows in t:
        keys = [(min(r[4], 4095), coff[r[0]] + r[1], r[3]) for r in rows]
        assert len(set(keys)) == len(keys), name
        assert keys == sorted(keys, key=lambda k: (-k[0], k[1], k[2])), name


def test_coverage():
    """no hit count or contig count of the list is missing from the case set"""
    cov = HC.coverage()
    missing = [e for e in HC.REQUIRED if e not in cov]
    assert not missing, missing


def test_chunk_lengths():
    """E = ceil(n / NT) | 1 on both sides of every border the cases are named for, and the batches of the global class"""
    assert [HC.chunk(n) for n in (2, 3, 255, 256, 257, 1984, 1985, 3840, 3841, 4096)] == [1, 1, 1, 1, 3, 9, 9, 15, 17, 17]
    assert [HC.chunk(n) for n in (4097, 7680, 7681, 8192, 15872, 15873, 20000)] == [9, 15, 17, 17, 31, 33, 41]
    # the largest chunk of each LDS class is the bound its kernel is unrolled to; it fits the 8-bit count of one digit
    assert max(HC.chunk(n) for n in range(2, HC.HS_FIRST + 1)) == 9 and max(HC.chunk(n) for n in range(HC.HS_FIRST + 1, 8193)) == 17 < 256
    assert HC.HS_BATCH < 256


def test_arrays_give_a_row_per_copy():
    """a unit of >= 3 minimizers in an array: a row per copy up to the cap of 300, each with the unit's anchors, on the forward strand;
    a unit of 2 minimizers: no row"""
    for name in ("chunk_small", "chunk_mid", "chunk_global"):
        c, t = HC.get(name), table_of(name)
        for k, n in c["rows"].items():
            m = len(HC.CL.kept_minimizers(c["cands"][k]))
            assert len(t[k]) == n and all(r[4] == m and r[3] == 0 for r in t[k]), (name, k)
    assert HC.get("chunk_small")["rows"][0] == 0


def test_contig_end_cuts_the_run():
    """the run of 800 hits is two clusters at every contig count, neither is a chain, and the element in the middle contig is found
    once, in that contig"""
    for name in ("contigs_94", "contigs_95", "contigs_96"):
        c, t = HC.get(name), table_of(name)
        nc = len(c["contigs"])
        assert t[0] == [] and len(t[1]) == 1 and t[1][0][0] == nc // 2 and t[1][0][3] == 0, (name, t[1])
        assert t[1][0][2] - t[1][0][1] + 1 == 200, (name, t[1])


def test_alone_is_the_batch():
    """a candidate searched alone gives the rows it has in its batch (the twin has no state to carry over: this pins the expectation
    the GPU test holds the device to)"""
    for name in ("chunk_small", "contigs_95"):
        c = HC.get(name)
        for k in c["alone"]:
            assert twin_table(c, [c["cands"][k]])[0] == table_of(name)[k], (name, k)
