"""The cases of tests/copy_limit_cases.py on the CPU: every builder reaches the edge it is named for (it asserts so with the model),
the case set as a whole names every edge of the minimizer, occurrence, sort-class, chain, extension, filter and cap limits
(test_coverage), and the twin (oracle/hite_oracle_copies.c: orc_find_copies), which is the definition of the copy table, gives the
rows, clip words and anchor counts the constructions are built for.  tests/test_gpu_copy_limits.py compares the device with the same
tables."""
import pytest

import copy_limit_cases as CL
import oracle_lib as O
import seed_limit_cases as SC


def twin_table(case, cands=None):
    O.find_copies_config(case["aligned"])
    try:
        return O.find_copies(case["contigs"], case["cands"] if cands is None else cands, clips=True)
    finally:
        O.find_copies_config(None)


_tables = {}


def table_of(name):
    if name not in _tables:
        _tables[name] = twin_table(CL.get(name))
    return _tables[name]


@pytest.mark.parametrize("name", CL.names())
def test_case_against_twin(name):
    """the builder's own assertions, then the twin's table: rows per candidate, clip words and anchor counts of the construction; the
    sort keys (anchors capped at 4095, global start, strand) of a candidate's rows are unique: the order of the table is defined"""
    c = CL.get(name)
    t = table_of(name)
    CL.check_closed_forms(name, t)
    coff = [0]
    for s in c["contigs"]:
        coff.append(coff[-1] + len(s))
    for rows in t:
        keys = [(min(r[4], 4095), coff[r[0]] + r[1], r[3]) for r in rows]
        assert len(set(keys)) == len(keys), name
        assert keys == sorted(keys, key=lambda k: (-k[0], k[1], k[2])), name


def test_coverage():
    """no edge of the issue's list is missing from the case set"""
    cov = CL.coverage()
    missing = [e for e in CL.REQUIRED if e not in cov]
    assert not missing, missing


def test_split_minimizers_are_the_plain_ones():
    """contig_minimizers (cut at runs of N, a piece computed once) == the minimizers of seed_limit_cases, on arrays and at contig ends"""
    u = CL.get("array_1999")["cands"][0]
    for s in (("N" * 70).join([u] * 9), "NNN" + ("N" * 10).join([u] * 12) + "N" * 9, CL.get("dense_array_cut")["contigs"][1][:3000],
              CL.get("chain_counts")["contigs"][0][:4000], "N" * 500, u + "N" * 400):
        assert CL.contig_minimizers(s) == [(p, hs) for p, hs, _w in SC.minimizers(s)]


def test_alone_is_the_batch():
    """a candidate of groups 1 and 3 searched alone gives the rows it has in its batch (the twin has no state to carry over: this pins
    the expectation the GPU test holds the device to)"""
    for name in ("ext_long", "anchors_2_and_3"):
        c = CL.get(name)
        for k in c["alone"]:
            assert twin_table(c, [c["cands"][k]])[0] == table_of(name)[k], (name, k)


def test_minimizer_candidates_have_copies_at_every_alignment():
    """most candidates of the minimizer case have copies, on both strands, and their offsets in the batch take all four values mod 4"""
    c, t = CL.get("minimizer_limits"), table_of("minimizer_limits")
    off, seen = 0, set()
    for q, rows in zip(c["cands"], t):
        if {r[3] for r in rows} == {0, 1}:
            seen.add(off % 4)
        off += len(q)
    assert seen == {0, 1, 2, 3}, seen
    assert sum(1 for rows in t if rows) >= len(t) - 8


def test_extensions_start_at_every_byte_alignment():
    """the end extension reads the candidate through aligned words: over the chains of the chain and extension cases (as the model
    clusters them), the first byte read takes all four alignments at either end on either strand"""
    seen = set()
    for name in CL.names("chains") + ["band_and_n", "minimizer_limits"]:
        c = CL.get(name)
        index = CL.index_of(c["contigs"])
        qb = 0
        for q in c["cands"]:
            L = len(q)
            for x in CL.clusters_of(index, q):
                nl, nr = x["qlo"], L - (x["qhi"] + CL.K)
                if x["na"] < CL.MINANCH or not x["span_ok"] or nl > CL.EXT_MAXLEN or nr > CL.EXT_MAXLEN:
                    continue
                if nl >= 1:
                    seen.add((0, x["rel"], (qb + L - x["qlo"] if x["rel"] else qb + x["qlo"] - 1) % 4))
                if nr >= 1:
                    seen.add((1, x["rel"], (qb + L - 1 - (x["qhi"] + CL.K) if x["rel"] else qb + x["qhi"] + CL.K) % 4))
            qb += L
    assert len(seen) == 16, sorted(seen)


def test_overhang_rows_lie_at_the_contig_ends():
    """aligned interval: it ends where the contig ends; whole-candidate interval: the same rows after clamping, no clip words"""
    for v in CL.OVERHANGS[:-1]:
        a, w = table_of("overhang_%d_aligned" % v), table_of("overhang_%d_whole" % v)
        lens = [len(s) for s in CL.get("overhang_%d_aligned" % v)["contigs"]]
        for k in range(2):
            assert [r[:5] for r in a[k]] == [r[:5] for r in w[k]] and all(r[5] == 0 for r in w[k]), v
            by = {r[0]: r for r in a[k]}
            assert by[0][1] == 1 and by[4][1] == 1 and by[1][2] == lens[1] and by[5][2] == lens[5], (v, a[k])
            assert all(r[2] - r[1] + 1 == 600 - v for r in a[k]), (v, a[k])


def test_cap_cut_is_decided_by_the_global_start():
    """cap_order: three anchor counts in the table; the last group is cut: its kept rows are the 280 with the smallest GLOBAL starts (all
    of contig 0's, then contig 1's first), and with the contigs swapped the rows dropped before appear with the SAME anchor count"""
    c, t = CL.get("cap_order"), table_of("cap_order")[0]
    lo = min(c["anchors"])
    assert len(t) == CL.MAXCOPY and len({r[4] for r in t}) >= 3 and t[-1][4] == lo
    last = [r for r in t if r[4] == lo]
    assert len(last) == 280 and {r[0] for r in t} == {0, 1}
    assert [r[0] for r in last] == [0] * 150 + [1] * 130 and last == sorted(last, key=lambda r: (r[0], r[1]))
    swapped = O.find_copies(c["contigs"][::-1], c["cands"], clips=True)[0]
    low2 = [r for r in swapped if r[4] == lo]
    assert len(low2) == 280 and [r[0] for r in low2] == [0] * 150 + [1] * 130
    # contig 1 of the first order is contig 0 of the second: its 150 rows of the last group appear, 130 of them in the first table too
    first = sorted(r[1] for r in last if r[0] == 1)
    second = sorted(r[1] for r in low2 if r[0] == 0)
    assert len(second) == 150 and second[:130] == first            # the 20 behind them were dropped with equal anchors: the start decided
