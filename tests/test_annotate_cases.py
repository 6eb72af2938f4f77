"""CPU-only: the twin of the genome annotation (tests/annotate_twin.py, both forms) on the labelled cases of tests/annotate_cases.py:
every case reaches the limit it names (its closed forms of counters, records and status), the two forms of the twin agree, a record
buffer that is too small is reported with the true count, and the twin alone meets the recall bar on the planted genome that
tests/test_gpu_annotate.py holds the HIP code to."""
import functools

import pytest

import annotate_cases as AC
import annotate_twin as AT

CASES = AC.small_cases()


def _by_label(label):
    (c,) = [c for c in CASES if c["label"] == label]
    return c


@functools.lru_cache(maxsize=None)
def _twin(k):
    c = CASES[k]
    st = {}
    recs, status = AT.annotate(c["seqs"], c["lib"], c["piece_len"], stats=st)
    return recs, status, st


@pytest.mark.parametrize("k", range(len(CASES)), ids=[c["label"] for c in CASES])
def test_case_reaches_what_it_names(k):
    c = CASES[k]
    recs, status, st = _twin(k)
    assert {n: st[n] for n in c["stats"]} == c["stats"]
    if c["records"] is not None:
        assert recs == c["records"]
    if c["status"] is not None:
        assert status == c["status"]
    assert st["records"] == len(recs) == st["hsps"] - st["duplicates"] - st["dominated"]
    assert st["runs"] == st["hsps"] + st["no_hsp"] and st["alignments"] == st["runs"] + st["redos"]
    key = [AT.order_key(r) for r in recs]
    assert key == sorted(key)


def test_the_list_covers_the_limits():
    labels = " | ".join(c["label"] for c in CASES)
    for word in ("16 table entries", "17 table entries", "chain of 2 hits", "chain of 3 hits", "gap of 300", "gap of 301", "bin edge", "both lattices",
                 "reverse complement", "another byte", "lower-case", "pad level 1", "pad level 2", "pad level 3", "MAX_SPAN", "MAX_LIB_LEN + 1",
                 "piece edge", "80 %", "79 %", "each end", "empty and short", "no entry"):
        assert word in labels, word
    assert len(CASES) >= 30


def test_the_seeded_copy_of_20000_bases_ends_inside_it():
    k = [c["label"] for c in CASES].index("a copy of 20 000 bases seeded in its middle: the last pad does not reach its ends")
    ((seq, gs, ge, lib, strand, qs, qe, _s, _m, _c),) = _twin(k)[0]
    assert (seq, lib, strand) == (0, 0, 0) and gs - 700 == qs and ge - 700 == qe
    # the run is the exact stretch around bases 9 980 .. 10 020 of the entry; the last pad is 8 192
    assert 10000 - 20 - 10 - AT.PADS[-1] <= qs <= 10000 - AT.PADS[-1] and 10000 + AT.PADS[-1] <= qe <= 10000 + 20 + 10 + AT.PADS[-1]


def test_piece_len_changes_the_hits_and_not_the_records():
    a, b = _by_label("a copy across a piece edge"), _by_label("the same genome in one piece")
    assert a["seqs"] == b["seqs"] and a["piece_len"] == 4096 and b["piece_len"] == 0
    assert AT.pieces(12000, 4096) == [(0, 12000), (4096, 12000), (8192, 12000)] and AT.pieces(12000, 0) == [(0, 12000)]
    ra, _sa, sta = _twin(CASES.index(a))
    rb, _sb, stb = _twin(CASES.index(b))
    assert ra == rb and sta["hits"] - stb["hits"] >= 4500 - 12 - 4096 and sta["duplicates"] == stb["duplicates"] + 2


def test_pieces():
    assert AT.pieces(0, 0) == [] and AT.pieces(5, 256) == [(0, 5)] and AT.pieces(256, 256) == [(0, 256)]
    assert AT.pieces(257, 256) == [(0, 257), (256, 257)]
    n = AT.PIECE + AT.OVERLAP + 1
    assert AT.pieces(n, 0) == [(0, n - 1), (AT.PIECE, n)]


@pytest.mark.parametrize("k", [k for k, c in enumerate(CASES) if sum(map(len, c["seqs"])) <= 30000 and sum(map(len, c["lib"])) <= 30000],
                         ids=lambda k: CASES[k]["label"])
def test_python_form_equals_c_form(k):
    c = CASES[k]
    st = {}
    recs, status = AT.annotate(c["seqs"], c["lib"], c["piece_len"], stats=st, form="py")
    assert (recs, status, st) == _twin(k)


def test_pure_python_alignment_on_a_small_case():
    c = _by_label("two entries on one locus, 79 % of the lesser under the better")
    small = dict(c, seqs=[c["seqs"][0][900:2300]])
    a = AT.annotate(small["seqs"], small["lib"], form="py", align=AT.align_py)
    assert a == AT.annotate(small["seqs"], small["lib"]) and len(a[0]) == 2


def test_a_cap_smaller_than_the_result():
    c = _by_label("copies in three sequences")
    recs, _status, st, rc = AT.annotate_c(c["seqs"], c["lib"], cap=3)
    assert rc == -4 and st["records"] == 4 and recs == c["records"][:3]
    recs, _status, st, rc = AT.annotate_c(c["seqs"], c["lib"], cap=4)
    assert rc == 0 and recs == c["records"]
    assert AT.annotate_c(c["seqs"], c["lib"], cap=0)[3] == -4


def test_limits():
    with pytest.raises(ValueError):
        AT.annotate(["ACGT"], ["ACGT"], piece_len=AT.MIN_PIECE - 1)
    with pytest.raises(ValueError):
        AT.annotate(["ACGT"], ["ACGT"], piece_len=AT.PIECE + 1)
    with pytest.raises(ValueError):
        AT.annotate(["ACGT"], ["A"] * (AT.MAX_LIB + 1))
    assert AT.annotate(["ACGT"], ["ACGT"], piece_len=AT.MIN_PIECE) == ([], [0])


def test_resolve_has_no_order_dependence():
    """A is held against every B, kept or not: C is dropped by B although A drops B"""
    a, b, c = (0, 0, 1000, 0, 0, 0, 1000, 2000, 1000, 1000), (0, 200, 1200, 1, 0, 0, 1000, 1900, 1000, 1000), (0, 400, 1400, 2, 0, 0, 1000, 1800, 1000, 1000)
    for recs in ([a, b, c], [c, b, a], [b, c, a]):
        st = dict.fromkeys(AT.STATS, 0)
        assert AT.resolve(list(recs), st) == [a] and st["dominated"] == 2
    st = dict.fromkeys(AT.STATS, 0)
    tie = (0, 0, 1000, 1, 0, 0, 1000, 2000, 1000, 1000)      # the same score: the smaller order key is the better one
    assert AT.resolve([tie, a], st) == [a] and AT.resolve([a, a], st) == [a] and st["duplicates"] == 1


def test_the_twin_alone_meets_the_recall_bar_on_the_planted_genome():
    """the condition of tests/test_gpu_annotate.py, checked before a GPU is involved: every planted copy at 10 % divergence or less is
    covered for at least 90 % of its length by records of its own entry and strand"""
    genome, lib, truth = AC.planted()
    assert len(genome) == 2_000_000 and len(lib) == 40 and len(truth) == 320
    assert {r[4] for r in truth} == set(AC.DIVERGENCES) and {r[1] for r in truth} == {0, 1}
    recs, status = AC.planted_twin()[:2]
    assert status == [0] * 40
    low = [r for r in truth if r[4] <= 0.10]
    assert len(low) == 240
    for row in low:
        assert 10 * AC.coverage(row, recs) >= 9 * (row[3] - row[2]), row
