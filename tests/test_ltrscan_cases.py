"""CPU-only: the definition of the LTR candidate scan (include/hite_gpu.h, "LTR candidate scan") as its twin states it
(tests/ltrscan_twin.py, tests/ltrscan_twin.c): the closed forms of tests/ltrscan_cases.py, the Python form against the C form on
every small case, the limits, and the two conditions on the genome of 32 planted elements -- every element found at exactly its
planted place, and the chain into util.ltr_scn_filter keeping what it should.  The HIP code is held to the twin in
tests/test_gpu_ltrscan.py."""
import os
import re

import pytest

import ltrscan_cases as LC
import ltrscan_twin as LT
import pairhsp_twin as PT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_in_the_header():
    txt = open(os.path.join(ROOT, "include", "hite_gpu.h")).read()
    for name, v in (("WORD", LT.WORD), ("MAX_OCC", LT.MAX_OCC), ("BIN_SHIFT", LT.BIN_SHIFT), ("LATTICE", LT.LATTICES[1]), ("GAP", LT.GAP),
                    ("MIN_HITS", LT.MIN_HITS), ("BAND_BELOW", LT.BAND_BELOW), ("BAND_ABOVE", LT.BAND_ABOVE), ("PAD_0", LT.PADS[0]),
                    ("PAD_1", LT.PADS[1]), ("PAD_2", LT.PADS[2]), ("EDGE", LT.EDGE), ("MAX_REDO", LT.MAX_REDO), ("MAX_LTR", LT.MAX_LTR),
                    ("STATS", len(LT.STATS))):
        assert re.search(r"^#define HITE_LTRSCAN_%s +%s$" % (name, v), txt, re.M), name
    assert LT.LATTICES == (0, 32)


def test_closed_forms():
    n_rec = n_stat = 0
    for c in LC.small_cases():
        st = {}
        recs = LT.scan(c["seqs"], stats=st, **c["kw"])
        if c["records"] is not None:
            assert recs == c["records"], c["label"]
            n_rec += 1
        for k, v in (c["stats"] or {}).items():
            assert st[k] == v, (c["label"], k, st[k], v)
            n_stat += 1
        assert st["records"] == len(recs)
        assert st["runs"] - st["runs_span"] - st["no_hsp"] - sum(st[k] for k in LT.STATS[7:11]) >= st["records"], c["label"]
        assert st["alignments"] - st["redos"] == st["runs"] - st["runs_span"], c["label"]
    assert n_rec >= 45 and n_stat >= 80


def test_python_form_equals_c_form():
    for c in LC.small_cases():
        st_c, st_p = {}, {}
        assert LT.scan(c["seqs"], stats=st_p, form="py", **c["kw"]) == LT.scan(c["seqs"], stats=st_c, **c["kw"]), c["label"]
        assert st_p == st_c, c["label"]


def test_pure_python_alignment_on_the_smallest_cases():
    """step 4 through pairhsp_twin.align (no C at all) where the windows are small"""
    n = 0
    for c in LC.small_cases():
        if c["label"] in ("4 hits", "hit diagonals 992 and 1055", "terminals of min_ltr bases", "a repeat at the first and the last position of its sequence"):
            st_c, st_p = {}, {}
            assert LT.scan(c["seqs"], stats=st_p, form="py", align=LT.align_py, **c["kw"]) == LT.scan(c["seqs"], stats=st_c, **c["kw"]), c["label"]
            assert st_p == st_c
            n += 1
    assert n == 4


def test_every_redo_count_is_among_the_cases():
    seen = set()
    for c in LC.small_cases():
        if c["label"].startswith("terminals of") and "shared words" in c["label"]:
            seen.add(c["stats"]["redos"] // 2)
    assert seen == {0, 1, 2, 3}


def test_band_edge():
    by = {c["label"]: c for c in LC.small_cases()}
    inside, outside = (LT.scan(by["a drift of %d diagonals" % d]["seqs"], **by["a drift of %d diagonals" % d]["kw"]) for d in (95, 97))
    assert len(inside) == 1 and inside[0][7] - inside[0][6] == 95       # one record with 95 gap columns
    assert len(outside) == 2 and all(r[7] - r[6] < 5 for r in outside)   # two records, neither across the 97 bases
    assert [r[1] for r in outside] == [inside[0][1], inside[0][1] + 400] and outside[1][4] - outside[1][3] == 600


def test_one_place_at_several_scores_keeps_the_best():
    c = [c for c in LC.small_cases() if c["label"] == "one place from two bands at two scores"][0]
    s = PT.as_bytes(c["seqs"][0])
    kw = c["kw"]
    hits = LT.links(LT.words(PT.codes(s)), kw["min_ltr"], kw["max_len"] - kw["min_ltr"])
    found = []
    for lam in LT.LATTICES:
        for run in LT.runs(hits, lam):
            if run[4] >= LT.MIN_HITS:
                r = LT.extend(s, run, kw["max_ltr"], PT.align_c, dict.fromkeys(LT.STATS, 0))
                if r is not None:
                    found.append(r)
    by_place = {}
    for r in found:
        by_place.setdefault(r[:4], set()).add(r[4])
    several = {k: v for k, v in by_place.items() if len(v) > 1}
    assert several, by_place
    recs = LT.scan(c["seqs"], **kw)
    for place, scores in several.items():
        assert [r[5] for r in recs if tuple(r[1:5]) == place] == [max(scores)]


def test_limits():
    ok = dict(LT.DEFAULTS)
    assert LT.scan(["ACGT" * 10], **ok) == []
    for bad in (dict(min_ltr=0), dict(min_ltr=6001), dict(max_ltr=8193), dict(min_len=22001), dict(identity=0), dict(identity=101)):
        with pytest.raises(ValueError):
            LT.scan(["ACGT" * 10], **dict(ok, **bad))
        with pytest.raises(AssertionError):
            LT.scan_c(["ACGT" * 10], **dict(ok, **bad))
    assert LT.scan(["ACGT" * 10], **dict(ok, max_ltr=8192, min_ltr=8192)) == []


@pytest.fixture(scope="module")
def planted():
    names, seqs, truth, places = LC.planted()
    st = {}
    return dict(names=names, seqs=seqs, truth=truth, places=places, recs=LT.scan(seqs, stats=st), stats=st)


def test_planted_condition_1_every_element_at_its_place(planted):
    assert len(planted["truth"]) == 32 and sum(len(s) for s in planted["seqs"]) == 293000
    have = {r[:5] for r in planted["recs"]}
    missing = [(t["kind"], p) for t, p in zip(planted["truth"], planted["places"]) if p not in have]
    assert not missing, missing


def test_planted_condition_2_the_chain_into_the_scn_filter(planted, tmp_path):
    from hite_amd import util

    ref = str(tmp_path / "genome.fa")
    util.store_fasta(dict(zip(planted["names"], planted["seqs"])), ref)
    scn = str(tmp_path / "total.scn")
    lines = util.ltr_candidate_scan(ref, scn, scan=LT.scan_array)
    assert len(lines) == len(planted["recs"])
    final, _dirty, _terminals = util.ltr_scn_filter(scn, ref, str(tmp_path / "out"), hsps=PT.pair_hsps)
    kept = {tuple(ln.split(" ")[3:9] + ln.split(" ")[11:12]) for ln in open(final).read().splitlines()}
    n_true = 0
    for t, (seq, ls, le, rs, re_) in zip(planted["truth"], planted["places"]):
        key = tuple(str(x) for x in (ls + 1, le, le - ls, rs + 1, re_, re_ - rs)) + (planted["names"][seq],)
        if t["kind"] in ("clean", "dup", "dirty", "inner", "nested", "shifted"):
            assert key in kept, (t["kind"], key)
            n_true += 1
        elif t["kind"] == "recomb":
            assert key not in kept, key
    assert n_true == 26
