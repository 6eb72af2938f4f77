"""CPU-only: the Helitron candidate scan off the GPU -- the pattern grammar (util.parse_lcvs) on the tool's 880 lines and on refused
lines; the twin (tests/helitron_twin.py) against an independent count with `re` and against what every case of
tests/helitron_cases.py expects; the scoring code of hite_amd/csrc/hite_helitron.hip compiled for the host (tests/helitron_host.py)
against the twin.  tests/test_gpu_helitron.py runs the same cases on the device."""
import re

import numpy as np
import pytest

import helitron_cases as HC
import helitron_host as HH
import helitron_twin as T
from hite_amd import util


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return HH.build(tmp_path_factory.mktemp("helitron_host"))


def test_parser_round_trip_on_the_tool_lists():
    head, tail = HC.lcv_lists()
    assert (len(head), len(tail)) == (304, 576) and len(set(head)) < len(head)        # repeated lines stay
    for side, lines in (("head", head), ("tail", tail)):
        rec = util.parse_lcvs(lines, side)
        assert len(rec) == len(lines)
        assert [util.lcv_line(r, side) for r in rec] == lines
        assert int(rec["body_len"].max()) <= 32 and int(rec["gap_max"].max()) <= 63
        for r, line in zip(rec, lines):                  # the twin's own grammar reads the same numbers
            gmin, gmax, body = T.parse(line, side)
            assert (int(r["gap_min"]), int(r["gap_max"]), int(r["body_len"])) == (gmin, gmax, len(body))
    assert int(util.parse_lcvs(head, "head")["gap_max"].max()) == 39 and max(len(x) for x in head + tail) == 27
    rec = util.parse_lcvs(["", "# a comment", "  TC.{3,9}AC.T  ", "TCG"], "head")
    assert [util.lcv_line(r, "head") for r in rec] == ["TC.{3,9}AC.T", "TCG"]
    assert len(util.parse_lcvs([], "tail")) == 0


@pytest.mark.parametrize("side,line", [
    ("head", "TC.{64}ACGT"), ("head", "TC.{3,64}ACGT"), ("head", "TC.{5,3}ACGT"), ("head", "TC" + "ACGT" * 8 + "A"), ("head", "TCAC[AG]T"),
    ("head", "TC.ACGT"), ("head", "TCACG."), ("head", "TC"), ("head", "GAACGT"), ("head", "TCacgt"), ("head", "TCAC.{2}GT"), ("head", "TCACNT"),
    ("tail", "ACGT.{64}CT[AG]{2}"), ("tail", "ACGT" * 8 + "A" + "CT[AG]{2}"), ("tail", "ACGTCT[AG]{3}"), ("tail", "ACGTCTAG"), ("tail", ".CGTCT[AG]{2}"),
    ("tail", "ACG..{2}CT[AG]{2}"), ("tail", "CT[AG]{2}"), ("tail", "AC|GTCT[AG]{2}"), ("tail", "TC.{2}ACGT")])
def test_parser_refuses(side, line):
    with pytest.raises(ValueError) as e:
        util.parse_lcvs(["TCACGT" if side == "head" else "ACGTCT[AG]{2}", line], side)
    assert line in str(e.value) and "line 2" in str(e.value)


def test_parser_accepts_the_limits():
    rec = util.parse_lcvs(["TC.{63}" + "ACGT" * 8, "TC.{0,63}A"], "head")
    assert rec["gap_max"].tolist() == [63, 63] and rec["body_len"].tolist() == [32, 1] and int(rec["care"][0]) == 2 ** 64 - 1
    rec = util.parse_lcvs(["ACGT" * 8 + ".{63}CT[AG]{2}"], "tail")
    assert rec["gap_min"].tolist() == [63] and rec["body_len"].tolist() == [32]


def _re_scores(seqs, head, tail):
    """per position, the number of lines whose regular expression matches there: heads at the T of TC, tails at the
    last base of CT[AG][AG].  The sequences are joined by line feeds,
    which `.` does not match and no letter does: nothing matches across a sequence end.  -> [2, total bytes]"""
    text = "\n".join(seqs)
    keep = np.array([c != "\n" for c in text], dtype=bool)
    hs, ts = np.zeros(len(text), dtype=np.int32), np.zeros(len(text), dtype=np.int32)

    def starts(expr, txt):       # every position a match begins at, overlapping ones too
        pat, at = re.compile(expr), 0
        while True:
            m = pat.search(txt, at)
            if m is None:
                return
            yield m.start()
            at = m.start() + 1

    for line in head:
        for p in starts(line, text):
            hs[p] += 1
    for line in tail:            # one expression of fixed length per gap of the range; a position counts once per line
        gmin, gmax, body = T.parse(line, "tail")
        ends = set()
        for g in range(gmin, gmax + 1):
            ends.update(p + len(body) + g + 3 for p in starts("%s.{%d}CT[AG]{2}" % (body, g), text))
        for q in ends:
            ts[q] += 1
    return np.stack([hs[keep], ts[keep]])


def test_twin_vs_regular_expressions():
    head, tail = HC.lcv_lists()
    seqs = HC.random_batch(5, 200, 2000)
    seqs[3] = seqs[3][:700] + "N" * 40 + seqs[3][740:]
    seqs += ["", "TC", HC.rand_dna(np.random.default_rng(1), 37)]
    got = T.scores(seqs, head, tail)
    plus, minus = _re_scores(seqs, head, tail), _re_scores([T.revcomp(s).decode() for s in seqs], head, tail)
    assert np.array_equal(got[:2], plus) and np.array_equal(got[2:], minus)
    assert int((plus[0] > 0).sum()) > 100 and int((plus[1] > 0).sum()) > 100 and int(got.max()) >= 2


def _check_expect(c, rec, sc):
    exp = c["expect"]
    off = np.concatenate([[0], np.cumsum([len(s) for s in c["seqs"]])])
    if exp["records"] is not None:
        assert [tuple(r) for r in rec] == exp["records"], c["label"]
    for (row, q, pos), v in exp["scores"].items():
        assert int(sc[row, off[q] + pos]) == v, (c["label"], row, q, pos)
    if exp["nonzero"] is not None:
        for row, v in enumerate(exp["nonzero"]):
            assert v is None or int((sc[row] > 0).sum()) == v, (c["label"], row)


def test_every_case_expectation_against_the_twin():
    cases = HC.small_cases() + HC.batch_cases()
    assert len(cases) > 50
    for c in cases:
        rec = T.scan(c["seqs"], c["head"], c["tail"], **c["kw"])
        _check_expect(c, rec, T.scores(c["seqs"], c["head"], c["tail"]))
    real = [c for c in cases if c["label"] == "the tool's lists"][0]             # (24 planted elements and what random text adds)
    assert len(T.scan(real["seqs"], real["head"], real["tail"], **real["kw"])) >= 24


def test_host_compiled_scoring_vs_twin(host):
    n = 0
    for c in HC.small_cases() + HC.batch_cases():
        hp, tp = util.parse_lcvs(c["head"], "head"), util.parse_lcvs(c["tail"], "tail")
        st_t, st_h = {}, {}
        want = T.scan(c["seqs"], c["head"], c["tail"], stats=st_t, **c["kw"])
        assert np.array_equal(HH.scores(host, c["seqs"], hp, tp), T.scores(c["seqs"], c["head"], c["tail"])), c["label"]
        got = HH.scan(host, c["seqs"], hp, tp, stats=st_h, **c["kw"])
        assert got.tolist() == [list(r) for r in want] and st_h == st_t, c["label"]
        n += len(want)
    assert n > 60


def test_host_compiled_scoring_vs_twin_random(host):
    head, tail = HC.lcv_lists()
    hp, tp = util.parse_lcvs(head, "head"), util.parse_lcvs(tail, "tail")
    rng = np.random.default_rng(8)
    seqs = HC.random_batch(6, 60, 3000) + [HC.rand_dna(rng, int(n)) for n in rng.integers(0, 120, 80)]
    seqs[7] = "".join(c if rng.random() > 0.03 else "Nn-acgt"[int(rng.integers(0, 7))] for c in seqs[7])
    assert np.array_equal(HH.scores(host, seqs, hp, tp), T.scores(seqs, head, tail))
    for lr, ht, tt in (((200, 20000), 1, 1), ((50, 400), 1, 2), ((1, 3000), 2, 1)):
        st_t, st_h = {}, {}
        want = T.scan(seqs, head, tail, ht, tt, lr, stats=st_t)
        got = HH.scan(host, seqs, hp, tp, ht, tt, lr, stats=st_h)
        assert len(want) >= 10 and got.tolist() == [list(r) for r in want] and st_h == st_t


def test_host_compiled_refuses_malformed_records(host):
    good = util.parse_lcvs(["TC.{2}ACG.T"], "head")
    tail = util.parse_lcvs(["ACGTCT[AG]{2}"], "tail")
    for field, value in (("body_len", 0), ("body_len", 33), ("gap_max", 64), ("gap_min", 3), ("care", 1), ("care", 3 << 10), ("body", 3 << 6)):
        bad = good.copy()
        bad[field][0] = value
        with pytest.raises(AssertionError):
            HH.scores(host, ["ACGT"], bad, tail)
    assert HH.scores(host, ["ACGT"], good, tail).shape == (4, 4)


def test_lcv_dir_lookup(tmp_path, monkeypatch):
    monkeypatch.delenv("HITE_HSDIR", raising=False)
    assert util.helitron_lcv_dir(None) is None and util.helitron_lcv_dir(str(tmp_path)) is None
    head, tail = HC.lcv_lists()
    a, b = tmp_path / "a", tmp_path / "b"
    for d in (a, b):
        d.mkdir()
        (d / "head.lcvs").write_text("\n".join(head) + "\n")
    (b / "tail.lcvs").write_text("\n".join(tail) + "\n")
    assert util.helitron_lcv_dir(str(a)) is None            # one list alone is no directory of lists
    assert util.helitron_lcv_dir(str(b)) == str(b)
    monkeypatch.setenv("HITE_HSDIR", str(b))
    assert util.helitron_lcv_dir(None) == str(b) and util.helitron_lcv_dir(str(a)) == str(b)
    with pytest.raises(FileNotFoundError):
        monkeypatch.delenv("HITE_HSDIR")
        util.multi_process_helitronscanner(str(tmp_path / "x.fa"), str(tmp_path / "y.fa"), None, None, str(a), None, 1, 0)


def test_twin_alone_meets_the_stage_condition():
    """what tests/test_gpu_helitron.py asks of the stage script on the GPU, from the twin alone: of the planted families with >= 3
    copies at least 80 % have a candidate with both ends within 3 bases of a planted copy (families shorter than the 200-base
    minimum and elements with a nearer tail inside them are the misses)"""
    head, tail = HC.lcv_lists()
    g, names, seqs = HC.stage_input()
    rec = T.scan(seqs, head, tail)
    n_fam, hit = HC.stage_recall(g, ["%s_%d_%d_%s" % (names[q], s + 1, e, "-" if st else "+") for q, s, e, st, _h, _t in rec])
    assert n_fam >= 5 and hit >= 0.8 * n_fam, (n_fam, hit)
