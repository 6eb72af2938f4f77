"""CPU-only: the clustering of frames (include/hite_gpu.h, hite_frame_cluster) and the LTR flank filter built on it, away from the
device --
  - the twin in both its forms (tests/framecluster_twin.py, tests/framecluster_twin.c) against the plain model of
    tests/framecluster_cases.py and against the values and clusters worked out by hand;
  - the decision rules of util.ltr_flank_decide, driven through the twins, against tests/golden/ltr_flank_filter.json.gz: what the
    reference's own generate_sort_matrix, filter_ltr_by_flanking_cluster_sub, get_low/high_copy_LTR_sub and judge_both_ends_frame
    make of the same matrices (tools/gen_ltr_filter_fixture.py);
  - the wrappers under the reference's names on `.matrix` directories against the in-memory driver.
What only the device has is left to tests/test_gpu_framecluster.py and tests/test_gpu_ltr_filter.py."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import framecluster_cases as FC  # noqa: E402
import framecluster_twin as T  # noqa: E402
import oracle_lib as O  # noqa: E402
from conftest import load_golden  # noqa: E402
from hite_amd import util  # noqa: E402


def frame_vote(matrices, flank, window, side):
    """the oracle's frame vote with the interface of Context.ltr_frame"""
    return [O.ltr_frame(list(rows), flank, window, side) for rows in matrices]


def test_pair_values():
    for label, a, b, both, exp in FC.pair_values():
        plain = FC.plain_pair(a, b, both)
        assert T.pair_value(a, b, both) == plain and T.pair_value_c(a, b, both) == plain, label
        if exp is not None:
            assert plain == exp, label


def test_twin_equals_plain_model_on_every_small_case():
    for label, groups, kw in FC.small_cases():
        plain = [FC.plain_cluster(g, **kw) for g in groups]
        assert T.frame_cluster(groups, **kw) == plain, label
        assert T.frame_cluster(groups, form="py", **kw) == plain, label
        if label in FC.EXPECT:
            assert plain == FC.EXPECT[label], label
    assert set(FC.EXPECT) <= {label for label, _g, _k in FC.small_cases()}


def test_both_forms_of_the_twin_at_the_limits():
    for label, groups, kw in FC.length_edges()[2:]:
        assert T.frame_cluster(groups, **kw) == T.frame_cluster(groups, form="py", **kw), label
    for label, groups, kw in FC.row_edges() + FC.length_edges():
        got = T.frame_cluster(groups, **kw)
        assert [g is None for g in got] == [len(g) > FC.MAX_ROWS or any(len(r) > FC.MAX_LEN for r in g) for g in groups], label
        for rows, cls in zip(groups, got):
            if cls is not None:
                assert sorted(r for cl in cls for r in cl) == [k for k in range(len(rows)) if len(rows[k]) > kw["min_len"]], label
    groups = FC.many_small(40)
    assert T.frame_cluster(groups, **FC.SORT) == T.frame_cluster(groups, form="py", **FC.SORT)


@pytest.fixture(scope="module")
def golden():
    g = load_golden("ltr_flank_filter")
    assert 20 <= len(g["cases"]) <= 40 and all(c["sort_pinned"] for c in g["cases"])
    return g


def _rows(m):
    return [tuple(r) for r in m]


def _reaches(case):
    """the matrix the later rules were recorded on: the sorted one, or the input where the sort rule dropped it"""
    return _rows(case["sort"] if case["sort_keep"] else case["matrix"])


def test_options_are_the_reference_command_lines():
    assert util.LTR_SORT_OPTIONS == FC.SORT and util.LTR_JOINED_OPTIONS == FC.JOINED


def test_each_rule_against_the_reference(golden):
    flank = golden["flank"]
    mats = [_rows(c["matrix"]) for c in golden["cases"]]
    kept = util._ltr_sort_batch(mats, T.frame_cluster)
    for c, k in zip(golden["cases"], kept):
        assert (k is not None) == c["sort_keep"], c["name"]
        if k is not None:
            assert k == _rows(c["sort"]), c["name"]       # (rows in the left side's cluster order)
    later = [_reaches(c) for c in golden["cases"]]
    assert util._ltr_joined_batch(later, T.frame_cluster) == [c["flank_keep"] for c in golden["cases"]]
    assert util._ltr_vote_batch(later, flank, 20, frame_vote) == [c["vote"] for c in golden["cases"]]
    assert [len(m) <= 5 for m in later] == [c["low"] for c in golden["cases"]] and [len(m) > 5 for m in later] == [c["high"] for c in golden["cases"]]
    n = lambda key: sum(1 for c in golden["cases"] if c[key])  # noqa: E731
    assert 0 < n("sort_keep") < len(mats) and 0 < n("flank_keep") < len(mats) and 0 < n("vote") < len(mats) and n("low") and n("high")


def _expected_table(golden):
    table = {}
    for c in golden["cases"]:
        if not c["sort_keep"]:
            table[c["name"]] = (False, None, "sort")
        elif not c["flank_keep"]:
            table[c["name"]] = (False, None, "flank_cluster")
        else:
            table[c["name"]] = (c["vote"], "low" if c["low"] else "high", None if c["vote"] else "frame_vote")
    return table


def test_decision_rules_against_the_reference(golden):
    mats = {c["name"]: _rows(c["matrix"]) for c in golden["cases"]}
    seconds = {}
    table, high = util.ltr_flank_decide(mats, golden["flank"], cluster=T.frame_cluster, frame_vote=frame_vote, seconds=seconds)
    exp = _expected_table(golden)
    assert table == exp
    assert {v[2] for v in exp.values()} == {None, "sort", "flank_cluster", "frame_vote"} and {v[1] for v in exp.values()} == {None, "low", "high"}
    assert high == {c["name"]: _rows(c["sort"]) for c in golden["cases"] if exp[c["name"]][1] == "high"}
    assert sorted(seconds) == ["cluster_joined", "cluster_left", "cluster_right", "frame_vote"]
    assert util.ltr_flank_decide({}, golden["flank"], cluster=T.frame_cluster, frame_vote=frame_vote) == ({}, {})


def test_directory_wrappers_write_the_same_table(golden, tmp_path):
    """the reference's sequence of calls (LTR_filter.py:72-170 without the deep model) on `.matrix` directories"""
    flank = golden["flank"]
    d = {k: str(tmp_path / k) for k in ("frames", "sort", "keep", "low", "high", "tmp")}
    os.makedirs(d["frames"])
    for c in golden["cases"]:
        util._write_matrix(os.path.join(d["frames"], c["name"] + ".matrix"), c["matrix"])
    assert util.sort_matrix_dir(d["frames"], d["sort"], d["tmp"], 1, cluster=T.frame_cluster) == (
        len(golden["cases"]), sum(1 for c in golden["cases"] if c["sort_keep"]))
    util.filter_ltr_by_flanking_cluster(d["sort"], d["keep"], d["tmp"], 1, None, cluster=T.frame_cluster)
    util.get_low_copy_LTR(d["keep"], d["low"], 1, copy_num_threshold=5)
    util.get_high_copy_LTR(d["keep"], d["high"], 1, copy_num_threshold=5)
    lc, hc = str(tmp_path / "is_LTR_homo.lc.txt"), str(tmp_path / "is_LTR_homo.hc.txt")
    util.judge_ltr_from_both_ends_frame(d["low"], lc, 1, "Low copy", flank, None, frame_vote=frame_vote)
    util.judge_ltr_from_both_ends_frame(d["high"], hc, 1, "High copy", flank, None, frame_vote=frame_vote)
    got = {}
    for path, label in ((lc, "low"), (hc, "high")):
        for line in open(path):
            name, flag = line.split()
            got[name] = (flag == "1", label)
    exp = {n: (v[0], v[1]) for n, v in _expected_table(golden).items() if v[1] is not None}
    assert got == exp
    assert sorted(os.listdir(d["high"])) == sorted(n + ".matrix" for n, v in exp.items() if v[1] == "high")
