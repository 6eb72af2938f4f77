"""CPU: util.ltr_flank_decide with the high-copy vote of the hybrid CNN, driven through the twins (tests/framecluster_twin.py, the
oracle's frame vote, tests/ltrdeep_twin.py) on the matrices of tests/golden/ltr_flank_filter.json.gz.  Without a model the result
must be what the function returned before it knew of a model: tests/golden/ltr_flank_decide_recorded.json.gz is that return value,
recorded from the commit before the model was added (same matrices, same twins)."""
import os

import numpy as np
import pytest

import framecluster_twin as FT
import ltrdeep_twin as T
import oracle_lib as O
from conftest import load_golden
from hite_amd import util

HERE = os.path.dirname(os.path.abspath(__file__))


def frame_vote(matrices, flank, window, side):
    return [O.ltr_frame(list(rows), flank, window, side) for rows in matrices]


@pytest.fixture(scope="module")
def world():
    g = load_golden("ltr_flank_filter")
    rec = load_golden("ltr_flank_decide_recorded")
    mats = {c["name"]: [tuple(r) for r in c["matrix"]] for c in g["cases"]}
    recorded = ({n: tuple(v) for n, v in rec["table"].items()}, {n: [tuple(r) for r in m] for n, m in rec["high"].items()})
    params = np.load(os.path.join(HERE, "golden", "ltr_deep_model.npy"))
    votes = util.ltr_deep_votes(recorded[1], params, deep=T.ltr_deep)          # the twin's votes, computed once
    return dict(flank=g["flank"], mats=mats, recorded=recorded, params=params, votes=votes)


def test_without_a_model_nothing_changes(world, monkeypatch):
    monkeypatch.delenv("HITE_LTR_DEEP", raising=False)
    seconds = {}
    got = util.ltr_flank_decide(world["mats"], world["flank"], cluster=FT.frame_cluster, frame_vote=frame_vote, seconds=seconds)
    assert got == world["recorded"] and "deep" not in seconds
    assert got == util.ltr_flank_decide(world["mats"], world["flank"], cluster=FT.frame_cluster, frame_vote=frame_vote, model=None, deep=T.ltr_deep)


def test_with_the_model_high_copy_is_homology_and_model(world):
    table0, high0 = world["recorded"]
    votes = world["votes"]
    assert sorted(votes) == sorted(high0) and len(high0) >= 8 and set(votes.values()) == {0, 1}      # every high-copy matrix is scored; both answers occur
    seconds = {}
    table, high = util.ltr_flank_decide(world["mats"], world["flank"], cluster=FT.frame_cluster, frame_vote=frame_vote, seconds=seconds,
                                        model=world["params"], deep=T.ltr_deep)
    assert high == high0 and sorted(table) == sorted(table0) and "deep" in seconds
    for n, old in table0.items():
        if old[1] != "high":
            assert table[n] == old, n                                   # low-copy and dropped candidates: unchanged
        elif old[0] and not votes[n]:
            assert table[n] == (False, "high", "deep"), n
        else:
            assert table[n] == old, n                                   # the model can only veto what the homology rule passes ...
    merged = util.alter_deep_learning_results(votes, {n: int(table0[n][0]) for n in high0}, list(high0))
    assert {n: table[n][0] for n in high0} == {n: bool(merged[n]) for n in high0}


def test_veto_and_absent_cases(world):
    """a frame vote that fails one high-copy candidate and a model that leaves two unscored: the homology rule's 0 stands, a candidate
    the homology rule passes and the model did not score is no LTR ("deep_missing")"""
    high0 = world["recorded"][1]
    names = sorted(high0)
    failed, unscored, says_no = names[0], {names[0], names[1]}, names[2]
    mats = {n: world["mats"][n] for n in names}

    def vote(matrices, flank, window, side):
        return [(n != failed, 0) for n, _m in zip(order, matrices)]

    def deep(model, matrices, pooled=False):
        assert model == "the model"
        logits = np.array([[1.0, -1.0] if n == says_no else [-1.0, 1.0] for n in order], dtype=np.float32)
        return logits, np.array([1 if n in unscored else 0 for n in order], dtype=np.int8)

    def cluster(groups, **kw):          # every row alone: the sort rule and the joined rule keep every matrix in its order
        return [[[r] for r in range(len(g))] for g in groups]

    order = names
    mats = {n: mats[n] for n in order}
    table, high = util.ltr_flank_decide(mats, world["flank"], cluster=cluster, frame_vote=vote, model="the model", deep=deep)
    assert list(high) == order
    for n in order:
        exp = ((False, "high", "frame_vote") if n == failed else (False, "high", "deep_missing") if n in unscored else
               (False, "high", "deep") if n == says_no else (True, "high", None))
        assert table[n] == exp, n
    # a threshold above every probability: the model rejects all it scored
    table, _high = util.ltr_flank_decide(mats, world["flank"], cluster=cluster, frame_vote=vote, model="the model", deep=deep, threshold=0.99)
    assert all(table[n] == (False, "high", "deep") for n in order if n != failed and n not in unscored)
