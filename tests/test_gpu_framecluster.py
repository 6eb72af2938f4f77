"""GPU: hite_frame_cluster (hite_amd/csrc/hite_framecluster.hip; Context.frame_cluster) against its CPU twin
(tests/framecluster_twin.py, the C form) for exact equality, cluster for cluster, on the cases of tests/framecluster_cases.py --
degenerate inputs, the row and length limits and the 64 lanes of a wavefront, uneven lengths, odd byte offsets, every threshold
at its edge, the order rules, the recurrence, the strands, closed forms, thousands of small groups in one call and in many batches
(a fresh process), refused arguments."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import framecluster_cases as FC
import framecluster_twin as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    import hite_amd

    c = hite_amd.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _many():
    """the small groups and their twin result, computed once"""
    groups = FC.many_small()
    return groups, T.frame_cluster(groups, **FC.SORT)


def _same(ctx, cases):
    for label, groups, kw in cases:
        exp = T.frame_cluster(groups, **kw)
        got = ctx.frame_cluster(groups, **kw)
        bad = [g for g in range(len(groups)) if got[g] != exp[g]]
        assert len(got) == len(exp) and not bad, (label, bad[:5], got[bad[0]] if bad else None, exp[bad[0]] if bad else None)
        if label in FC.EXPECT:
            assert got == FC.EXPECT[label], label


def test_limits_in_the_header():
    txt = open(os.path.join(ROOT, "include", "hite_gpu.h")).read()
    assert "#define HITE_FRAMECLUSTER_MAX_ROWS %d\n" % FC.MAX_ROWS in txt and "#define HITE_FRAMECLUSTER_MAX_LEN  %d\n" % FC.MAX_LEN in txt


def test_degenerate(ctx):
    _same(ctx, FC.degenerate())


def test_row_edges(ctx):
    _same(ctx, FC.row_edges())
    _label, groups, kw = FC.row_edges()[-1]
    got = ctx.frame_cluster(groups, **kw)
    assert got[1] is None and got[0] and got[2]


def test_length_edges_uneven_lengths_and_odd_offsets(ctx):
    _same(ctx, FC.length_edges())


def test_thresholds_at_their_edges(ctx):
    _same(ctx, FC.thresholds())


def test_rule_order(ctx):
    _same(ctx, FC.rule_order())


def test_recurrence(ctx):
    _same(ctx, FC.recurrence())


def test_strands(ctx):
    _same(ctx, FC.strands())


def test_closed_forms(ctx):
    for label, groups, kw in FC.closed_forms():
        assert ctx.frame_cluster(groups, **kw) == FC.EXPECT[label], label


def test_every_case_in_one_call_per_option_set(ctx):
    """the groups of all cases that share their options, side by side in one call: groups of a unit do not see each other"""
    by_kw = {}
    for label, groups, kw in FC.all_cases():
        by_kw.setdefault(json.dumps(kw, sort_keys=True), []).extend(groups)
    for key, groups in by_kw.items():
        kw = json.loads(key)
        assert ctx.frame_cluster(groups, **kw) == T.frame_cluster(groups, **kw), key


def test_many_small_groups(ctx):
    groups, exp = _many()
    assert ctx.frame_cluster(groups, **FC.SORT) == exp
    joined = [[a + b for a, b in zip(g, reversed(g))] for g in groups[:1000]]
    assert ctx.frame_cluster(joined, **FC.JOINED) == T.frame_cluster(joined, **FC.JOINED)


def test_small_batches_in_a_fresh_process(ctx, tmp_path):
    """HITE_FRAMECLUSTER_BATCH_BYTES is read when a context is created: the child sends the same groups up in batches of 4 096 bytes"""
    out = tmp_path / "child.json"
    env = dict(os.environ, HITE_FRAMECLUSTER_BATCH_BYTES="4096")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_framecluster_child.py"), str(out)], check=True, env=env, timeout=300)
    res = json.load(open(out))
    groups, exp = _many()
    assert res["many"] == exp
    for label, groups, kw in FC.row_edges() + FC.length_edges():
        assert res[label] == T.frame_cluster(groups, **kw), label


def test_refused_arguments(ctx):
    import hite_amd

    groups, kw = [["ACGTACGTACGTACGTACGTACGT", "ACGTACGTACGTACGTACGTACGA"]], FC.kw()
    nan = float("nan")
    for bad in (dict(ident=nan), dict(ident=-0.1), dict(ident=1.5), dict(cov_short=nan), dict(cov_short=1.01), dict(cov_long=-1.0),
                dict(cov_long=nan), dict(min_cov=-1), dict(min_len=-1)):
        with pytest.raises(hite_amd.HiteError, match=r"hite_frame_cluster failed: -1\b"):
            ctx.frame_cluster(groups, **dict(kw, **bad))
        assert ctx.frame_cluster(groups, **kw) == [[[0, 1]]]
    lib, h = ctx.lib, ctx.h
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    roff, soff = np.array([0, 2], dtype=np.int64), np.array([0, 24, 48], dtype=np.int64)
    buf = np.frombuffer("".join(groups[0]).encode() + b"\0" * 16, dtype=np.uint8)
    cl, ncl = np.zeros(3, dtype=np.int32), np.zeros(2, dtype=np.int32)

    def call(n=1, roff=roff, buf=buf, soff=soff, cl=cl, ncl=ncl):
        return lib.hite_frame_cluster(h, C.c_int64(n), None if roff is None else p(roff), None if buf is None else p(buf),
                                      None if soff is None else p(soff), C.c_double(0.8), C.c_double(0.3), C.c_double(0.0), C.c_int32(20),
                                      C.c_int32(10), C.c_int32(1), None if cl is None else p(cl), None if ncl is None else p(ncl))

    assert call(n=-1) == -1
    assert call(roff=None) == -1 and call(buf=None) == -1 and call(soff=None) == -1 and call(cl=None) == -1 and call(ncl=None) == -1
    assert call(roff=np.array([2, 0], dtype=np.int64)) == -1 and call(roff=np.array([-1, 2], dtype=np.int64)) == -1
    assert call(soff=np.array([0, 48, 24], dtype=np.int64)) == -1
    assert call(n=0, roff=None, buf=None, soff=None, cl=None, ncl=None) == 0
    assert call() == 0 and cl[:2].tolist() == [0, 0] and ncl[0] == 1
    assert ctx.frame_cluster(groups, **kw) == [[[0, 1]]]
