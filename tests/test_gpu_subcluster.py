"""GPU: hite_msa_subcluster (hite_amd/csrc/hite_subcluster.hip; Context.msa_subcluster) against its CPU twin
(tests/subcluster_twin.py) for exact equality on the cases of tests/subcluster_cases.py -- degenerate shapes, column tails and
unaligned starts, the threshold, the order rules, leader counts around the chunk size, chunk boundaries (default chunk and, in a
fresh process, chunks of 8 rows), byte values, a batch of size, the cutoffs, refused arguments -- and the switch of the host layer
(util._generate_cons_batch, generate_cons_v1) against the default route."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import subcluster_cases as SC
import subcluster_twin as T
from conftest import load_golden

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    import hite_amd

    c = hite_amd.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _families():
    """the 300 random family alignments and their twin results per cutoff, computed once"""
    als = SC.family_batch()
    return als, {c: [T.subcluster(al, c) for al in als] for c in (0.0, 0.2, 0.5, 1.0)}


def _same(ctx, cases):
    for label, als, cutoff in cases:
        exp = [T.subcluster(al, cutoff) for al in als]
        got = ctx.msa_subcluster(als, cutoff)
        bad = [k for k in range(len(als)) if got[k] != exp[k]]
        assert len(got) == len(exp) and not bad, (label, bad[:5], got[bad[0]][:4] if bad else None, exp[bad[0]][:4] if bad else None)


def test_chunk_constant():
    from hite_amd import _lib

    txt = open(os.path.join(ROOT, "include", "hite_gpu.h")).read()
    assert "#define HITE_SUBCLUSTER_CHUNK %d\n" % SC.CHUNK in txt and _lib.HITE_SUBCLUSTER_CHUNK == SC.CHUNK


def test_degenerate(ctx):
    _same(ctx, SC.degenerate())
    for label, als, cutoff in SC.degenerate():
        assert ctx.msa_subcluster(als, cutoff) == SC.DEGENERATE_EXPECT[label], label


def test_column_tails_and_unaligned_starts(ctx):
    (label, als, cutoff), = SC.tails()
    assert sum(1 for k in range(len(als)) if sum(a.size for a in als[:k]) % 16) >= 14      # most start off a 16-byte boundary
    _same(ctx, [(label, als, cutoff)])
    _same(ctx, [(label + "-reversed", als[::-1], cutoff)])


def test_threshold(ctx):
    _same(ctx, SC.threshold())
    (_label, als, cutoff), = SC.threshold()
    assert ctx.msa_subcluster(als, cutoff) == [[[0, 1], [2]]] * len(SC.THRESHOLD_N)


def test_order(ctx):
    _same(ctx, SC.order())
    for label, als, cutoff in SC.order():
        assert ctx.msa_subcluster(als, cutoff) == SC.ORDER_EXPECT[label], label
    # the seven of them as one batch
    assert ctx.msa_subcluster([als[0] for _l, als, _c in SC.order()], 0.2) == [SC.ORDER_EXPECT[l][0] for l, _a, _c in SC.order()]


def test_leader_counts(ctx):
    _same(ctx, SC.leader_counts())


def test_chunk_boundaries_at_the_default_chunk(ctx):
    _same(ctx, SC.chunk_boundary())


def test_small_chunks_in_a_fresh_process(ctx, tmp_path):
    import _subcluster_child as child

    out = tmp_path / "child.json"
    env = dict(os.environ, HITE_SUBCLUSTER_CHUNK_ROWS="8")
    env.pop("HITE_SUBCLUSTER_BATCH_BYTES", None)
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_subcluster_child.py"), str(out)], check=True, env=env, timeout=300)
    res = json.loads(out.read_text())
    fam_als, fam_exp = _families()
    assert sum(1 for al in fam_als if al.shape[0] > 8) > 200
    for label, als, cutoff in child.cases():
        exp = fam_exp[cutoff] if label == "families" else [T.subcluster(al, cutoff) for al in als]
        assert res["chunk"][label] == exp, label
        assert res["batches"][label] == exp, label
        assert ctx.msa_subcluster(als, cutoff) == exp, label           # the default run


def test_bytes(ctx):
    _same(ctx, SC.byte_values())
    (label, als, cutoff), = SC.byte_values()
    assert ctx.msa_subcluster(als, cutoff) == SC.BYTES_EXPECT[label]


def test_size(ctx):
    (label, als, cutoff), = SC.size_batch()
    exp = [T.subcluster(al, cutoff) for al in als]
    assert len(exp[0]) == 600 and len(exp[1]) == 6
    assert ctx.msa_subcluster(als, cutoff) == exp


@pytest.mark.parametrize("cutoff", [0.0, 0.2, 0.5, 1.0])
def test_cutoffs(ctx, cutoff):
    als, exp = _families()
    assert ctx.msa_subcluster(als, cutoff) == exp[cutoff]


def test_refused_arguments_leave_the_context_usable(ctx):
    import hite_amd

    al = [b"ACGTACGTAC", b"ACGTACGTAC", b"TTTTTTTTTT"]
    for cutoff in (float("nan"), -0.1, 1.5):
        with pytest.raises(hite_amd.HiteError, match=r"hite_msa_subcluster failed: -1\b"):
            ctx.msa_subcluster([al], cutoff)
        assert ctx.msa_subcluster([al], 0.2) == [[[0, 1], [2]]]
    with pytest.raises(hite_amd.HiteError, match=r"hite_msa_subcluster failed: -1\b"):
        ctx.msa_subcluster([al, np.full((2, 65536), 65, dtype=np.uint8)], 0.2)
    assert ctx.msa_subcluster([al, np.full((2, 65535), 65, dtype=np.uint8)], 0.2) == [[[0, 1], [2]], [[0, 1]]]
    with pytest.raises(ValueError):
        ctx.msa_subcluster([[b"ACGT", b"ACG"]], 0.2)


# ---- the host layer ------------------------------------------------------------------------------------------------------------
def test_generate_cons_batch_switch(ctx, tmp_path, monkeypatch):
    from hite_amd import util

    monkeypatch.delenv("HITE_SUBCLUSTER", raising=False)
    batch = SC.cons_clusters()
    off = util._generate_cons_batch(ctx, batch)
    assert sum(len(d) for d in off[:3]) >= 6 and "c1_short" in off[1] and off[3] == dict(batch[3])
    assert util._generate_cons_batch(ctx, batch, subcluster="gpu") == off
    # ... and through generate_cons_v1 with the environment's switch
    util._CTX = ctx
    for ci, cl in enumerate(batch):
        fa = tmp_path / ("cl%d.fa" % ci)
        fa.write_text("".join(">%s\n%s\n" % r for r in cl))
        monkeypatch.delenv("HITE_SUBCLUSTER", raising=False)
        exp = util.generate_cons_v1(ci, str(fa), str(tmp_path), 1)
        assert exp == off[ci]
        monkeypatch.setenv("HITE_SUBCLUSTER", "gpu")
        assert util.generate_cons_v1(ci, str(fa), str(tmp_path), 1) == exp


def test_cons_v1_golden_with_the_switch_on(ctx, tmp_path, monkeypatch):
    """a caller's Ninja clusters override the switch: the reference's results stay"""
    from hite_amd import util

    util._CTX = ctx
    monkeypatch.setenv("HITE_SUBCLUSTER", "gpu")
    for ci, c in enumerate(load_golden("cons_v1")):
        fa = tmp_path / ("cl%d.fa" % ci)
        fa.write_text("".join(">%s\n%s\n" % (n, s) for n, s in zip(c["names"], c["seqs"])))
        ninja = {int(k): v for k, v in c["ninja"].items()}
        assert util.generate_cons_v1(0, str(fa), str(tmp_path), 1, ninja_clusters=ninja) == c["expected"], ci
