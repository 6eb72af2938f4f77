"""GPU: hite_pair_hsps (hite_amd/csrc/hite_pairhsp.hip; Context.pair_hsps) against its CPU twin (tests/pairhsp_twin.py, the C form)
for exact equality, record for record, on the cases of tests/pairhsp_cases.py -- the lengths around the 64 columns of a strip, the
word and window rules at their edges, diag_min, bytes outside ACGT, alignments at and across the edges of their band, the
rectangles before and after a first HSP, ties, two pairs at production size, refused pairs, thousands of pairs in one call and in
many batches (a fresh process), the empty batch and a record buffer that is too small."""
import ctypes as C
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pairhsp_cases as PC
import pairhsp_twin as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    import hite_amd

    c = hite_amd.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _mixed():
    """the mixed pairs and their twin result, computed once"""
    seqs, pairs = PC.mixed()
    return seqs, pairs, T.pair_hsps(seqs, pairs)


def _same(ctx, cases, min_hsps=1):
    exp = PC.run(T.pair_hsps, cases)
    got = PC.run(ctx.pair_hsps, cases)
    bad = [k for k in range(len(cases)) if got[k] != exp[k]]
    assert not bad, (len(bad), cases[bad[0]][0], got[bad[0]], exp[bad[0]])
    assert sum(len(e) for e in exp) >= min_hsps


def test_constants_in_the_header():
    txt = open(os.path.join(ROOT, "include", "hite_gpu.h")).read()
    for name, v in (("MAX_LEN", T.MAX_LEN), ("WORD", T.WORD), ("MAX_OCC", T.MAX_OCC), ("BIN_SHIFT", T.BIN_SHIFT), ("MIN_VOTES", T.MIN_VOTES),
                    ("MAX_WINDOWS", T.MAX_WINDOWS), ("BAND_BELOW", T.BAND_BELOW), ("BAND_ABOVE", T.BAND_ABOVE), ("MATCH", T.MATCH),
                    ("MISMATCH", "(%d)" % T.MISMATCH), ("GAP", "(%d)" % T.GAP), ("MIN_SCORE", T.MIN_SCORE), ("MIN_RECT", T.MIN_RECT),
                    ("MAX_HSPS", T.MAX_HSPS)):
        assert re.search(r"^#define HITE_PAIRHSP_%s +%s$" % (name, re.escape(str(v))), txt, re.M), name


def test_closed_forms(ctx):
    forms = PC.closed_forms()
    got = PC.run(ctx.pair_hsps, [f[:4] for f in forms])
    for (label, q, s, dm, recs), g in zip(forms, got):
        assert g == recs, (label, g)


def test_lengths_crossed_over_the_strip_edges(ctx):
    _same(ctx, PC.length_grid(), 100)


def test_word_and_window_rules(ctx):
    _same(ctx, PC.word_and_window_rules(), 40)


def test_diag_min(ctx):
    _same(ctx, PC.diag_min_cases(), 10)


def test_bytes_outside_acgt_and_lower_case(ctx):
    _same(ctx, PC.bytes_cases(), 3)


def test_band_edges_and_drift(ctx):
    _same(ctx, PC.band_edges(), 48)


def test_ties(ctx):
    _same(ctx, PC.ties(), 10)


def test_rectangles_before_and_after(ctx):
    _same(ctx, PC.rectangles(), 20)


def test_production_sizes(ctx):
    _same(ctx, PC.production(), 3)


def test_refused_pairs(ctx):
    seqs, pairs, ok = PC.refused()
    got = ctx.pair_hsps(seqs, pairs)
    assert [g is not None for g in got] == ok
    assert got == T.pair_hsps(seqs, pairs)


def test_many_pairs_in_one_call(ctx):
    seqs, pairs, exp = _mixed()
    assert ctx.pair_hsps(seqs, pairs) == exp
    assert ctx.pair_hsps(seqs, pairs, diag_min=-5) == T.pair_hsps(seqs, pairs, -5)


def test_small_batches_in_a_fresh_process(ctx, tmp_path):
    """HITE_PAIRHSP_BATCH_PAIRS is read when a context is created: the child sends the same pairs up 257 at a time"""
    out = tmp_path / "child.json"
    env = dict(os.environ, HITE_PAIRHSP_BATCH_PAIRS="257")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_pairhsp_child.py"), str(out)], check=True, env=env, timeout=300)
    res = json.load(open(out))
    seqs, pairs, exp = _mixed()
    assert [None if r is None else [tuple(h) for h in r] for r in res["mixed"]] == exp
    assert ctx.pair_hsps(seqs, pairs) == exp


def test_empty_batch_and_capacity(ctx):
    assert ctx.pair_hsps([], []) == [] and ctx.pair_hsps(["ACGT"], []) == []
    lib, h = ctx.lib, ctx.h
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    cases = PC.word_and_window_rules()[:12]
    seqs, pairs = [], []
    for _label, q, s, _dm in cases:
        seqs += [q, s]
        pairs.append((len(seqs) - 2, 0, len(q), len(seqs) - 1, 0, len(s)))
    exp = T.pair_hsps(seqs, pairs)
    need = sum(len(e) for e in exp)
    assert need >= 8
    buf, off, n, cols = T.pack_args(seqs, pairs)
    status, first = np.zeros(n, dtype=np.int32), np.zeros(n + 1, dtype=np.int64)

    def call(cap, n_pair=n):
        recs, n_out = np.full((max(cap, 1) + 1, 7), -7, dtype=np.int32), C.c_int64(-1)
        rc = lib.hite_pair_hsps(h, C.c_int64(len(off) - 1), p(buf), p(off), C.c_int64(n_pair), *[p(c) for c in cols], C.c_int32(T.NO_DIAG_MIN),
                                C.c_int64(cap), p(status), p(first), p(recs), C.byref(n_out))
        return rc, n_out.value, recs

    rc, n_out, recs = call(need - 3)
    assert rc == -4 and n_out == need and (recs[need - 3:] == -7).all()       # HITE_ECAP with the need; nothing past cap is written
    assert status.tolist() == [len(e) for e in exp] and first.tolist() == np.cumsum([0] + [len(e) for e in exp]).tolist()
    rc, n_out, recs = call(0)
    assert rc == -4 and n_out == need
    rc, n_out, recs = call(need)
    assert rc == 0 and n_out == need and T.unpack(n, status, first, recs) == exp
    rc, n_out, _ = call(need, n_pair=0)
    assert rc == 0 and n_out == 0
    assert lib.hite_pair_hsps(h, C.c_int64(0), None, None, C.c_int64(0), None, None, None, None, None, None, C.c_int32(0), C.c_int64(0), None,
                              None, None, None) == 0
    assert call(-1)[0] == -1 and call(need, n_pair=-1)[0] == -1
    assert ctx.pair_hsps(seqs, pairs) == exp
