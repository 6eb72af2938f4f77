"""GPU: hite_ltr_scan (hite_amd/csrc/hite_ltrscan.hip; Context.ltr_scan) against its CPU twin (tests/ltrscan_twin.py, the C form) for
exact equality, record for record in order and counter for counter: every small case of tests/ltrscan_cases.py and its closed form,
the genome of 32 planted elements, one random sequence of 5 Mbp with 40 planted elements (more elements than RS_WIDE_MIN: the wide
form of the sort) in one batch and, cut into pieces, in several batches of a context made in a fresh process (the narrow form), a
record buffer that is too small, every refused argument and the empty call."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ltrscan_cases as LC
import ltrscan_twin as LT

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIECES = 6
ECAP, EINVAL = -4, -1


@pytest.fixture(scope="module")
def ctx():
    import hite_amd

    c = hite_amd.Context(0)
    yield c
    c.close()


def _scan(ctx, seqs, **kw):
    st = {}
    return [tuple(r) for r in ctx.ltr_scan(seqs, stats=st, **kw).tolist()], st


@functools.lru_cache(maxsize=None)
def _volume_twin(pieces):
    """the twin's result on the volume genome, whole (pieces = 1) or cut, computed once"""
    seq, cuts = LC.volume()
    st = {}
    return LT.scan([seq] if pieces == 1 else LC.split(seq, cuts, pieces), stats=st), st


def test_every_small_case(ctx):
    n = 0
    for c in LC.small_cases():
        st = {}
        exp = LT.scan(c["seqs"], stats=st, **c["kw"])
        got, st_g = _scan(ctx, c["seqs"], **c["kw"])
        assert got == exp, (c["label"], got, exp)
        assert st_g == st, (c["label"], st_g, st)
        if c["records"] is not None:
            assert got == c["records"], c["label"]
        n += len(exp)
    assert len(LC.small_cases()) >= 60 and n >= 40


def test_planted_genome(ctx):
    names, seqs, truth, places = LC.planted()
    st = {}
    exp = LT.scan(seqs, stats=st)
    got, st_g = _scan(ctx, seqs)
    assert got == exp and st_g == st
    assert not [p for p in places if p not in {r[:5] for r in got}] and len(places) == 32


def test_volume_in_one_batch(ctx):
    seq, _cuts = LC.volume()
    assert len(seq) == 5_000_000 > 1 << 22
    exp, st = _volume_twin(1)
    got, st_g = _scan(ctx, [seq])
    assert got == exp and st_g == st
    assert len(got) >= 38 and st["words"] > 1 << 22


def test_volume_in_small_batches_in_a_fresh_process(ctx, tmp_path):
    """HITE_LTRSCAN_BATCH_BYTES is read when a context is created: the child sends the pieces up one batch each"""
    seq, cuts = LC.volume()
    pieces = LC.split(seq, cuts, PIECES)
    assert len(pieces) == PIECES and b"".join(pieces) == seq and max(len(p) for p in pieces) < 1 << 22
    exp, st = _volume_twin(PIECES)
    assert len(exp) == len(_volume_twin(1)[0])        # the cuts lie between the elements
    out = tmp_path / "child.json"
    env = dict(os.environ, HITE_LTRSCAN_BATCH_BYTES=str(max(len(p) for p in pieces)))       # >= 3 batches: no two pieces fit one
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_ltrscan_child.py"), str(out), str(PIECES)], check=True, env=env, timeout=300)
    res = json.load(open(out))
    assert [tuple(r) for r in res["records"]] == exp and res["stats"] == st
    got, st_g = _scan(ctx, pieces)                     # the same pieces in one batch of this context
    assert got == exp and st_g == st


def _raw(ctx, seqs, cap, kw=None, n=None, with_stats=True, off=None):
    kw = dict(LT.DEFAULTS, **(kw or {}))
    buf, o = ctx._csr(seqs)
    o = o if off is None else np.asarray(off, dtype=np.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    recs, n_out, st = np.full((max(cap, 0) + 2, 8), -7, dtype=np.int32), C.c_int64(-1), np.full(len(LT.STATS), -1, dtype=np.int64)
    rc = ctx.lib.hite_ltr_scan(ctx.h, C.c_int64(len(o) - 1 if n is None else n), p(buf), p(o), C.c_int32(kw["min_len"]), C.c_int32(kw["max_len"]),
                               C.c_int32(kw["min_ltr"]), C.c_int32(kw["max_ltr"]), C.c_int32(kw["identity"]), C.c_int64(cap), p(recs),
                               C.byref(n_out), p(st) if with_stats else None)
    return rc, n_out.value, recs, st


def test_capacity(ctx):
    names, seqs, truth, places = LC.planted()
    exp = LT.scan(seqs)
    need = len(exp)
    assert need == 41
    rc, n_out, recs, st = _raw(ctx, seqs, need - 5)
    assert rc == ECAP and n_out == need and st[-1] == need
    assert [tuple(r) for r in recs[:need - 5].tolist()] == exp[:need - 5] and (recs[need - 5:] == -7).all()      # nothing past cap is written
    rc, n_out, recs, _ = _raw(ctx, seqs, 0)
    assert rc == ECAP and n_out == need and (recs == -7).all()
    rc, n_out, recs, _ = _raw(ctx, seqs, need, with_stats=False)
    assert rc == 0 and n_out == need and [tuple(r) for r in recs[:need].tolist()] == exp
    # the binding asks again with the room reported
    assert [tuple(r) for r in ctx.ltr_scan(seqs, cap=3).tolist()] == exp
    assert [tuple(r) for r in ctx.ltr_scan(seqs, cap=0).tolist()] == exp


def test_refused_arguments(ctx):
    seqs = ["ACGT" * 50]
    assert _raw(ctx, seqs, 4)[0] == 0
    for bad in (dict(max_ltr=8193), dict(min_ltr=0), dict(min_ltr=-5), dict(min_ltr=6001), dict(min_len=22001), dict(max_len=399), dict(identity=0),
                dict(identity=101), dict(identity=-1)):
        rc, n_out, recs, _ = _raw(ctx, seqs, 4, bad)
        assert rc == EINVAL and (recs == -7).all(), bad
        with pytest.raises(Exception):
            ctx.ltr_scan(seqs, **bad)
    assert _raw(ctx, seqs, 4, dict(max_ltr=8192))[0] == 0 and _raw(ctx, seqs, 4, dict(min_ltr=6000))[0] == 0
    assert _raw(ctx, seqs, 4, dict(min_len=22000))[0] == 0 and _raw(ctx, seqs, 4, dict(identity=100))[0] == 0
    assert _raw(ctx, seqs, -1)[0] == EINVAL and _raw(ctx, seqs, 4, n=-1)[0] == EINVAL
    assert _raw(ctx, seqs, 4, off=[0, 2 ** 31])[0] == EINVAL            # a sequence of 2^31 bytes (refused before a byte is read)
    assert _raw(ctx, seqs + seqs, 4, off=[0, 200, 100])[0] == EINVAL     # descending offsets
    lib, h = ctx.lib, ctx.h
    n_out = C.c_int64(0)
    off = np.array([0, 200], dtype=np.int64)
    recs = np.zeros((4, 8), dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    args = [C.c_int32(v) for v in (400, 22000, 100, 6000, 85)]
    assert lib.hite_ltr_scan(h, C.c_int64(1), None, p(off), *args, C.c_int64(4), p(recs), C.byref(n_out), None) == EINVAL       # no bytes
    assert lib.hite_ltr_scan(h, C.c_int64(1), p(ctx._csr(seqs)[0]), None, *args, C.c_int64(4), p(recs), C.byref(n_out), None) == EINVAL
    assert lib.hite_ltr_scan(h, C.c_int64(1), p(ctx._csr(seqs)[0]), p(off), *args, C.c_int64(4), None, C.byref(n_out), None) == EINVAL
    assert lib.hite_ltr_scan(h, C.c_int64(1), p(ctx._csr(seqs)[0]), p(off), *args, C.c_int64(4), p(recs), None, None) == EINVAL
    assert lib.hite_ltr_scan(None, C.c_int64(1), p(ctx._csr(seqs)[0]), p(off), *args, C.c_int64(4), p(recs), C.byref(n_out), None) == EINVAL


def test_empty_calls(ctx):
    n_out, st = C.c_int64(-1), np.full(len(LT.STATS), -1, dtype=np.int64)
    args = [C.c_int32(v) for v in (400, 22000, 100, 6000, 85)]
    assert ctx.lib.hite_ltr_scan(ctx.h, C.c_int64(0), None, None, *args, C.c_int64(0), None, C.byref(n_out), st.ctypes.data_as(C.c_void_p)) == 0
    assert n_out.value == 0 and (st == 0).all()
    for seqs in ([], [""], ["", "ACGT", ""], ["ACGTACGTACGT"], ["N" * 500], ["ACGTTGCAAGCTA"]):
        got, st_g = _scan(ctx, seqs)
        assert got == [] and st_g["words"] == (1 if seqs == ["ACGTTGCAAGCTA"] else 0) and st_g["hits"] == 0
    assert ctx.ltr_scan([]).shape == (0, 8) and ctx.ltr_scan([]).dtype == np.int32
