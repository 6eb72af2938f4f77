"""GPU: hite_annotate (hite_amd/csrc/hite_annotate.hip; Context.annotate) against its CPU twin (tests/annotate_twin.py, the C form) for
exact equality, record for record in order and counter for counter: every case of tests/annotate_cases.py, the same in a fresh context
whose HITE_ANNOT_BATCH_BYTES forces several batches, a slice of the planted genome cut into pieces that share batches, the planted
genome of 2 Mbp with its recall bar, a record buffer that is too small, every refused argument and the empty calls."""
import ctypes as C
import functools

import numpy as np
import pytest

import annotate_cases as AC
import annotate_twin as AT

pytestmark = pytest.mark.gpu
ECAP, EINVAL = -4, -1
CASES = AC.small_cases()


@pytest.fixture(scope="module")
def ctx():
    import hite_amd

    c = hite_amd.Context(0)
    yield c
    c.close()


def _annotate(ctx, seqs, lib, piece_len=0, **kw):
    st = {}
    recs, status = ctx.annotate(seqs, lib, piece_len, stats=st, **kw)
    assert recs.dtype == np.int32 and recs.shape[1:] == (10,) and status.dtype == np.int8 and len(status) == len(lib)
    return [tuple(r) for r in recs.tolist()], status.tolist(), st


@functools.lru_cache(maxsize=None)
def _twin(k):
    c = CASES[k]
    st = {}
    recs, status = AT.annotate(c["seqs"], c["lib"], c["piece_len"], stats=st)
    return recs, status, st


@functools.lru_cache(maxsize=None)
def _slice():
    """the first 300 000 bases of the planted genome with pieces of 65 536 (+ the overlap): five pieces, the twin's result"""
    genome, lib, _truth = AC.planted()
    seqs = [genome[:300_000], genome[300_000:340_000]]
    st = {}
    recs, status = AT.annotate(seqs, lib, 65536, stats=st)
    st0 = {}
    recs0, status0 = AT.annotate(seqs, lib, 0, stats=st0)
    return seqs, lib, (recs, status, st), (recs0, status0, st0)


def test_every_case(ctx):
    n = 0
    for k, c in enumerate(CASES):
        got = _annotate(ctx, c["seqs"], c["lib"], c["piece_len"])
        assert got == _twin(k), (c["label"], got, _twin(k))
        if c["records"] is not None:
            assert got[0] == c["records"], c["label"]
        n += len(got[0])
    assert len(CASES) >= 30 and n == sum(len(_twin(k)[0]) for k in range(len(CASES))) >= 25


def test_every_case_in_small_batches_of_a_fresh_context(monkeypatch):
    """HITE_ANNOT_BATCH_BYTES is read when a context is created; 6 000 bytes: no two pieces of a case share a batch but the short ones"""
    import hite_amd

    monkeypatch.setenv("HITE_ANNOT_BATCH_BYTES", "6000")
    c2 = hite_amd.Context(0)
    try:
        for k, c in enumerate(CASES):
            assert _annotate(c2, c["seqs"], c["lib"], c["piece_len"]) == _twin(k), c["label"]
        monkeypatch.setenv("HITE_ANNOT_BATCH_BYTES", "200000")
        seqs, lib, exp, _whole = _slice()
        c3 = hite_amd.Context(0)
        try:
            assert _annotate(c3, seqs, lib, 65536) == exp      # pieces of 131 072 + margins, one to a batch; the last two together
        finally:
            c3.close()
    finally:
        c2.close()


def test_pieces_that_share_a_batch(ctx):
    seqs, lib, exp, whole = _slice()
    assert AT.pieces(300_000, 65536) == [(0, 131072), (65536, 196608), (131072, 262144), (196608, 300000), (262144, 300000)]
    assert _annotate(ctx, seqs, lib, 65536) == exp
    assert exp[2]["duplicates"] > exp[2]["records"] > 30      # every copy is found by two lattices and most by two pieces
    assert _annotate(ctx, seqs, lib) == whole
    assert whole[0] == exp[0] and whole[2]["hits"] < exp[2]["hits"]      # on this input the pieces change the hits and not the records


def test_planted_genome(ctx):
    genome, lib, truth = AC.planted()
    exp = AC.planted_twin()
    low = [r for r in truth if r[4] <= 0.10]
    # the bar is a condition on the input: the twin alone meets it (tests/test_annotate_cases.py checks the same without a GPU)
    assert len(low) == 240 and all(10 * AC.coverage(r, exp[0]) >= 9 * (r[3] - r[2]) for r in low)
    got = _annotate(ctx, [genome], lib)
    assert got == exp
    for row in low:
        assert 10 * AC.coverage(row, got[0]) >= 9 * (row[3] - row[2]), row
    assert got[2]["hits"] > 400_000 and got[2]["runs"] > 1000


def _raw(ctx, seqs, lib, cap, piece_len=0, n_seq=None, n_lib=None, off=None, loff=None, with_stats=True, with_status=True):
    buf, o = ctx._csr(seqs)
    lbuf, lo = ctx._csr(lib)
    o = o if off is None else np.asarray(off, dtype=np.int64)
    lo = lo if loff is None else np.asarray(loff, dtype=np.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    recs, n_out = np.full((max(cap, 0) + 2, 10), -7, dtype=np.int32), C.c_int64(-1)
    st, status = np.full(len(AT.STATS), -1, dtype=np.int64), np.full(len(lo) + 1, 9, dtype=np.int8)
    rc = ctx.lib.hite_annotate(ctx.h, C.c_int64(len(o) - 1 if n_seq is None else n_seq), p(buf), p(o), C.c_int32(len(lo) - 1 if n_lib is None else n_lib),
                               p(lbuf), p(lo), C.c_int32(piece_len), C.c_int64(cap), p(recs), C.byref(n_out), p(status) if with_status else None,
                               p(st) if with_stats else None)
    return rc, n_out.value, recs, st, status


def test_capacity(ctx):
    c = [c for c in CASES if c["label"] == "copies in three sequences"][0]
    exp = c["records"]
    rc, n_out, recs, st, status = _raw(ctx, c["seqs"], c["lib"], 3)
    assert rc == ECAP and n_out == 4 and st[-1] == 4 and status[:2].tolist() == [0, 0] and status[2] == 9
    assert [tuple(r) for r in recs[:3].tolist()] == exp[:3] and (recs[3:] == -7).all()      # nothing past cap is written
    rc, n_out, recs, _, _ = _raw(ctx, c["seqs"], c["lib"], 0)
    assert rc == ECAP and n_out == 4 and (recs == -7).all()
    rc, n_out, recs, _, _ = _raw(ctx, c["seqs"], c["lib"], 4, with_stats=False, with_status=False)
    assert rc == 0 and n_out == 4 and [tuple(r) for r in recs[:4].tolist()] == exp
    # the binding asks again with the room reported
    assert _annotate(ctx, c["seqs"], c["lib"], cap=1)[0] == exp and _annotate(ctx, c["seqs"], c["lib"], cap=0)[0] == exp


def test_refused_arguments(ctx):
    seqs, lib = ["ACGT" * 50], ["ACGTTGCA" * 10]
    assert _raw(ctx, seqs, lib, 4)[0] == 0
    for pl in (AT.MIN_PIECE - 1, AT.PIECE + 1, -1):
        rc, _n, recs, _st, _s = _raw(ctx, seqs, lib, 4, piece_len=pl)
        assert rc == EINVAL and (recs == -7).all(), pl
        with pytest.raises(Exception):
            ctx.annotate(seqs, lib, pl)
    assert _raw(ctx, seqs, lib, 4, piece_len=AT.MIN_PIECE)[0] == 0 and _raw(ctx, seqs, lib, 4, piece_len=AT.PIECE)[0] == 0
    assert _raw(ctx, seqs, lib, -1)[0] == EINVAL and _raw(ctx, seqs, lib, 4, n_seq=-1)[0] == EINVAL and _raw(ctx, seqs, lib, 4, n_lib=-1)[0] == EINVAL
    assert _raw(ctx, seqs, lib, 4, n_lib=AT.MAX_LIB + 1, loff=[0] * (AT.MAX_LIB + 2))[0] == EINVAL
    assert _raw(ctx, seqs, [""] * AT.MAX_LIB, 4)[0] == 0                                     # 32 768 entries are allowed
    assert _raw(ctx, seqs, lib, 4, off=[0, 2 ** 31])[0] == EINVAL                            # a sequence of 2^31 bytes (refused before a byte is read)
    assert _raw(ctx, seqs + seqs, lib, 4, off=[0, 200, 100])[0] == EINVAL                    # descending offsets
    assert _raw(ctx, seqs, lib + lib, 4, loff=[0, 80, 40])[0] == EINVAL
    h, f = ctx.h, ctx.lib.hite_annotate
    n_out = C.c_int64(0)
    off, loff = np.array([0, 200], dtype=np.int64), np.array([0, 80], dtype=np.int64)
    recs = np.zeros((4, 10), dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    sb, lb = ctx._csr(seqs)[0], ctx._csr(lib)[0]
    one, zero, four = C.c_int64(1), C.c_int32(0), C.c_int64(4)
    assert f(h, one, None, p(off), C.c_int32(1), p(lb), p(loff), zero, four, p(recs), C.byref(n_out), None, None) == EINVAL       # no bytes
    assert f(h, one, p(sb), None, C.c_int32(1), p(lb), p(loff), zero, four, p(recs), C.byref(n_out), None, None) == EINVAL
    assert f(h, one, p(sb), p(off), C.c_int32(1), None, p(loff), zero, four, p(recs), C.byref(n_out), None, None) == EINVAL
    assert f(h, one, p(sb), p(off), C.c_int32(1), p(lb), None, zero, four, p(recs), C.byref(n_out), None, None) == EINVAL
    assert f(h, one, p(sb), p(off), C.c_int32(1), p(lb), p(loff), zero, four, None, C.byref(n_out), None, None) == EINVAL
    assert f(h, one, p(sb), p(off), C.c_int32(1), p(lb), p(loff), zero, four, p(recs), None, None, None) == EINVAL
    assert f(None, one, p(sb), p(off), C.c_int32(1), p(lb), p(loff), zero, four, p(recs), C.byref(n_out), None, None) == EINVAL
    assert f(h, one, p(sb), p(off), C.c_int32(1), p(lb), p(loff), zero, four, p(recs), C.byref(n_out), None, None) == 0


def test_empty_calls(ctx):
    n_out, st = C.c_int64(-1), np.full(len(AT.STATS), -1, dtype=np.int64)
    f = ctx.lib.hite_annotate
    assert f(ctx.h, C.c_int64(0), None, None, C.c_int32(0), None, None, C.c_int32(0), C.c_int64(0), None, C.byref(n_out), None,
             st.ctypes.data_as(C.c_void_p)) == 0
    assert n_out.value == 0 and (st == 0).all()
    r = "ACGTTGCAAGCTAGGCTTAACG" * 20
    for seqs, lib in (([], []), ([], [r]), ([r], []), ([""], [""]), (["", "ACGT", ""], [r]), ([r], ["ACGTACGTACGT"]), (["N" * 500], [r]), ([r], ["N" * 500])):
        got = _annotate(ctx, seqs, lib)
        assert got[0] == [] and got[1] == [0] * len(lib) and got[2]["hits"] == 0, (seqs, lib)
    recs, status = ctx.annotate([], [])
    assert recs.shape == (0, 10) and recs.dtype == np.int32 and status.shape == (0,)
