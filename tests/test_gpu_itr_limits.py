"""itr_search_kernel (hite_amd/csrc/hite_itr.hip) on the device at the limits of its own code, against the CPU twin
(oracle/hite_oracle_itr.c), a closed form and the tool's own answers (tests/golden/itr_limits.json.gz) on the records of
tests/itr_limit_cases.py -- the same check_* functions that test_itr_limit_cases.py runs with the twin in the device's place, where
every family is also shown to reach its limit.  Exact integer equality on all 8 fields everywhere.
   * closed form: perfect repeats of 6 .. 600 bases under three scorings, 0 / 1 / 2 bases between the ends;
   * path equivalence: every record of h <= 64 alone (store in LDS) and beside one record of h = 65, first or last (store in HBM);
     one mixed batch in three orders of h;
   * strip seams: planted gaps in either direction across columns 64, 128 and 192; alignments whose first cell is (1, 64 s + 1);
     a tie of gap open and gap extension on the path;
   * ties for the end cell: in two lanes of two strips, and in ONE lane of two strips (the same row, 64 columns apart);
   * alphabet and thresholds: all N, runs of N at either end of either sequence, lower case and IUPAC, identities exactly at and
     just below min_identity, min_len at end1, end1 + 1, 0 and -1;
   * lengths: L 0 .. 15, end_len 1 .. 600 against L below, at, between and above;
   * slots: 517 records through the 512 slots of the HBM path, long and short in turn, and 8199 through the 8192 of the LDS path,
     in one call and in pieces of 100;
   * bands: 1500 seeded records with h around 64, 128 and 500 under four scorings;
   * guards: the device entry's max_h promise (flags 8), bad arguments, n = 0, empty records."""
import ctypes as C

import numpy as np
import pytest

import itr_limit_cases as IC
from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import hite_amd

    c = hite_amd.Context(0)
    yield c
    c.close()


def _csr(seqs):
    sb = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
    off = np.zeros(len(sb) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in sb], out=off[1:])
    return np.frombuffer(b"".join(sb) + b"\0" * 16, dtype=np.uint8).copy(), off


def _dev_call(ctx, n, d_buf, d_off, d_out, end_len=0, max_h=IC.MAX_H, scoring=(10, 16, 32, 32), ctx_h=True):
    ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)     # noqa: E731
    return ctx.lib.hite_itr_search_dev(ctx.h if ctx_h else C.c_void_p(0), C.c_int64(n), ptr(d_buf), ptr(d_off), int(end_len), int(max_h),
                                       C.c_double(0.7), 7, *[int(x) for x in scoring], ptr(d_out), C.c_void_p(0))


def _dev_search(ctx):
    """hite_itr_search_dev on torch device buffers (the null stream, which torch's default stream is)"""
    import torch

    def search(seqs, end_len, max_h):
        buf, off = _csr(seqs)
        d_buf, d_off = torch.from_numpy(buf).cuda(), torch.from_numpy(off).cuda()
        d_out = torch.full((len(seqs) * 8,), -7, dtype=torch.int32, device="cuda")
        assert _dev_call(ctx, len(seqs), d_buf, d_off, d_out, end_len, max_h) == 0
        torch.cuda.synchronize()
        return d_out.cpu().numpy().reshape(len(seqs), 8)
    return search


def test_limits_are_exported(ctx):
    assert ctx.itr_limits() == IC.TABLE


def test_closed_form(ctx):
    IC.check_closed_form(ctx.itr_search)


def test_path_equivalence(ctx):
    n, n_hbm = IC.check_path_equivalence(ctx.itr_search)
    assert n_hbm > 500


def test_order(ctx):
    IC.check_order(ctx.itr_search)


def test_strip_seams(ctx):
    IC.check_seams(ctx.itr_search)


def test_ties(ctx):
    IC.check_ties(ctx.itr_search)


def test_alphabet_and_thresholds(ctx):
    IC.check_alphabet(ctx.itr_search)


def test_lengths(ctx):
    IC.check_lengths(ctx.itr_search)


@pytest.mark.parametrize("which", (0, 1), ids=("hbm", "lds"))
def test_slot_reuse(ctx, which):
    IC.check_slots(ctx.itr_search, which)


def test_bands(ctx):
    IC.check_bands(ctx.itr_search)


def test_tool_fixture(ctx):
    """the tool's own found / "Length itr=" / end1 / end2 at the limits"""
    IC.check_fixture(ctx.itr_search, load_golden("itr_limits"))


def test_max_h_promise(ctx):
    IC.check_max_h(_dev_search(ctx))


def test_bad_arguments_and_empty_batches(ctx):
    import torch

    seqs = [c[1] for c in IC.guard_batch()[1:6]]
    buf, off = _csr(seqs)
    n = len(seqs)
    d_buf, d_off = torch.from_numpy(buf).cuda(), torch.from_numpy(off).cuda()
    d_out = torch.full((n * 8,), -7, dtype=torch.int32, device="cuda")
    # the device entry
    assert _dev_call(ctx, -1, d_buf, d_off, d_out) == IC.EINVAL
    assert _dev_call(ctx, n, d_buf, d_off, d_out, ctx_h=False) == IC.EINVAL
    assert _dev_call(ctx, n, None, d_off, d_out) == IC.EINVAL
    assert _dev_call(ctx, n, d_buf, None, d_out) == IC.EINVAL
    assert _dev_call(ctx, n, d_buf, d_off, None) == IC.EINVAL
    assert _dev_call(ctx, n, d_buf, d_off, d_out, max_h=-1) == IC.EINVAL
    for k in range(4):
        for bad in (0, -1):
            sc = [10, 16, 32, 32]
            sc[k] = bad
            assert _dev_call(ctx, n, d_buf, d_off, d_out, scoring=sc) == IC.EINVAL
    assert _dev_call(ctx, 0, d_buf, d_off, d_out) == 0
    torch.cuda.synchronize()
    assert bool((d_out == -7).all()), "a refused or empty call wrote to the output"
    # the host entry
    out = np.full((n, 8), -7, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)     # noqa: E731

    def host(n_, buf_, off_, out_, sc=(10, 16, 32, 32), h=ctx.h):
        return ctx.lib.hite_itr_search(h, C.c_int64(n_), buf_, off_, 0, C.c_double(0.7), 7, *[int(x) for x in sc], out_)

    assert host(-1, p(buf), p(off), p(out)) == IC.EINVAL
    assert host(n, p(buf), p(off), p(out), h=C.c_void_p(0)) == IC.EINVAL
    assert host(n, None, p(off), p(out)) == IC.EINVAL
    assert host(n, p(buf), None, p(out)) == IC.EINVAL
    assert host(n, p(buf), p(off), None) == IC.EINVAL
    for k in range(4):
        sc = [10, 16, 32, 32]
        sc[k] = 0
        assert host(n, p(buf), p(off), p(out), sc) == IC.EINVAL
    unsorted = off.copy()
    unsorted[2], unsorted[3] = off[3], off[2]
    assert host(n, p(buf), p(unsorted), p(out)) == IC.EINVAL
    assert host(0, p(buf), p(off), p(out)) == 0 and host(0, None, None, None) == 0
    assert (out == -7).all(), "a refused or empty call wrote to the output"
    assert host(n, p(buf), p(off), p(out)) == 0 and np.array_equal(out, IC.twin_search(seqs, 0))
    # empty records only
    assert ctx.itr_search(["", "", ""], 0).tolist() == [IC.EMPTY_ROW] * 3
    assert ctx.itr_search(["", ""], 40).tolist() == [IC.EMPTY_ROW] * 2
    assert _dev_search(ctx)(["", "", "", "", ""], 0, 0).tolist() == [IC.EMPTY_ROW] * 5
    assert ctx.itr_search([], 0).shape == (0, 8)
