"""The window gather in chunks of the destination (hite_pipeline.hip: row_meta_kernel's row descriptors, gather_items_kernel,
row_gather_chunks_kernel; hite_genome.h: the gather_chunk block) on the device, through hite_fine_rows -- the launches of the stage
itself -- on the tables of tests/gather_chunk_cases.py: window lengths on both sides of a chunk and of an item of 256 chunks (rows of
exactly 1, 2, 3 and 4 items), the seam of the first500 + last500 form with pads on both sides of it on all four strand combinations,
rows of 1 and 4 items in turn with candidates of 0 / 1 / 5 / 100 rows and an empty last one, windows at genome position 0, on the last
base and at the first base of a later contig.  Both forms of the gather (HITE_GATHER_CHUNKS = 1 and 0, chosen per context) must give
the rows of the twin (tests/oracle_pipeline.py: pass_rows), byte for byte, on both passes, and hence each other's; the chunk form also
leaves the bytes between a row's length and the end of its slot zero."""
import ctypes as C

import numpy as np
import pytest

import fine_row_cases as FR
import gather_chunk_cases as GC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import hite_amd

    c = hite_amd.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("name", GC.names())
def test_both_forms_equal_the_twin(ctx, name):
    FR.use(ctx)
    c = GC.case(name)
    try:
        for p in (0, 1):
            exp, et = GC.twin(name, p)
            got = {}
            for chunks in (False, True):
                ctx.gather_config(chunks)
                got[chunks], gt = ctx.fine_rows(c["cands"], c["copies"], flank=FR.FLANK, rows_pass=p)
                assert [int(x) for x in gt] == et, (name, p, chunks, gt, et)
                for k, (gr, er) in enumerate(zip(got[chunks], exp)):
                    assert [(r[0], r[2], len(r[1])) for r in gr] == [(r[0], r[2], len(r[1])) for r in er], (name, p, chunks, k)
                    for a, b in zip(gr, er):
                        if a[1] != b[1]:
                            bad = [i for i in range(len(b[1])) if a[1][i] != b[1][i]]
                            raise AssertionError("%s pass %d chunks %d candidate %d copy %d: %d bytes differ, first at %d: %r != %r" %
                                                 (name, p, chunks, k, a[0], len(bad), bad[0], a[1][bad[0]:bad[0] + 8], b[1][bad[0]:bad[0] + 8]))
            assert got[False] == got[True], (name, p)
    finally:
        ctx.gather_config(None)


_CHILD = r"""
import hashlib, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import hite_amd
import fine_row_cases as FR
import gather_chunk_cases as GC
ctx = hite_amd.Context(0)
FR.use(ctx)
c = GC.case("seam_+")
h = hashlib.sha256()
for p in (0, 1):
    rows, tot = ctx.fine_rows(c["cands"], c["copies"], flank=FR.FLANK, rows_pass=p)
    h.update(repr(([[(int(a), bytes(b), bool(t)) for a, b, t in r] for r in rows], [int(x) for x in tot])).encode())
print("mode", int(ctx.gather_mode()), h.hexdigest())
ctx.close()
"""


@pytest.mark.parametrize("value, chunks", (("0", False), ("1", True), (None, True)))
def test_the_environment_chooses_the_form(value, chunks):
    """HITE_GATHER_CHUNKS in a fresh process (the default is read from the environment once): 0 = a wavefront per row, anything else
    or nothing = chunks; the rows are the twin's either way"""
    import hashlib
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k != "HITE_GATHER_CHUNKS"}
    if value is not None:
        env["HITE_GATHER_CHUNKS"] = value
    res = subprocess.run([sys.executable, "-c", _CHILD, root, os.path.join(root, "tests")], env=env, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    h = hashlib.sha256()
    for p in (0, 1):
        exp, et = GC.twin("seam_+", p)
        h.update(repr(([[(int(a), bytes(b), bool(t)) for a, b, t in r] for r in exp], [int(x) for x in et])).encode())
    assert res.stdout.split() == ["mode", str(int(chunks)), h.hexdigest()], res.stdout


def _raw_rows(ctx, c, p):
    """hite_fine_rows itself: the whole window buffer, slots and all"""
    from hite_amd._lib import _arr, _p

    n = len(c["cands"])
    cb = [s.encode() for s in c["cands"]]
    coff = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(s) for s in cb], out=coff[1:])
    cbuf = np.frombuffer(b"".join(cb) + b"\0" * 16, dtype=np.uint8)
    cf = np.zeros(n + 1, dtype=np.int32)
    np.cumsum([len(s) for s in c["copies"]], out=cf[1:])
    flat = [t for s in c["copies"] for t in s]
    rows, wbytes = GC.twin(c["name"], p)[1][:2]
    nrows = np.zeros(n + 1, dtype=np.int32)
    row_copy, row_len = np.zeros(rows + 1, dtype=np.int32), np.zeros(rows + 1, dtype=np.int32)
    row_trunc, win_off = np.zeros(rows + 1, dtype=np.uint8), np.zeros(rows + 2, dtype=np.int64)
    win = np.full(wbytes + 16, 0x5a, dtype=np.uint8)
    totals = np.zeros(4, dtype=np.int64)
    rc = ctx.lib.hite_fine_rows(ctx.h, n, _p(cbuf), _p(coff), _p(cf), C.c_int64(len(flat)), _p(_arr([t[0] for t in flat], np.int32)),
                                _p(_arr([t[1] for t in flat], np.int64)), _p(_arr([t[2] for t in flat], np.int64)),
                                _p(_arr([t[3] for t in flat], np.uint8)), _p(_arr([t[5] for t in flat], np.uint32)), FR.FLANK, p, _p(nrows),
                                C.c_int64(rows), _p(row_copy), _p(row_len), _p(row_trunc), _p(win_off), C.c_int64(wbytes), _p(win), _p(totals))
    assert rc == 0 and int(totals[0]) == rows and int(totals[1]) == wbytes
    return row_len[:rows], win_off[:rows + 1], win


@pytest.mark.parametrize("name", ("item_edges_+", "seam_-", "item_search"))
def test_slot_tails_are_zero(ctx, name):
    """the chunk form writes every byte of a row's slot: zeros behind the row's length"""
    FR.use(ctx)
    ctx.gather_config(True)
    try:
        for p in (0, 1):
            row_len, win_off, win = _raw_rows(ctx, GC.case(name), p)
            tails = 0
            for L, o, o1 in zip(row_len, win_off[:-1], win_off[1:]):
                assert o1 - o == (L + 15) // 16 * 16 and not win[o + L:o1].any(), (name, p, int(o))
                tails += int(o1 - o - L)
            assert tails > 0
    finally:
        ctx.gather_config(None)
