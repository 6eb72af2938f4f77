"""CPU twin of the pairwise identity (hite_amd/csrc/hite_ident.hip, hite_pair_identity; the primitive under the `-c` / `-A` of the
build's cd-hit-est stand-in).  Test infrastructure: the product imports none of this.  The definition is in the header comment of
tests/identity_twin.c (the same text as in include/hite_gpu.h); this module compiles that file with the host compiler and gives it the
interface of hite_amd.Context.pair_identity."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

MAX_LEN = 32767
MAX_WIDTH = 2048        # HITE_IDENT_MAX_WIDTH

_CLIB = None


def clib():
    """tests/identity_twin.c built with the host compiler (as tests/protein_twin.py builds its C file)"""
    global _CLIB
    if _CLIB is None:
        d = tempfile.mkdtemp(prefix="identity_twin_")
        so = os.path.join(d, "identity_twin.so")
        extra = os.environ.get("HITE_HOST_CXXFLAGS", "").split()
        subprocess.run(["gcc", "-O2", "-shared", "-fPIC"] + extra + ["-o", so, os.path.join(HERE, "identity_twin.c")], check=True)
        _CLIB = C.CDLL(so)
    return _CLIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def csr(seqs):
    sb = [s.encode("latin-1") if isinstance(s, str) else bytes(s) for s in seqs]
    off = np.zeros(len(sb) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in sb], out=off[1:])
    return np.frombuffer(b"".join(sb) + b"\0" * 16, dtype=np.uint8), off


def pair_columns(pairs):
    """pairs: rows (a_id, a_start, a_end, b_id, b_start, b_end, strand) -> the seven arrays of the C interface"""
    pr = np.asarray(pairs, dtype=np.int64).reshape(-1, 7)
    col = lambda k, t: np.ascontiguousarray(pr[:, k], dtype=t)  # noqa: E731
    return (col(0, np.int32), col(1, np.int64), col(2, np.int64), col(3, np.int32), col(4, np.int64), col(5, np.int64),
            np.ascontiguousarray(pr[:, 6] != 0, dtype=np.uint8))


def pair_identity(seqs, pairs, band=32, max_width=MAX_WIDTH):
    """-> int32 [n_pair, 2]: (cost, matches) of every pair, (-1, 0) for a pair beyond a limit or outside its sequences.
    max_width=0 lifts the limit on the band width (for bands that cover a whole matrix)."""
    buf, off = csr(seqs)
    ai, as_, ae, bi, bs, be, st = pair_columns(pairs)
    n = len(ai)
    cost, mat = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    rc = clib().twin_pair_identity(C.c_int64(len(off) - 1), _p(buf), _p(off), C.c_int64(n), _p(ai), _p(as_), _p(ae), _p(bi), _p(bs), _p(be),
                                   _p(st), C.c_int32(int(band)), C.c_int32(int(max_width)), _p(cost), _p(mat))
    assert rc == 0, rc
    return np.stack([cost, mat], axis=1)


def one(a, b, band, strand=0, max_width=0):
    """(cost, matches) of the whole of `a` against the whole of `b`"""
    r = pair_identity([a, b], [(0, 0, len(a), 1, 0, len(b), strand)], band, max_width)
    return int(r[0, 0]), int(r[0, 1])
