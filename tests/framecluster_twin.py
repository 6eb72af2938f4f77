"""TEST INFRASTRUCTURE: the CPU twin of hite_frame_cluster (include/hite_gpu.h, "clusters of a group of frames"), a plain statement
of the definition; the product imports none of this.  Two forms that the CPU suite holds equal:
  - this module: the recurrence over packed 64-bit cells (numpy, one anti-diagonal of the matrix per step) and the ordered pass;
  - tests/framecluster_twin.c, compiled with the host compiler: the same definition cell by cell and row by row -- the form the
    GPU tests and the stage tests use, because it is fast (frame_cluster(..., form="c"), the default).
A third statement that shares no code with either, tuple arithmetic on Python lists, is tests/framecluster_cases.py::plain_cluster."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_ROWS, MAX_LEN = 128, 256        # HITE_FRAMECLUSTER_MAX_ROWS, HITE_FRAMECLUSTER_MAX_LEN

# a value (score, matches, columns, bases of A, bases of B) as one integer: 10 + 9 + 10 + 9 + 9 bits, the score on top
SCORE = 1 << 37
MATCH = 2 * SCORE + (1 << 28) + (1 << 18) + (1 << 9) + 1
MISMATCH = -2 * SCORE + (1 << 18) + (1 << 9) + 1
GAP_A = -3 * SCORE + (1 << 18) + (1 << 9)
GAP_B = -3 * SCORE + (1 << 18) + 1

_CODE = np.full(256, 4, dtype=np.int64)
for _k, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _CODE[ord(_c.lower())] = _k


def as_bytes(s):
    return s.encode("latin-1") if isinstance(s, str) else bytes(s)


def codes(s):
    return _CODE[np.frombuffer(as_bytes(s), dtype=np.uint8)]


def unpack(v):
    v = int(v)
    return (v >> 37, (v >> 28) & 511, (v >> 18) & 1023, (v >> 9) & 511, v & 511)


def pair_value_codes(a, b):
    """R(A, B) of two code arrays as the packed integer"""
    m, n = len(a), len(b)
    best = 0
    if m == 0 or n == 0:
        return best
    p1 = np.zeros(m + 1, dtype=np.int64)      # V(i, d - 1 - i)
    p2 = np.zeros(m + 1, dtype=np.int64)      # V(i, d - 2 - i)
    for d in range(2, m + n + 1):
        lo, hi = max(1, d - n), min(m, d - 1)
        i = np.arange(lo, hi + 1)
        ca, cb = a[i - 1], b[d - i - 1]
        v = p2[i - 1] + np.where((ca == cb) & (ca < 4), MATCH, MISMATCH)
        v = np.maximum(v, p1[i - 1] + GAP_A)
        v = np.maximum(v, p1[i] + GAP_B)
        v[v < SCORE] = 0
        cur = np.zeros(m + 1, dtype=np.int64)
        cur[lo:hi + 1] = v
        best = max(best, int(v.max()))
        p2, p1 = p1, cur
    return best


def revcomp_codes(b):
    r = b[::-1].copy()
    r[r < 4] = 3 - r[r < 4]
    return r


def pair_value(a, b, both_strands=True):
    """R as the tuple (score, matches, columns, bases of a, bases of b)"""
    ca, cb = codes(a), codes(b)
    v = pair_value_codes(ca, cb)
    if both_strands:
        v = max(v, pair_value_codes(ca, revcomp_codes(cb)))
    return unpack(v)


def similar(r, la, lb, ident, cov_short, cov_long, min_cov):
    _s, k, c, a, b = r
    return (c > 0 and float(k) >= ident * float(c) and a >= min_cov and b >= min_cov and float(a) >= cov_long * float(la)
            and float(b) >= cov_short * float(lb))


def cluster_group(rows, ident, cov_short=0.0, cov_long=0.0, min_cov=0, min_len=10, both_strands=True, value=pair_value):
    """one group -> its clusters (lists of row indices: the representative, then the rows that joined, in the order they joined),
    in order of creation; None beyond a limit"""
    rows = [as_bytes(r) for r in rows]
    if len(rows) > MAX_ROWS or any(len(r) > MAX_LEN for r in rows):
        return None
    order = sorted((k for k in range(len(rows)) if len(rows[k]) > min_len), key=lambda k: (-len(rows[k]), k))
    clusters = []
    for k in order:
        for cl in clusters:
            rep = rows[cl[0]]
            if similar(value(rep, rows[k], both_strands), len(rep), len(rows[k]), ident, cov_short, cov_long, min_cov):
                cl.append(k)
                break
        else:
            clusters.append([k])
    return clusters


_CLIB = None


def clib():
    """tests/framecluster_twin.c built with the host compiler (as tests/identity_twin.py builds its C file)"""
    global _CLIB
    if _CLIB is None:
        d = tempfile.mkdtemp(prefix="framecluster_twin_")
        so = os.path.join(d, "framecluster_twin.so")
        extra = os.environ.get("HITE_HOST_CXXFLAGS", "").split()
        subprocess.run(["gcc", "-O2", "-shared", "-fPIC"] + extra + ["-o", so, os.path.join(HERE, "framecluster_twin.c")], check=True)
        _CLIB = C.CDLL(so)
    return _CLIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def pair_value_c(a, b, both_strands=True):
    a, b = as_bytes(a), as_bytes(b)
    out = np.zeros(5, dtype=np.int32)
    ab, bb = np.frombuffer(a + b"\0", dtype=np.uint8), np.frombuffer(b + b"\0", dtype=np.uint8)
    clib().twin_pair_value(_p(ab), len(a), _p(bb), len(b), int(bool(both_strands)), _p(out))
    return tuple(int(x) for x in out)


def groups_from_rows(groups, cluster_of_row, n_cluster, lens):
    """the C interface's per-row cluster index -> per group the list of clusters, members in the order they joined"""
    out, at = [], 0
    for g, rows in enumerate(groups):
        n = len(rows)
        if n_cluster[g] < 0:
            out.append(None)
        else:
            cls = [[] for _ in range(n_cluster[g])]
            for k in sorted(range(n), key=lambda k: (-lens[at + k], k)):
                if cluster_of_row[at + k] >= 0:
                    cls[cluster_of_row[at + k]].append(k)
            out.append(cls)
        at += n
    return out


def frame_cluster(groups, ident, cov_short=0.0, cov_long=0.0, min_cov=0, min_len=10, both_strands=True, form="c"):
    """what hite_amd.Context.frame_cluster returns; form "c" (tests/framecluster_twin.c) or "py" (this module)"""
    groups = [[as_bytes(r) for r in g] for g in groups]
    if form == "py":
        return [cluster_group(g, ident, cov_short, cov_long, min_cov, min_len, both_strands) for g in groups]
    flat = [r for g in groups for r in g]
    row_off = np.zeros(len(groups) + 1, dtype=np.int64)
    np.cumsum([len(g) for g in groups], out=row_off[1:])
    seq_off = np.zeros(len(flat) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in flat], out=seq_off[1:])
    buf = np.frombuffer(b"".join(flat) + b"\0" * 16, dtype=np.uint8)
    cl = np.zeros(len(flat) + 1, dtype=np.int32)
    ncl = np.zeros(len(groups) + 1, dtype=np.int32)
    rc = clib().twin_frame_cluster(C.c_int64(len(groups)), _p(row_off), _p(buf), _p(seq_off), C.c_double(ident), C.c_double(cov_short),
                                   C.c_double(cov_long), C.c_int32(min_cov), C.c_int32(min_len), C.c_int32(int(bool(both_strands))), _p(cl),
                                   _p(ncl))
    assert rc == 0, rc
    return groups_from_rows(groups, cl.tolist(), ncl.tolist(), np.diff(seq_off).tolist())
