"""TEST INFRASTRUCTURE: the CPU twin of hite_pair_hsps (include/hite_gpu.h, "local alignments of pairs of intervals"), the readable
statement of the definition the HIP code (hite_amd/csrc/hite_pairhsp.hip) must equal record for record.  Two forms:
  - this module, tuples and dictionaries, for small pairs (form="py");
  - tests/pairhsp_twin.c, compiled with the host compiler: the same definition step by step -- the form the GPU tests and the
    stage tests use, because a band of a few thousand rows is too slow here (pair_hsps(..., form="c"), the default).
It is not blastn: see the header for what is and is not claimed."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

MAX_LEN = 32768             # HITE_PAIRHSP_MAX_LEN
WORD = 12                   # HITE_PAIRHSP_WORD
MAX_OCC = 8                 # HITE_PAIRHSP_MAX_OCC
BIN_SHIFT = 6               # HITE_PAIRHSP_BIN_SHIFT
MIN_VOTES = 8               # HITE_PAIRHSP_MIN_VOTES
MAX_WINDOWS = 4             # HITE_PAIRHSP_MAX_WINDOWS
BAND_BELOW, BAND_ABOVE = 32, 160    # HITE_PAIRHSP_BAND_BELOW / _ABOVE: 64 b - 32 <= k < 64 b + 160
MATCH, MISMATCH, GAP = 2, -4, -5    # HITE_PAIRHSP_MATCH / _MISMATCH / _GAP
MIN_SCORE = 56              # HITE_PAIRHSP_MIN_SCORE
MIN_RECT = 28               # HITE_PAIRHSP_MIN_RECT
MAX_HSPS = 12               # HITE_PAIRHSP_MAX_HSPS
NO_DIAG_MIN = -2 ** 31      # INT32_MIN: no limit

E = (0, 0, 0, 0, 0)
_CODE = {65: 0, 67: 1, 71: 2, 84: 3, 97: 0, 99: 1, 103: 2, 116: 3}


def as_bytes(s):
    return s.encode("latin-1") if isinstance(s, str) else bytes(s)


def codes(s):
    return [_CODE.get(c, 4) for c in as_bytes(s)]


def words(c):
    """position -> the word that begins there, for the positions whose twelve bases are all in ACGT"""
    out = {}
    for i in range(len(c) - WORD + 1):
        w = 0
        for x in c[i:i + WORD]:
            if x == 4:
                break
            w = w * 4 + x
        else:
            out[i] = w
    return out


def votes(qc, sc, diag_min=NO_DIAG_MIN):
    """vote[b] for b = 0 .. ((m + n - 2) >> 6) + 1 (the last one is always 0: w(b) reads one bin further)"""
    m, n = len(qc), len(sc)
    where = {}
    for i, w in words(qc).items():
        where.setdefault(w, []).append(i)
    vote = [0] * (((m + n - 2) >> BIN_SHIFT) + 2)
    for j, w in words(sc).items():
        occ = where.get(w, ())
        if len(occ) > MAX_OCC:
            continue
        for i in occ:
            if j - i >= diag_min:
                vote[(j - i + m - 1) >> BIN_SHIFT] += 1
    return vote


def windows(vote):
    """the chosen bins, in the order they are chosen"""
    chosen = []
    for _ in range(MAX_WINDOWS):
        best = None
        for b in range(len(vote) - 1):
            if any(abs(b - c) < 2 for c in chosen):
                continue
            w = vote[b] + vote[b + 1]
            if w >= MIN_VOTES and (best is None or w > best[0]):
                best = (w, b)
        if best is None:
            break
        chosen.append(best[1])
    return chosen


def band_of(b, m, diag_min=NO_DIAG_MIN):
    """the diagonals j - i of the band of bin b: (lowest, highest)"""
    return max((b << BIN_SHIFT) - BAND_BELOW - (m - 1), diag_min), (b << BIN_SHIFT) + BAND_ABOVE - 1 - (m - 1)


def _key(v):
    return (v[0], v[1], v[2], -v[3], -v[4])


def cell(diag, up, left, ca, cb, i, j):
    """V(i, j) from its three neighbours; the empty value starts a path at (i, j)"""
    hit = ca == cb and ca < 4
    if diag == E:
        d = (MATCH, 1, 1, i, j) if hit else E
    else:
        d = (diag[0] + (MATCH if hit else MISMATCH), diag[1] + (1 if hit else 0), diag[2] + 1, diag[3], diag[4])
    u = (up[0] + GAP, up[1], up[2] + 1, up[3], up[4]) if up != E else E
    le = (left[0] + GAP, left[1], left[2] + 1, left[3], left[4]) if left != E else E
    v = max((x if x[0] > 0 else E for x in (d, u, le)), key=_key)
    return v


def align(qc, sc, dlo, dhi, r0, r1, c0, c1):
    """the best cell of the rectangle inside the band dlo <= j - i <= dhi -> (q_start, q_end, s_start, s_end, score, matches,
    columns), or None when no cell has a positive score"""
    best, best_key = None, None
    prev = {}
    for i in range(r0, r1 + 1):
        cur = {}
        for j in range(max(c0, i + dlo), min(c1, i + dhi) + 1):
            v = cell(prev.get(j - 1, E), prev.get(j, E), cur.get(j - 1, E), qc[i - 1], sc[j - 1], i, j)
            if v != E:
                cur[j] = v
                k = _key(v) + (-i, -j)
                if best is None or k > best_key:
                    best, best_key = (v[3], i, v[4], j, v[0], v[1], v[2]), k
        prev = cur
    return best


def band_hsps(qc, sc, dlo, dhi):
    """the first HSP of a band and one more from the rectangle before it and from the one after it"""
    m, n = len(qc), len(sc)
    h = align(qc, sc, dlo, dhi, 1, m, 1, n)
    if h is None or h[4] < MIN_SCORE:
        return []
    out = [h]
    for r0, r1, c0, c1 in ((1, h[0] - 1, 1, h[2] - 1), (h[1] + 1, m, h[3] + 1, n)):
        if r1 - r0 + 1 >= MIN_RECT and c1 - c0 + 1 >= MIN_RECT:
            g = align(qc, sc, dlo, dhi, r0, r1, c0, c1)
            if g is not None and g[4] >= MIN_SCORE:
                out.append(g)
    return out


def order_and_dedup(hsps):
    """score descending, then q_start, s_start, q_end, s_end (equal keys stay in the order they were found); an HSP inside an
    earlier kept one on both sequences goes"""
    kept = []
    for h in sorted(hsps, key=lambda h: (-h[4], h[0], h[2], h[1], h[3])):
        if not any(k[0] <= h[0] and h[1] <= k[1] and k[2] <= h[2] and h[3] <= k[3] for k in kept):
            kept.append(h)
    return kept


def pair_hsps_one(q, s, diag_min=None):
    """the records of one pair of sequences, or None beyond a limit"""
    qc, sc = codes(q), codes(s)
    m, n = len(qc), len(sc)
    if m == 0 or n == 0 or m > MAX_LEN or n > MAX_LEN:
        return None
    dm = NO_DIAG_MIN if diag_min is None else int(diag_min)
    found = []
    for b in windows(votes(qc, sc, dm)):
        dlo, dhi = band_of(b, m, dm)
        found += band_hsps(qc, sc, dlo, dhi)
    return order_and_dedup(found)


_CLIB = None


def clib():
    """tests/pairhsp_twin.c built with the host compiler (as tests/framecluster_twin.py builds its C file)"""
    global _CLIB
    if _CLIB is None:
        d = tempfile.mkdtemp(prefix="pairhsp_twin_")
        so = os.path.join(d, "pairhsp_twin.so")
        extra = os.environ.get("HITE_HOST_CXXFLAGS", "").split()
        subprocess.run(["gcc", "-O2", "-shared", "-fPIC"] + extra + ["-o", so, os.path.join(HERE, "pairhsp_twin.c")], check=True)
        _CLIB = C.CDLL(so)
    return _CLIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def align_c(q, s, dlo, dhi, r0, r1, c0, c1):
    """align() of the C form, on the bytes of the two sequences"""
    q, s = as_bytes(q), as_bytes(s)
    out = np.zeros(7, dtype=np.int32)
    ok = clib().twin_align(q, len(q), s, len(s), C.c_int64(dlo), C.c_int64(dhi), r0, r1, c0, c1, _p(out))
    return tuple(int(x) for x in out) if ok else None


def pack_args(seqs, pairs):
    """the arrays of the C interface: (buf, off, n_pair, [a_id, a_start, a_end, b_id, b_start, b_end])"""
    sb = [as_bytes(s) for s in seqs]
    off = np.zeros(len(sb) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in sb], out=off[1:])
    buf = np.frombuffer(b"".join(sb) + b"\0" * 16, dtype=np.uint8)
    pr = np.asarray(pairs, dtype=np.int64).reshape(-1, 6)
    cols = [np.ascontiguousarray(pr[:, k], dtype=np.int32 if k in (0, 3) else np.int64) for k in range(6)]
    return buf, off, len(pr), cols


def unpack(n, status, first, recs):
    """status / first / recs of the C interface -> per pair None or a list of 7-tuples"""
    out = []
    for p in range(n):
        if status[p] < 0:
            out.append(None)
        else:
            out.append([tuple(int(x) for x in recs[k]) for k in range(first[p], first[p + 1])])
    return out


def pair_hsps(seqs, pairs, diag_min=None, form="c"):
    """what hite_amd.Context.pair_hsps returns: pairs are rows (a_id, a_start, a_end, b_id, b_start, b_end), intervals 0-based and
    half-open; form "c" (tests/pairhsp_twin.c) or "py" (this module)"""
    if form == "py":
        sb, out = [as_bytes(s) for s in seqs], []
        for a, a0, a1, b, b0, b1 in pairs:
            ok = 0 <= a < len(sb) and 0 <= b < len(sb) and 0 <= a0 <= a1 <= len(sb[a]) and 0 <= b0 <= b1 <= len(sb[b])
            out.append(pair_hsps_one(sb[a][a0:a1], sb[b][b0:b1], diag_min) if ok else None)
        return out
    buf, off, n, cols = pack_args(seqs, pairs)
    if n == 0:
        return []
    cap = MAX_HSPS * n
    status, first, recs = np.zeros(n, dtype=np.int32), np.zeros(n + 1, dtype=np.int64), np.zeros((cap, 7), dtype=np.int32)
    n_out = C.c_int64(0)
    rc = clib().twin_pair_hsps(C.c_int64(len(off) - 1), _p(buf), _p(off), C.c_int64(n), *[_p(c) for c in cols],
                               C.c_int32(NO_DIAG_MIN if diag_min is None else int(diag_min)), C.c_int64(cap), _p(status), _p(first), _p(recs),
                               C.byref(n_out))
    assert rc == 0, rc
    return unpack(n, status, first, recs)


def one(q, s, diag_min=None, form="c"):
    q, s = as_bytes(q), as_bytes(s)
    return pair_hsps([q, s], [(0, 0, len(q), 1, 0, len(s))], diag_min, form)[0]
