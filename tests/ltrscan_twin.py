"""TEST INFRASTRUCTURE: the CPU twin of hite_ltr_scan (include/hite_gpu.h, "LTR candidate scan"), the readable statement of the
definition the HIP code (hite_amd/csrc/hite_ltrscan.hip) must equal record for record and counter for counter.  Two forms:
  - this module (form="py"): steps 1-3 and 5-6 in tuples and dictionaries; step 4 is the recurrence of hite_pair_hsps, taken from
    tests/pairhsp_twin.py as it stands (align_c by default, the pure Python align with align=align_py);
  - tests/ltrscan_twin.c (form="c", the default), compiled with the host compiler, for the volume cases.
It is not LtrDetector: see the header for what is and is not claimed."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import pairhsp_twin as PT

HERE = os.path.dirname(os.path.abspath(__file__))

WORD = 13                   # HITE_LTRSCAN_WORD
MAX_OCC = 16                # HITE_LTRSCAN_MAX_OCC
BIN_SHIFT = 6               # HITE_LTRSCAN_BIN_SHIFT
LATTICES = (0, 32)          # HITE_LTRSCAN_LATTICE: the second lattice is shifted by half a bin
GAP = 100                   # HITE_LTRSCAN_GAP
MIN_HITS = 4                # HITE_LTRSCAN_MIN_HITS
BAND_BELOW, BAND_ABOVE = 96, 96     # HITE_LTRSCAN_BAND_BELOW / _ABOVE: dc - 96 <= y - x <= dc + 95
PADS = (256, 1024, 4096)    # HITE_LTRSCAN_PAD_0 .. _2; the last pad is max_ltr
EDGE = 32                   # HITE_LTRSCAN_EDGE
MAX_REDO = 3                # HITE_LTRSCAN_MAX_REDO
MAX_LTR = 8192              # HITE_LTRSCAN_MAX_LTR
DEFAULTS = dict(min_len=400, max_len=22000, min_ltr=100, max_ltr=6000, identity=85)
STATS = ("words", "hits", "runs", "runs_span", "alignments", "redos", "no_hsp", "drop_ltr", "drop_len", "drop_overlap", "drop_identity",
         "records")


def limits_ok(min_len, max_len, min_ltr, max_ltr, identity):
    return 1 <= min_ltr <= max_ltr <= MAX_LTR and min_len <= max_len and 1 <= identity <= 100


def words(c):
    """position -> the 13-base word that begins there"""
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


def links(wd, dmin, dmax):
    """step 2: [(i, d)] ascending in i"""
    where = {}
    for i in sorted(wd):
        where.setdefault(wd[i], []).append(i)
    hits = []
    for occ in where.values():
        for k, i in enumerate(occ):
            for j in occ[k + 1:k + 1 + MAX_OCC]:
                if j - i >= dmin:
                    if j - i <= dmax:
                        hits.append((i, j - i))
                    break
    return sorted(hits)


def runs(hits, lam):
    """step 3 on one lattice: [(i_lo, i_hi, d_lo, d_hi, hits)] of every maximal chain"""
    out, cur, key = [], None, None
    for b, i, d in sorted(((d + lam) >> BIN_SHIFT, i, d) for i, d in hits):
        if cur is not None and key == b and i - cur[1] <= GAP:
            cur = [cur[0], i, min(cur[2], d), max(cur[3], d), cur[4] + 1]
        else:
            if cur is not None:
                out.append(tuple(cur))
            cur, key = [i, i, d, d, 1], b
    if cur is not None:
        out.append(tuple(cur))
    return out


def align_py(q, s, dlo, dhi, r0, r1, c0, c1):
    """pairhsp_twin.align (pure Python) on the bytes of the two windows, as align_c takes them"""
    return PT.align(PT.codes(q), PT.codes(s), dlo, dhi, r0, r1, c0, c1)


def extend(s, run, max_ltr, align, st):
    """step 4 -> (ls, le, rs, re, score, matches, columns) or None"""
    i_lo, i_hi, d_lo, d_hi = run[:4]
    n = len(s)
    dc = (d_lo + d_hi) >> 1
    pads = [min(p, max_ltr) for p in PADS] + [max_ltr]
    pl = pr = redo = 0
    while True:
        qb, qe = max(0, i_lo - pads[pl]), min(n, i_hi + WORD + pads[pr])
        sb, se = max(0, qb + dc - BAND_BELOW), min(n, qe + dc + BAND_ABOVE)
        dlo = dc - BAND_BELOW - (sb - qb)
        st["alignments"] += 1
        h = align(s[qb:qe], s[sb:se], dlo, dlo + BAND_BELOW + BAND_ABOVE - 1, 1, qe - qb, 1, se - sb) if se > sb else None
        if h is None or h[4] < PT.MIN_SCORE:
            st["no_hsp"] += 1
            return None
        ls, le, rs, re_ = qb + h[0] - 1, qb + h[1], sb + h[2] - 1, sb + h[3]
        step = False
        if ls - qb < EDGE and qb > 0 and pl < len(pads) - 1:
            pl, step = pl + 1, True
        if qe - le < EDGE and qe < n and pr < len(pads) - 1:
            pr, step = pr + 1, True
        if not step or redo == MAX_REDO:
            return (ls, le, rs, re_, h[4], h[5], h[6])
        redo += 1
        st["redos"] += 1


def passes(r, min_len, max_len, min_ltr, max_ltr, identity):
    """step 5 -> None or the name of the first filter that drops (ls, le, rs, re, score, matches, columns)"""
    ls, le, rs, re_, _score, matches, columns = r
    if not (min_ltr <= le - ls <= max_ltr and min_ltr <= re_ - rs <= max_ltr):
        return "drop_ltr"
    if not min_len <= re_ - ls <= max_len:
        return "drop_len"
    if le > rs:
        return "drop_overlap"
    if 100 * matches < identity * columns:
        return "drop_identity"
    return None


def order_and_dedup(recs):
    """step 6 on (seq, ls, le, rs, re, score, matches, columns)"""
    out = []
    for r in sorted(recs, key=lambda r: (r[0], r[1], r[4], r[2], r[3], -r[5], -r[6], r[7])):
        if not out or out[-1][:5] != r[:5]:
            out.append(r)
    return out


def scan_py(seqs, min_len, max_len, min_ltr, max_ltr, identity, align=None):
    align = align or PT.align_c
    st = dict.fromkeys(STATS, 0)
    recs = []
    dmin, dmax = min_ltr, max_len - min_ltr
    for q, s in enumerate(seqs):
        s = PT.as_bytes(s)
        wd = words(PT.codes(s))
        st["words"] += len(wd)
        hits = links(wd, dmin, dmax)
        st["hits"] += len(hits)
        for lam in LATTICES:
            for run in runs(hits, lam):
                if run[4] < MIN_HITS:
                    continue
                st["runs"] += 1
                if run[1] - run[0] + WORD > max_ltr:
                    st["runs_span"] += 1
                    continue
                r = extend(s, run, max_ltr, align, st)
                if r is None:
                    continue
                why = passes(r, min_len, max_len, min_ltr, max_ltr, identity)
                if why:
                    st[why] += 1
                else:
                    recs.append((q,) + r)
    recs = order_and_dedup(recs)
    st["records"] = len(recs)
    return recs, st


_CLIB = None


def clib():
    """tests/ltrscan_twin.c built with the host compiler (it includes tests/pairhsp_twin.c for step 4)"""
    global _CLIB
    if _CLIB is None:
        d = tempfile.mkdtemp(prefix="ltrscan_twin_")
        so = os.path.join(d, "ltrscan_twin.so")
        extra = os.environ.get("HITE_HOST_CXXFLAGS", "").split()
        subprocess.run(["gcc", "-O2", "-shared", "-fPIC"] + extra + ["-o", so, os.path.join(HERE, "ltrscan_twin.c")], check=True)
        _CLIB = C.CDLL(so)
    return _CLIB


def scan_c(seqs, min_len, max_len, min_ltr, max_ltr, identity):
    buf, off, _n, _cols = PT.pack_args(seqs, [])
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    st = np.zeros(len(STATS), dtype=np.int64)
    cap = 1 << 12
    while True:
        recs, n_out = np.zeros((cap, 8), dtype=np.int32), C.c_int64(0)
        rc = clib().twin_ltr_scan(C.c_int64(len(off) - 1), p(buf), p(off), C.c_int32(min_len), C.c_int32(max_len), C.c_int32(min_ltr),
                                  C.c_int32(max_ltr), C.c_int32(identity), C.c_int64(cap), p(recs), C.byref(n_out), p(st))
        if rc == -4:
            cap = n_out.value
            continue
        assert rc == 0, rc
        break
    return [tuple(r) for r in recs[:n_out.value].tolist()], dict(zip(STATS, (int(v) for v in st)))


def scan(seqs, min_len=400, max_len=22000, min_ltr=100, max_ltr=6000, identity=85, stats=None, form="c", align=None):
    """what hite_amd.Context.ltr_scan returns, as a list of 8-tuples (seq, ls, le, rs, re, score, matches, columns); stats (a dict)
    receives the counters.  ValueError beyond the limits (HITE_EINVAL)."""
    if not limits_ok(min_len, max_len, min_ltr, max_ltr, identity):
        raise ValueError("ltr_scan: limits")
    recs, st = scan_py(seqs, min_len, max_len, min_ltr, max_ltr, identity, align) if form == "py" else \
        scan_c(seqs, min_len, max_len, min_ltr, max_ltr, identity)
    if stats is not None:
        stats.update(st)
    return recs


def scan_array(seqs, stats=None, **kw):
    """the twin with the signature and the return type of Context.ltr_scan (util.ltr_candidate_scan(scan=...))"""
    kw.pop("cap", None)
    return np.asarray(scan(seqs, stats=stats, **kw), dtype=np.int32).reshape(-1, 8)
