"""TEST INFRASTRUCTURE: the CPU twin of hite_annotate (include/hite_gpu.h, "genome annotation"), the readable statement of the
definition the HIP code (hite_amd/csrc/hite_annotate.hip) must equal record for record and counter for counter.  Two forms:
  - this module (form="py"): the six steps in tuples and dictionaries; step 4 is the recurrence of hite_pair_hsps, taken from
    tests/pairhsp_twin.py as it stands (align_c by default, the pure Python align with align=align_py);
  - tests/annotate_twin.c (form="c", the default), compiled with the host compiler, for the volume cases.
It is not RepeatMasker: see the header for what is and is not claimed."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import pairhsp_twin as PT

HERE = os.path.dirname(os.path.abspath(__file__))

WORD = 13                   # HITE_ANNOT_WORD
MAX_OCC = 16                # HITE_ANNOT_MAX_OCC
BIN_SHIFT = 6               # HITE_ANNOT_BIN_SHIFT
LATTICES = (0, 32)          # HITE_ANNOT_LATTICE: the second lattice is shifted by half a bin
GAP = 300                   # HITE_ANNOT_GAP
MIN_HITS = 3                # HITE_ANNOT_MIN_HITS
MAX_SPAN = 8192             # HITE_ANNOT_MAX_SPAN
BAND_BELOW, BAND_ABOVE = 96, 96     # HITE_ANNOT_BAND_BELOW / _ABOVE: dc - 96 <= g - q <= dc + 95
PADS = (256, 1024, 4096, 8192)      # HITE_ANNOT_PAD_0 .. _3
EDGE = 32                   # HITE_ANNOT_EDGE
MAX_REDO = 3                # HITE_ANNOT_MAX_REDO
PIECE = 1 << 24             # HITE_ANNOT_PIECE
MIN_PIECE = 256             # HITE_ANNOT_MIN_PIECE
OVERLAP = 1 << 16           # HITE_ANNOT_OVERLAP
MAX_LIB_LEN = 24576         # HITE_ANNOT_MAX_LIB_LEN
MAX_LIB = 32768             # HITE_ANNOT_MAX_LIB
STATS = ("table", "silenced", "too_long", "hits", "runs", "alignments", "redos", "no_hsp", "hsps", "duplicates", "dominated", "records")


def limits_ok(n_lib, piece_len):
    return n_lib <= MAX_LIB and (piece_len == 0 or MIN_PIECE <= piece_len <= PIECE)


def revcomp_codes(c):
    return [3 - x if x < 4 else 4 for x in reversed(c)]


def words(c, lo=0, hi=None):
    """position -> the 13-base word that begins there, for the positions lo <= i, i + 13 <= hi"""
    hi = len(c) if hi is None else hi
    out = {}
    for i in range(lo, hi - WORD + 1):
        w = 0
        for x in c[i:i + WORD]:
            if x == 4:
                break
            w = w * 4 + x
        else:
            out[i] = w
    return out


def table(lib, st):
    """step 1 -> (texts: t -> codes or None, word -> [(t, q)] without the silenced words)"""
    texts, tab = [], {}
    for e in lib:
        c = PT.codes(e)
        if len(c) > MAX_LIB_LEN:
            st["too_long"] += 1
            texts += [None, None]
        else:
            texts += [c, revcomp_codes(c)]
    for t, c in enumerate(texts):
        for q, w in (words(c) if c is not None else {}).items():
            tab.setdefault(w, []).append((t, q))
    st["table"] = sum(len(v) for v in tab.values())
    st["silenced"] = sum(len(v) for v in tab.values() if len(v) > MAX_OCC)
    return texts, {w: v for w, v in tab.items() if len(v) <= MAX_OCC}


def pieces(n, piece_len):
    p = piece_len or PIECE
    return [(k * p, min(n, (k + 1) * p + OVERLAP)) for k in range((n + p - 1) // p)]


def hits_of(c, begin, end, tab):
    """step 2 on one piece: [(t, g, d)]"""
    return [(t, g, g - q) for g, w in words(c, begin, end).items() for t, q in tab.get(w, ())]


def runs(hits, begin, lam):
    """step 3 on one piece and one lattice: [(t, g_lo, g_hi, d_lo, d_hi, hits)] of every chain"""
    out, cur, key = [], None, None
    for t, b, g, d in sorted((t, (d - begin + lam + MAX_LIB_LEN) >> BIN_SHIFT, g, d) for t, g, d in hits):
        if cur is not None and key == (t, b) and g - cur[2] <= GAP and g - cur[1] < MAX_SPAN:
            cur = [t, cur[1], g, min(cur[3], d), max(cur[4], d), cur[5] + 1]
        else:
            if cur is not None:
                out.append(tuple(cur))
            cur, key = [t, g, g, d, d, 1], (t, b)
    if cur is not None:
        out.append(tuple(cur))
    return out


def align_py(q, s, dlo, dhi, r0, r1, c0, c1):
    """pairhsp_twin.align (pure Python) on the bytes of the two windows, as align_c takes them"""
    return PT.align(PT.codes(q), PT.codes(s), dlo, dhi, r0, r1, c0, c1)


_BYTES = b"ACGTN"


def extend(s, text, run, align, st):
    """step 4 for a run of a text (codes) on the sequence s (bytes) -> (gs, ge, qs, qe, score, matches, columns) or None"""
    _t, g_lo, g_hi, d_lo, d_hi = run[:5]
    n, L = len(s), len(text)
    dc = (d_lo + d_hi) >> 1
    q_lo, q_hi = g_lo - dc, g_hi - dc
    pl = pr = redo = 0
    tb = bytes(_BYTES[x] for x in text)
    while True:
        qb, qe = max(0, q_lo - PADS[pl]), min(L, q_hi + WORD + PADS[pr])
        sb, se = max(0, qb + dc - BAND_BELOW), min(n, qe + dc + BAND_ABOVE)
        dlo = dc - BAND_BELOW - (sb - qb)
        st["alignments"] += 1
        h = align(tb[qb:qe], s[sb:se], dlo, dlo + BAND_BELOW + BAND_ABOVE - 1, 1, qe - qb, 1, se - sb) if se > sb and qe > qb else None
        if h is None or h[4] < PT.MIN_SCORE:
            st["no_hsp"] += 1
            return None
        qs, qe_, gs, ge = qb + h[0] - 1, qb + h[1], sb + h[2] - 1, sb + h[3]
        step = False
        if qs - qb < EDGE and qb > 0 and pl < len(PADS) - 1:
            pl, step = pl + 1, True
        if qe - qe_ < EDGE and qe < L and pr < len(PADS) - 1:
            pr, step = pr + 1, True
        if not step or redo == MAX_REDO:
            return (gs, ge, qs, qe_, h[4], h[5], h[6])
        redo += 1
        st["redos"] += 1


def order_key(r):
    return r[:7] + (-r[7], -r[8], r[9])


def better(b, a):
    return b[7] > a[7] or (b[7] == a[7] and order_key(b) < order_key(a))


def covers(b, a):
    """B shares at least 80 % of A's bases"""
    ov = min(a[2], b[2]) - max(a[1], b[1])
    return ov > 0 and 5 * ov >= 4 * (a[2] - a[1])


def resolve(recs, st):
    """steps 5 and 6 on (seq, g_start, g_end, lib, strand, q_start, q_end, score, matches, columns)"""
    uniq = []
    for r in sorted(recs, key=order_key):
        if uniq and uniq[-1][:7] == r[:7]:
            st["duplicates"] += 1
        else:
            uniq.append(r)
    out = []
    for a in uniq:
        if any(b is not a and b[0] == a[0] and covers(b, a) and better(b, a) for b in uniq):
            st["dominated"] += 1
        else:
            out.append(a)
    return out


def annotate_py(seqs, lib, piece_len=0, align=None):
    align = align or PT.align_c
    st = dict.fromkeys(STATS, 0)
    texts, tab = table(lib, st)
    status = [-1 if texts[2 * e] is None else 0 for e in range(len(lib))]
    recs = []
    for q, s in enumerate(seqs):
        s = PT.as_bytes(s)
        c = PT.codes(s)
        for begin, end in pieces(len(s), piece_len):
            hits = hits_of(c, begin, end, tab)
            st["hits"] += len(hits)
            for lam in LATTICES:
                for run in runs(hits, begin, lam):
                    if run[5] < MIN_HITS:
                        continue
                    st["runs"] += 1
                    t = run[0]
                    r = extend(s, texts[t], run, align, st)
                    if r is None:
                        continue
                    gs, ge, qs, qe = r[:4]
                    L = len(texts[t])
                    recs.append((q, gs, ge, t >> 1, t & 1) + ((L - qe, L - qs) if t & 1 else (qs, qe)) + r[4:])
    st["hsps"] = len(recs)
    recs = resolve(recs, st)
    st["records"] = len(recs)
    return recs, status, st


_CLIB = None


def clib():
    """tests/annotate_twin.c built with the host compiler (it includes tests/pairhsp_twin.c for step 4)"""
    global _CLIB
    if _CLIB is None:
        d = tempfile.mkdtemp(prefix="annotate_twin_")
        so = os.path.join(d, "annotate_twin.so")
        extra = os.environ.get("HITE_HOST_CXXFLAGS", "").split()
        subprocess.run(["gcc", "-O2", "-shared", "-fPIC"] + extra + ["-o", so, os.path.join(HERE, "annotate_twin.c")], check=True)
        _CLIB = C.CDLL(so)
    return _CLIB


def annotate_c(seqs, lib, piece_len=0, cap=None):
    """-> (records, status, stats, rc): with cap set, one call as it is (rc -4: the first cap records); else asked again with the room"""
    buf, off, _n, _cols = PT.pack_args(seqs, [])
    lbuf, loff, _n, _cols = PT.pack_args(lib, [])
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    st = np.zeros(len(STATS), dtype=np.int64)
    status = np.zeros(max(len(lib), 1), dtype=np.int8)
    room = 1 << 12 if cap is None else cap
    while True:
        recs, n_out = np.zeros((max(room, 1), 10), dtype=np.int32), C.c_int64(0)
        rc = clib().twin_annotate(C.c_int64(len(off) - 1), p(buf), p(off), C.c_int32(len(lib)), p(lbuf), p(loff), C.c_int32(piece_len), C.c_int64(room),
                                  p(recs), C.byref(n_out), p(status), p(st))
        if rc == -4 and cap is None:
            room = n_out.value
            continue
        assert rc in (0, -4), rc
        break
    return ([tuple(r) for r in recs[:min(n_out.value, room)].tolist()], [int(x) for x in status[:len(lib)]],
            dict(zip(STATS, (int(v) for v in st))), rc)


def annotate(seqs, lib, piece_len=0, stats=None, form="c", align=None):
    """what hite_amd.Context.annotate returns: (the records as a list of 10-tuples (seq, g_start, g_end, lib, strand, q_start, q_end,
    score, matches, columns), the lib status as a list); stats (a dict) receives the counters.  ValueError beyond the limits."""
    if not limits_ok(len(lib), piece_len):
        raise ValueError("annotate: limits")
    if form == "py":
        recs, status, st = annotate_py(seqs, lib, piece_len, align)
    else:
        recs, status, st, _rc = annotate_c(seqs, lib, piece_len)
    if stats is not None:
        stats.update(st)
    return recs, status


def annotate_array(seqs, lib, piece_len=0, cap=None, stats=None):
    """the twin with the signature and the return types of Context.annotate (util.annotate_genome(annot=...))"""
    recs, status = annotate(seqs, lib, piece_len, stats=stats)
    return np.asarray(recs, dtype=np.int32).reshape(-1, 10), np.asarray(status, dtype=np.int8)
