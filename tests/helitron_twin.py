"""CPU twin of the Helitron candidate scan (hite_amd/csrc/hite_helitron.hip; the definition is in include/hite_gpu.h, "Helitron
candidate scan"): plain Python + numpy, brute force over anchors, patterns, gaps and body letters.  It reads the pattern LINES with
its own grammar (not util.parse_lcvs) and works on the bytes of the sequences.

  scores(seqs, head_lines, tail_lines)  -> int32 [4, total bytes]: plus heads, plus tails, minus heads, minus tails (the minus rows
                                            in the coordinates of the reverse complement), sequence k from column sum(len(seqs[:k]))
  scan(seqs, head_lines, tail_lines, ...) -> records (seq, start, end, strand, head score, tail score), ordered (seq, strand, start, end)
"""
import bisect
import re

import numpy as np

_GAP = r"(?:\.\{(\d+)(?:,(\d+))?\})?"
_BODY = r"([ACGT](?:[ACGT.]*[ACGT])?)"
_HEAD = re.compile("^TC" + _GAP + _BODY + "$")
_TAIL = re.compile("^" + _BODY + _GAP + r"CT\[AG\]\{2\}$")
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def parse(line, side):
    """-> (gap_min, gap_max, body)"""
    m = (_HEAD if side == "head" else _TAIL).match(line.strip())
    if not m:
        raise ValueError(line)
    a, b, body = (m.group(1), m.group(2), m.group(3)) if side == "head" else (m.group(2), m.group(3), m.group(1))
    gmin = int(a) if a is not None else 0
    return gmin, int(b) if b is not None else gmin, body


def as_bytes(s):
    return s.encode() if isinstance(s, str) else bytes(s)


def revcomp(s):
    """complement only ACGT (upper case), every other byte N"""
    s = as_bytes(s)
    keep = bytes(c if c in b"ACGT" else ord("N") for c in s)
    return keep.translate(_COMP)[::-1]


def _csr(seqs):
    sb = [as_bytes(s) for s in seqs]
    off = np.zeros(len(sb) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in sb], out=off[1:])
    return np.frombuffer(b"".join(sb) + b"\0" * 8, dtype=np.uint8), off


def _strand_scores(t, off, heads, tails):
    """t: bytes of a CSR batch (padded), off its offsets -> (head score, tail score) per byte"""
    nb = int(off[-1])
    hs, ts = np.zeros(nb, dtype=np.int32), np.zeros(nb, dtype=np.int32)
    if nb == 0:
        return hs, ts
    pos = np.arange(nb, dtype=np.int64)
    seq = np.searchsorted(off, pos, side="right") - 1
    b, e = off[seq], off[seq + 1]
    A, C, G, T = (t[:nb] == c for c in b"ACGT")
    R = A | G

    def at(mask, d):           # mask shifted: result[i] = mask[i + d], False outside the batch
        out = np.zeros(nb, dtype=bool)
        if abs(d) >= nb:
            return out
        if d >= 0:
            out[:nb - d] = mask[d:] if d else mask
        else:
            out[-d:] = mask[:nb + d]
        return out

    # heads: T at p, C at p + 1, both inside the sequence; the body begins at p + 2 + g and ends inside the sequence
    P = pos[T & at(C, 1) & (pos + 1 < e)]
    for gmin, gmax, body in heads:
        hit = np.zeros(len(P), dtype=bool)
        for g in range(gmin, gmax + 1):
            s0 = P + 2 + g
            ok = s0 + len(body) <= e[P]
            for k, ch in enumerate(body):
                if ch != ".":
                    ok &= t[np.minimum(s0 + k, nb)] == ord(ch)
            hit |= ok
        hs[P] += hit
    # tails: C T R R at q - 3 .. q inside the sequence; the body ends at q - 4 - g and begins inside the sequence
    Q = pos[R & at(R, -1) & at(T, -2) & at(C, -3) & (pos - 3 >= b)]
    for gmin, gmax, body in tails:
        hit = np.zeros(len(Q), dtype=bool)
        for g in range(gmin, gmax + 1):
            s0 = Q - 4 - g - len(body) + 1
            ok = s0 >= b[Q]
            for k, ch in enumerate(body):
                if ch != ".":
                    ok &= t[np.maximum(s0 + k, 0)] == ord(ch)
            hit |= ok
        ts[Q] += hit
    return hs, ts


def scores(seqs, head_lines, tail_lines):
    heads, tails = [parse(x, "head") for x in head_lines], [parse(x, "tail") for x in tail_lines]
    t, off = _csr(seqs)
    hp, tp = _strand_scores(t, off, heads, tails)
    tr, _ = _csr([revcomp(s) for s in seqs])
    hm, tm = _strand_scores(tr, off, heads, tails)
    return np.stack([hp, tp, hm, tm])


def pair(hs, ts, head_threshold, tail_threshold, len_min, len_max):
    """one strand of one sequence: (p, q, head score, tail score) per paired head, in position order"""
    tails = [int(q) for q in np.flatnonzero(ts >= tail_threshold)]
    out = []
    for p in np.flatnonzero(hs >= head_threshold):
        p = int(p)
        k = bisect.bisect_left(tails, p + len_min - 1)
        if k < len(tails) and tails[k] - p + 1 <= len_max:
            out.append((p, tails[k], int(hs[p]), int(ts[tails[k]])))
    return out


def scan(seqs, head_lines, tail_lines, head_threshold=1, tail_threshold=1, len_range=(200, 20000), stats=None):
    sc = scores(seqs, head_lines, tail_lines)
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    rec = []
    for k in range(len(seqs)):
        a, b = int(off[k]), int(off[k + 1])
        L = b - a
        for p, q, h, t in pair(sc[0, a:b], sc[1, a:b], head_threshold, tail_threshold, len_range[0], len_range[1]):
            rec.append((k, p, q + 1, 0, h, t))
        for p, q, h, t in pair(sc[2, a:b], sc[3, a:b], head_threshold, tail_threshold, len_range[0], len_range[1]):
            rec.append((k, L - 1 - q, L - p, 1, h, t))
    rec.sort(key=lambda r: (r[0], r[3], r[1], r[2]))
    if stats is not None:
        stats["anchors"] = anchors(seqs)
        stats["heads"] = int((sc[0] >= head_threshold).sum() + (sc[2] >= head_threshold).sum())
        stats["tails"] = int((sc[1] >= tail_threshold).sum() + (sc[3] >= tail_threshold).sum())
        stats["pairs"] = len(rec)
    return rec


def anchors(seqs):
    """the positions a score is computed at: TC and CT[AG][AG] on both strands"""
    n = 0
    for s in seqs:
        for x in (as_bytes(s), revcomp(s)):
            n += len(re.findall(b"(?=TC)", x)) + len(re.findall(b"(?=CT[AG][AG])", x))
    return n
