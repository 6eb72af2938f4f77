"""CPU twin of the translated protein search (hite_amd/csrc/hite_prot.hip; the stage where the reference runs
`blastx -evalue 1e-20 -outfmt 6`, get_domain_info Util.py:4571-4612).  Test infrastructure: the product imports none of this.

Definition (every constant is part of it; the same text is in include/hite_gpu.h):
 1 translation: query in upper case; frames +1 +2 +3 read it, -1 -2 -3 its reverse complement; standard genetic code, a codon with a
   byte outside ACGT is X, a stop '*'; residue t of frame f covers bases f + 3 t .. f + 3 t + 2 of that strand, a trailing partial
   codon is dropped.  Library letters outside the 20 standard residues are X.  Proteins <= 65 535 residues, queries <= 196 605 bases.
 2 scores: '*' against anything -4, else X against anything -1, else BLOSUM62; a gap of g residues costs 11 + g.
 3 seeds: four consecutive equal standard residues (frame position i, protein position j); fewer than three distinct letters: no seed.
 4 ungapped filter: the seed extended on its diagonal to both sides; a side keeps the first position of its best running sum and
   stops at a sequence end or once the sum is MORE than 16 below the best; the segment survives with a score >= 41; equal
   (query, frame, protein, diagonal, segment) count once.
 5 tasks: per (query, frame, protein) survivors by (diagonal d = j - i, segment start, end); a survivor joins the open cluster while
   d <= c + 16 (c: the cluster's first diagonal); the cluster by segment start splits where a segment starts more than 128 after the
   largest end so far; a piece is a task: band c - 24 .. c + 39, rows max(0, first start - 128) .. min(L_f - 1, largest end + 128).
 6 gapped: best local Gotoh alignment over the task's cells; H prefers diagonal, then E (gap in the protein), then F (gap in the
   frame); a gap prefers opening; best cell = first maximum in row-major order; start / identical / columns of that path.
 7 E = m n K exp(-lambda S), lambda 0.267, K 0.041, m = query bases // 3, n = library residues, no length adjustment; smin() is the
   smallest integer S with E <= evalue in binary64.
 8 output: per (query, frame, protein) HSPs by (score desc, frame start, protein start, frame end, protein end), one dropped when it
   shares a start or an end cell with a kept one or lies inside a kept one on both sequences; 1-based coordinates, minus strand
   q_start > q_end; final order (query, score desc, protein, frame index +1 +2 +3 -1 -2 -3, q_start, s_start).

search(..., exhaustive=True) replaces steps 3-5 by the full Smith-Waterman matrix of every frame against every protein (one HSP
per pair): the yardstick of the recall measurement (tools/protein_bench.py), nothing else uses it."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

LETTERS = "ARNDCQEGHILKMFPSTWYVX*"
X, STOP = 20, 21
LAMBDA, K = 0.267, 0.041
XDROP, UNGAPPED_MIN, DIAG_JOIN, SPLIT, BAND_LO, BAND_HI = 16, 41, 16, 128, 24, 39
MAX_AA = 65535

# BLOSUM62 as NCBI prints it (rows and columns A R N D C Q E G H I L K M F P S T W Y V)
_BLOSUM62 = """
 4 -1 -2 -2  0 -1 -1  0 -2 -1 -1 -1 -1 -2 -1  1  0 -3 -2  0
-1  5  0 -2 -3  1  0 -2  0 -3 -2  2 -1 -3 -2 -1 -1 -3 -2 -3
-2  0  6  1 -3  0  0  0  1 -3 -3  0 -2 -3 -2  1  0 -4 -2 -3
-2 -2  1  6 -3  0  2 -1 -1 -3 -4 -1 -3 -3 -1  0 -1 -4 -3 -3
 0 -3 -3 -3  9 -3 -4 -3 -3 -1 -1 -3 -1 -2 -3 -1 -1 -2 -2 -1
-1  1  0  0 -3  5  2 -2  0 -3 -2  1  0 -3 -1  0 -1 -2 -1 -2
-1  0  0  2 -4  2  5 -2  0 -3 -3  1 -2 -3 -1  0 -1 -3 -2 -2
 0 -2  0 -1 -3 -2 -2  6 -2 -4 -4 -2 -3 -3 -2  0 -2 -2 -3 -3
-2  0  1 -1 -3  0  0 -2  8 -3 -3 -1 -2 -1 -2 -1 -2 -2  2 -3
-1 -3 -3 -3 -1 -3 -3 -4 -3  4  2 -3  1  0 -3 -2 -1 -3 -1  3
-1 -2 -3 -4 -1 -2 -3 -4 -3  2  4 -2  2  0 -3 -2 -1 -2 -1  1
-1  2  0 -1 -3  1  1 -2 -1 -3 -2  5 -1 -3 -1  0 -1 -3 -2 -2
-1 -1 -2 -3 -1  0 -2 -3 -2  1  2 -1  5  0 -2 -1 -1 -1 -1  1
-2 -3 -3 -3 -2 -3 -3 -3 -1  0  0 -3  0  6 -4 -2 -2  1  3 -1
-1 -2 -2 -1 -3 -1 -1 -2 -2 -3 -3 -1 -2 -4  7 -1 -1 -4 -3 -2
 1 -1  1  0 -1  0  0  0 -1 -2 -2  0 -1 -2 -1  4  1 -3 -2 -2
 0 -1  0 -1 -1 -1 -1 -2 -2 -1 -1 -1 -1 -2 -1  1  5 -2 -2  0
-3 -3 -4 -4 -2 -2 -3 -2 -2 -3 -2 -3 -1  1 -4 -3 -2 11  2 -3
-2 -2 -2 -3 -2 -1 -2 -3  2 -1 -1 -2 -1  3 -3 -2 -2  2  7 -1
 0 -3 -3 -3 -1 -2 -2 -3 -3  3  1 -2  1 -1 -2 -2  0 -3 -1  4
"""
BLOSUM62 = np.array([[int(v) for v in ln.split()] for ln in _BLOSUM62.strip().splitlines()], dtype=np.int32)
assert BLOSUM62.shape == (20, 20) and (BLOSUM62 == BLOSUM62.T).all()

# NCBI translation table 1, codons in the order TTT TTC TTA TTG TCT ... GGG (bases T C A G)
_CODE = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"
CODON = {a + b + c: _CODE[16 * i + 4 * j + k] for i, a in enumerate("TCAG") for j, b in enumerate("TCAG") for k, c in enumerate("TCAG")}
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def score(a, b):
    """residue codes -> score (step 2)"""
    if a == STOP or b == STOP:
        return -4
    if a == X or b == X:
        return -1
    return int(BLOSUM62[a, b])


TAB = np.zeros((24, 24), dtype=np.int8)
for _a in range(22):
    for _b in range(22):
        TAB[_a, _b] = score(_a, _b)


def translate6(seq):
    """-> the six frames (+1 +2 +3 -1 -2 -3) as strings"""
    s = seq.upper()
    rc = "".join(_COMP.get(c, "N") for c in reversed(s))
    out = []
    for strand in (s, rc):
        for f in range(3):
            out.append("".join(CODON.get(strand[p:p + 3], "X") for p in range(f, len(strand) - 2, 3)))
    return out


def encode(aa):
    """letters -> residue codes; anything outside the 20 standard letters (either case) is X ... except '*', which only a frame has"""
    lut = np.full(256, X, dtype=np.uint8)
    for k, ch in enumerate(LETTERS[:20]):
        lut[ord(ch)] = k
        lut[ord(ch.lower())] = k
    return lut[np.frombuffer(aa.encode("latin-1"), dtype=np.uint8)] if aa else np.zeros(0, np.uint8)


def encode_frame(aa):
    c = encode(aa)
    if len(c):
        c[np.frombuffer(aa.encode(), dtype=np.uint8) == ord("*")] = STOP
    return c


def seed_key(c):
    """four residue codes -> bucket, or -1 (step 3)"""
    if max(c) >= 20 or len(set(int(v) for v in c)) < 3:
        return -1
    return ((int(c[0]) * 20 + int(c[1])) * 20 + int(c[2])) * 20 + int(c[3])


def evalue_of(m, n, s):
    return float(m) * float(n) * K * math.exp(-LAMBDA * float(s))


def smin(m, n, evalue):
    """step 7: the smallest integer S >= 1 with m n K exp(-lambda S) <= evalue"""
    s = 1
    if m > 0 and n > 0:
        while evalue_of(m, n, s) > evalue:
            s += 1
    return s


_CLIB = None


def clib():
    """tests/protein_twin.c built with the host compiler (as tests/test_host_compiled.py builds its blocks)"""
    global _CLIB
    if _CLIB is None:
        d = tempfile.mkdtemp(prefix="protein_twin_")
        so = os.path.join(d, "protein_twin.so")
        extra = os.environ.get("HITE_HOST_CXXFLAGS", "").split()
        subprocess.run(["gcc", "-O2", "-shared", "-fPIC"] + extra + ["-o", so, os.path.join(HERE, "protein_twin.c")], check=True)
        _CLIB = C.CDLL(so)
    return _CLIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def ungapped(x, i, y, j):
    """step 4 -> (score, first frame position, last frame position)"""
    seg = np.zeros(2, dtype=np.int32)
    s = clib().twin_ungapped(_p(x), len(x), int(i), _p(y), len(y), int(j), _p(TAB), _p(seg))
    return int(s), int(seg[0]), int(seg[1])


def gapped(x, lo, hi, y, dlo, dhi):
    """step 6 -> (score, start i, start j, end i, end j, identical, columns), zeros without an alignment"""
    out = np.zeros(7, dtype=np.int32)
    rc = clib().twin_gapped(_p(x), int(lo), int(hi), _p(y), len(y), C.c_long(int(dlo)), C.c_long(int(dhi)), _p(TAB), _p(out))
    assert rc == 0
    return tuple(int(v) for v in out)


def survivors(frames, prots):
    """steps 3-4 -> sorted distinct (frame index, protein, diagonal, segment start, segment end); also the number of seed hits"""
    index = {}
    for p, y in enumerate(prots):
        for j in range(len(y) - 3):
            k = seed_key(y[j:j + 4])
            if k >= 0:
                index.setdefault(k, []).append((p, j))
    out, hits = set(), 0
    for gf, x in enumerate(frames):
        for i in range(len(x) - 3):
            k = seed_key(x[i:i + 4])
            for p, j in index.get(k, ()) if k >= 0 else ():
                hits += 1
                s, i0, i1 = ungapped(x, i, prots[p], j)
                if s >= UNGAPPED_MIN:
                    out.add((gf, p, j - i, i0, i1))
    return sorted(out), hits


def form_tasks(surv, frame_len):
    """step 5 -> [(frame index, protein, c, first row, last row)]"""
    tasks = []
    a = 0
    while a < len(surv):
        gf, p, c = surv[a][0], surv[a][1], surv[a][2]
        b = a
        while b < len(surv) and surv[b][0] == gf and surv[b][1] == p and surv[b][2] <= c + DIAG_JOIN:
            b += 1
        segs = sorted((s[3], s[4]) for s in surv[a:b])
        k = 0
        while k < len(segs):
            first, last = segs[k]
            k += 1
            while k < len(segs) and segs[k][0] - last <= SPLIT:
                last = max(last, segs[k][1])
                k += 1
            tasks.append((gf, p, c, max(0, first - SPLIT), min(frame_len[gf] - 1, last + SPLIT)))
        a = b
    return tasks


def filter_hsps(hsps):
    """step 8 on one (frame, protein) group: hsps = [(score, si, sj, ei, ej, ...)] -> those that stay, best first"""
    kept = []
    for h in sorted(hsps, key=lambda t: (-t[0], t[1], t[2], t[3], t[4])):
        bad = False
        for k in kept:
            if (h[1], h[2]) == (k[1], k[2]) or (h[3], h[4]) == (k[3], k[4]) or (h[1] >= k[1] and h[3] <= k[3] and h[2] >= k[2] and h[4] <= k[4]):
                bad = True
                break
        if not bad:
            kept.append(h)
    return kept


def search(queries, proteins, evalue=1e-20, exhaustive=False, stats=None):
    """-> [(query, protein, frame (+-1..3), q_start, q_end, s_start, s_end, raw score, identical, columns)] in the final order"""
    prots = [encode(p) for p in proteins]
    n_res = sum(len(p) for p in prots)
    frames, owner = [], []
    for q, s in enumerate(queries):
        assert len(s) <= 3 * MAX_AA
        for f, aa in enumerate(translate6(s)):
            frames.append(encode_frame(aa))
            owner.append((q, f))
    assert all(len(p) <= MAX_AA for p in prots)
    s_min = [smin(len(s) // 3, n_res, evalue) for s in queries]
    groups = {}
    if exhaustive:
        for gf, x in enumerate(frames):
            for p, y in enumerate(prots):
                if len(x) and len(y):
                    h = gapped(x, 0, len(x) - 1, y, -(1 << 40), 1 << 40)
                    if h[0] > 0:
                        groups.setdefault((gf, p), []).append(h)
    else:
        surv, hits = survivors(frames, prots)
        tasks = form_tasks(surv, [len(x) for x in frames])
        if stats is not None:
            stats.update(hits=hits, survivors=len(surv), tasks=len(tasks), task_list=tasks, survivor_list=surv)
        for gf, p, c, lo, hi in tasks:
            h = gapped(frames[gf], lo, hi, prots[p], c - BAND_LO, c + BAND_HI)
            if h[0] > 0:
                groups.setdefault((gf, p), []).append(h)
    out = []
    for (gf, p), hs in groups.items():
        q, f = owner[gf]
        L, o = len(queries[q]), f % 3
        for (sc, si, sj, ei, ej, idn, cols) in filter_hsps([h for h in hs if h[0] >= s_min[q]]):
            if f < 3:
                qs, qe = o + 3 * si + 1, o + 3 * ei + 3
            else:
                qs, qe = L - (o + 3 * si), L - (o + 3 * ei + 2)
            out.append((q, p, f, qs, qe, sj + 1, ej + 1, sc, idn, cols))
    out.sort(key=lambda r: (r[0], -r[7], r[1], r[2], r[3], r[5]))
    return [(r[0], r[1], r[2] + 1 if r[2] < 3 else -(r[2] - 2)) + r[3:] for r in out]


def outfmt6(records, qnames, pnames, query_lens, n_res):
    """the twelve `-outfmt 6` columns of the records (mismatch and gapopen are written as 0: not computed)"""
    lines = []
    for (q, p, _f, qs, qe, ss, se, sc, idn, cols) in records:
        bits = (LAMBDA * sc - math.log(K)) / math.log(2.0)
        lines.append("%s\t%s\t%.3f\t%d\t0\t0\t%d\t%d\t%d\t%d\t%.2e\t%.1f" % (qnames[q], pnames[p], 100.0 * idn / cols, cols, qs, qe, ss, se,
                                                                             evalue_of(query_lens[q] // 3, n_res, sc), bits))
    return lines
