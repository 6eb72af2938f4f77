"""Inputs of the Helitron candidate scan's tests (tests/test_helitron_cases.py on the CPU, tests/test_gpu_helitron.py on the GPU).

A site is a pattern made concrete: every `.` of the body fixed to a random base, one gap of the range chosen and filled, the
literal written out.  Sites are embedded in filler text of A and T only, which holds no anchor on either strand (TC, GA, CT[AG][AG]
and [CT][CT]AG all need a C or a G), so what a case expects is exact.

A case is a dict: label, seqs (bytes), head / tail (pattern lines), kw (thresholds, len_range) and expect:
  "records": the exact records (seq, start, end, strand, head score, tail score), or None where only HIP == twin is asked;
  "scores": {(row, seq, position): score} for rows 0 plus heads, 1 plus tails, 2 minus heads, 3 minus tails (strand coordinates);
  "nonzero": per row the number of positions with a score, where the case pins it."""
import gzip
import json
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

H1, T1 = "TC.{2,4}ACG.T", "GA.CC.{1,3}CT[AG]{2}"
_LINE = {"head": re.compile(r"^TC(?:\.\{(\d+)(?:,(\d+))?\})?(.*)$"), "tail": re.compile(r"^(.*?)(?:\.\{(\d+)(?:,(\d+))?\})?CT\[AG\]\{2\}$")}


def lcv_lists():
    """the two lists of the tool's TrainingSet (tests/golden/helitron_lcvs.json.gz; tools/gen_helitron_fixture.py)"""
    with gzip.open(os.path.join(HERE, "golden", "helitron_lcvs.json.gz"), "rb") as f:
        d = json.loads(f.read().decode())
    return d["head"], d["tail"]


def split(line, side):
    """-> (gap_min, gap_max, body) of a line of either side"""
    m = _LINE[side].match(line)
    a, b, body = (m.group(1), m.group(2), m.group(3)) if side == "head" else (m.group(2), m.group(3), m.group(1))
    gmin = int(a) if a is not None else 0
    return gmin, int(b) if b is not None else gmin, body


def filler(rng, n):
    return "".join("AT"[int(x)] for x in rng.integers(0, 2, n))


def rand_dna(rng, n):
    return "".join("ACGT"[int(x)] for x in rng.integers(0, 4, n))


def revcomp(s):
    return "".join({"A": "T", "C": "G", "G": "C", "T": "A"}.get(c, "N") for c in reversed(s))


def body_of(rng, body):
    return "".join(c if c != "." else "ACGT"[int(rng.integers(0, 4))] for c in body)


def head_site(rng, line, gap=None, fill=None):
    gmin, gmax, body = split(line, "head")
    g = gmin if gap is None else gap
    return "TC" + (filler(rng, g) if fill is None else fill * g) + body_of(rng, body)


def tail_site(rng, line, gap=None, rr=None):
    gmin, gmax, body = split(line, "tail")
    g = gmin if gap is None else gap
    return body_of(rng, body) + filler(rng, g) + "CT" + (rr or "".join("AG"[int(x)] for x in rng.integers(0, 2, 2)))


def element(rng, head_line, tail_line, length, hgap=None, tgap=None):
    """a head site, filler, a tail site: `length` bases from the T of TC to the last base of CT[AG][AG]"""
    h, t = head_site(rng, head_line, hgap), tail_site(rng, tail_line, tgap)
    assert length >= len(h) + len(t)
    return h + filler(rng, length - len(h) - len(t)) + t


def case(label, seqs, head, tail, records=None, scores=None, nonzero=None, **kw):
    kw.setdefault("len_range", (20, 200))
    return {"label": label, "seqs": [s.encode() if isinstance(s, str) else s for s in seqs], "head": list(head), "tail": list(tail), "kw": kw,
            "expect": {"records": records, "scores": scores or {}, "nonzero": nonzero}}


def small_cases():
    rng = np.random.default_rng(20)
    out = []
    fl = lambda n: filler(rng, n)  # noqa: E731

    # ---- sequence length ------------------------------------------------------------------------------------------------------
    e40 = element(rng, H1, T1, 40)
    out.append(case("tiny sequences", ["", "T", "TC", "TCACG", "", e40, ""], [H1], [T1], records=[(5, 0, 40, 0, 1, 1)],
                    scores={(0, 5, 0): 1, (1, 5, 39): 1}, nonzero=[1, 1, 0, 0]))
    out.append(case("only empty sequences", ["", "", ""], [H1], [T1], records=[], nonzero=[0, 0, 0, 0]))
    # the head's body ends on the last base / needs one base more; the tail's body begins on the first base / one before it
    hs, ts = head_site(rng, H1, 2), tail_site(rng, T1, 1)
    out.append(case("body at the sequence ends", [fl(9) + hs, fl(9) + hs[:-1], ts + fl(7), ts[1:] + fl(7)], [H1], [T1], records=[],
                    scores={(0, 0, 9): 1, (0, 1, 9): 0, (1, 2, len(ts) - 1): 1, (1, 3, len(ts) - 2): 0}, nonzero=[1, 1, 0, 0]))
    # a gap range reaches past the end: the gaps that still fit count
    out.append(case("gap range cut by the end", [fl(3) + "TC" + "AAA" + "ACGAT", fl(3) + "TC" + "AAAA" + "ACGA"], [H1], [T1], records=[],
                    scores={(0, 0, 3): 1, (0, 1, 3): 0}, nonzero=[1, 0, 0, 0]))
    # a match only across the border of two neighbours: none
    out.append(case("sequence border", [fl(5) + hs[:6], hs[6:] + fl(5), ts[:4], ts[4:]], [H1], [T1], records=[], nonzero=[0, 0, 0, 0]))
    out.append(case("literal across the border", [fl(5) + "T", "C" + hs[2:], ts[:-1], ts[-1:] + fl(3)], [H1], [T1], records=[], nonzero=[0, 0, 0, 0]))

    # ---- gap range ----------------------------------------------------------------------------------------------------------------
    for g, want in ((1, 0), (2, 1), (3, 1), (4, 1), (5, 0)):
        out.append(case("head gap %d of 2..4" % g, [fl(6) + head_site(rng, H1, g) + fl(6)], [H1], [T1], records=[], scores={(0, 0, 6): want},
                        nonzero=[want, 0, 0, 0]))
    for g, want in ((0, 0), (1, 1), (3, 1), (4, 0)):
        s = fl(6) + tail_site(rng, T1, g) + fl(6)
        out.append(case("tail gap %d of 1..3" % g, [s], [H1], [T1], records=[], scores={(1, 0, len(s) - 7): want}, nonzero=[0, want, 0, 0]))
    # both ends of the range match at once (gap 2 and gap 7): still 1
    out.append(case("two gaps of the range match", [fl(4) + "TC" + "AA" + "ACGATACGAT" + fl(4)], ["TC.{2,7}ACGAT"], [T1], records=[],
                    scores={(0, 0, 4): 1}, nonzero=[1, 0, 0, 0]))
    out.append(case("no gap", [fl(4) + "TCACGTT" + fl(30) + "GATCCCTAG" + fl(4)], ["TCACG.T"], ["GA.CCCT[AG]{2}"], records=[(0, 4, 50, 0, 1, 1)]))

    # ---- limit patterns --------------------------------------------------------------------------------------------------------------
    b32 = "ACGTTGCA.C.GT.ACGGTCA.TTGACCAGTAC"[:32]
    assert len(b32) == 32 and b32[-1] != "."
    h63, t63 = "TC.{63}ACGT", "ACGT.{63}CT[AG]{2}"
    hb, tb = "TC" + b32, b32 + "CT[AG]{2}"
    e = element(rng, h63, t63, 160)
    out.append(case("gap 63", [fl(3) + e + fl(3), fl(3) + revcomp(e) + fl(3)], [h63], [t63], records=[(0, 3, 163, 0, 1, 1), (1, 3, 163, 1, 1, 1)]))
    e = element(rng, hb, tb, 90)
    out.append(case("body 32", [fl(3) + e + fl(3), revcomp(e)], [hb], [tb], records=[(0, 3, 93, 0, 1, 1), (1, 0, 90, 1, 1, 1)]))
    hx, tx = "TC.{60,63}" + b32, b32 + ".{31,63}CT[AG]{2}"
    e = element(rng, hx, tx, 200, hgap=63, tgap=63)
    out.append(case("gap 63 and body 32", [e, fl(1) + revcomp(e)], [hx], [tx], records=[(0, 0, 200, 0, 1, 1), (1, 1, 201, 1, 1, 1)]))

    # ---- non-ACGT bytes --------------------------------------------------------------------------------------------------------------
    tn = "GANCC" + "A" + "CTAG"
    out.append(case("N under a dot and in the gap", [fl(5) + "TC" + "NN" + "ACGNT" + fl(20) + tn + fl(5), fl(5) + "TC" + "nx" + "ACG-T"], [H1], [T1],
                    records=[(0, 5, 14 + 20 + 10, 0, 1, 1)], scores={(0, 1, 5): 1}))
    out.append(case("N under a letter", [fl(5) + "TC" + "AA" + "ANGAT", fl(5) + "TC" + "AA" + "ACGAN", "NACCC" + "A" + "CTAG", "GAACN" + "A" + "CTAG"],
                    [H1], [T1], records=[], nonzero=[0, 0, 0, 0]))
    out.append(case("N in the literal", [fl(5) + "TN" + "AA" + "ACGAT", fl(5) + "NC" + "AA" + "ACGAT", "GAACC" + "A" + "CNAG", "GAACC" + "A" + "CTNG",
                                         "GAACC" + "A" + "CTAN", "GAACC" + "A" + "NTAG", "GAACC" + "A" + "CTCG", "GAACC" + "A" + "CTAT"],
                    [H1], [T1], records=[], nonzero=[0, 0, 0, 0]))
    low = fl(5) + "TC" + "AA" + "ACGAT" + fl(20) + "GAACC" + "A" + "CTAG"
    out.append(case("lower case", [low.lower(), low[:5] + "tc" + low[7:], low[:9] + "AcGAT" + low[14:], low[:-4] + "CTaG", low[:-4] + "cTAG", low], [H1], [T1],
                    records=[(5, 5, len(low), 0, 1, 1)], nonzero=[3, 3, 0, 0]))

    # ---- strands ----------------------------------------------------------------------------------------------------------------------
    e = element(rng, H1, T1, 57, hgap=3, tgap=2)
    out.append(case("reverse complement", [fl(11) + e + fl(6), fl(6) + revcomp(e) + fl(11), fl(2) + revcomp(e)], [H1], [T1],
                    records=[(0, 11, 68, 0, 1, 1), (1, 6, 63, 1, 1, 1), (2, 2, 59, 1, 1, 1)]))
    # a palindromic site: the reverse complement of the element is the element, so both strands report it
    hp_, tp_ = "TC.{2}ACGTT", "AACGTCT[AG]{2}"
    half = "TCAG" + "ACGTT" + "ATTA"
    pal = half + revcomp(half)
    assert pal == revcomp(pal) and pal.endswith("AACGTCTGA")
    out.append(case("palindrome", [fl(7) + pal + fl(7)], [hp_], [tp_], len_range=(len(pal), len(pal)),
                    records=[(0, 7, 7 + len(pal), 0, 1, 1), (0, 7, 7 + len(pal), 1, 1, 1)]))

    # ---- score counting ----------------------------------------------------------------------------------------------------------------
    seven = ["TC.{2}ACG.T", "TC.{1,2}ACGAT", "TC.{2}A.G.T", "TCA.ACG", "TC.{4}GAT", "TC.{2,3}ACGA", "TC.{0,2}ACGATT"]
    site = "TC" + "AA" + "ACGATT"
    tails_ = ["GA.CC.{1}CT[AG]{2}", "GAACC.{1,2}CT[AG]{2}", "G..CCACT[AG]{2}"]
    for k in (1, 2, 7):
        s = fl(4) + site + fl(30) + "GAACC" + "A" + "CTGA" + fl(4)
        rec = [(0, 4, len(s) - 4, 0, k, 3)]
        out.append(case("score %d, threshold %d" % (k, k), [s], seven[:k], tails_, head_threshold=k, tail_threshold=3, records=rec, scores={(0, 0, 4): k}))
        out.append(case("score %d, threshold %d" % (k, k + 1), [s], seven[:k], tails_, head_threshold=k + 1, tail_threshold=3, records=[], scores={(0, 0, 4): k}))
        out.append(case("score %d, tail threshold 4" % k, [s], seven[:k], tails_, head_threshold=k, tail_threshold=4, records=[], scores={(1, 0, len(s) - 5): 3}))
    s = fl(4) + site + fl(30) + "GAACC" + "A" + "CTGA" + fl(4)
    out.append(case("a repeated line counts twice", [s, revcomp(s)], [seven[0], seven[1], seven[0]], [tails_[0], tails_[0]], head_threshold=3, tail_threshold=2,
                    records=[(0, 4, len(s) - 4, 0, 3, 2), (1, 4, len(s) - 4, 1, 3, 2)]))

    # ---- pairing ---------------------------------------------------------------------------------------------------------------------------
    for length, lr, ok in ((60, (60, 90), 1), (59, (60, 90), 0), (90, (60, 90), 1), (91, (60, 90), 0), (200, (200, 20000), 1), (199, (200, 20000), 0)):
        e = element(rng, H1, T1, length)
        s2 = [fl(8) + e + fl(8), fl(3) + revcomp(e) + fl(13)]
        out.append(case("length %d in %d..%d" % (length, lr[0], lr[1]), s2, [H1], [T1], len_range=lr,
                        records=[(0, 8, 8 + length, 0, 1, 1), (1, 3, 3 + length, 1, 1, 1)] if ok else []))
    big = element(rng, H1, T1, 20000)
    out.append(case("length 20000 and 20001", [big, revcomp(big), big[:50] + "A" + big[50:]], [H1], [T1], len_range=(200, 20000),
                    records=[(0, 0, 20000, 0, 1, 1), (1, 0, 20000, 1, 1, 1)]))
    t_a, t_b, t_c = tail_site(rng, T1, 1), tail_site(rng, T1, 2), tail_site(rng, T1, 3)
    hh = head_site(rng, H1, 2)
    s = fl(5) + hh + fl(6) + t_a + fl(10) + t_b + fl(25) + t_c + fl(5)       # the first tail is too near, the second wins over the third
    p = 5
    q_a = p + len(hh) + 6 + len(t_a)
    q_b = q_a + 10 + len(t_b)
    assert q_a - p < 30 <= q_b - p
    out.append(case("the nearer of two tails in range", [s, revcomp(s)], [H1], [T1], len_range=(30, 200),
                    records=[(0, p, q_b, 0, 1, 1), (1, len(s) - q_b, len(s) - p, 1, 1, 1)]))
    s = fl(5) + t_a + fl(20) + hh + fl(40)
    out.append(case("a tail upstream of the head", [s, revcomp(s)], [H1], [T1], len_range=(1, 200), records=[]))
    h2 = head_site(rng, H1, 4)
    s = fl(5) + hh + fl(9) + h2 + fl(30) + t_b + fl(5)
    p2 = 5 + len(hh) + 9
    q = p2 + len(h2) + 30 + len(t_b)
    out.append(case("two heads share a tail", [s, revcomp(s)], [H1], [T1],
                    records=[(0, 5, q, 0, 1, 1), (0, p2, q, 0, 1, 1), (1, len(s) - q, len(s) - p2, 1, 1, 1), (1, len(s) - q, len(s) - 5, 1, 1, 1)]))
    # several sequences with records on both strands, an empty one between them: the order (seq, strand, start, end)
    e1, e2, e3 = element(rng, H1, T1, 45), element(rng, H1, T1, 70), element(rng, H1, T1, 33)
    s0 = fl(4) + e1 + fl(9) + revcomp(e2) + fl(6) + e3 + fl(2)
    a2, a3 = 4 + 45 + 9, 4 + 45 + 9 + 70 + 6
    s1 = revcomp(e3) + fl(12) + revcomp(e1)
    out.append(case("order of the records", [s0, "", s1, fl(30), e2], [H1], [T1], len_range=(30, 80),
                    records=[(0, 4, 49, 0, 1, 1), (0, a3, a3 + 33, 0, 1, 1), (0, a2, a2 + 70, 1, 1, 1), (2, 0, 33, 1, 1, 1), (2, 45, 90, 1, 1, 1),
                             (4, 0, 70, 0, 1, 1)]))
    return out


def batch_cases():
    """the real lists (304 / 576: more than a wavefront of patterns and no multiple of 64), one pattern, none on a side"""
    rng = np.random.default_rng(21)
    head, tail = lcv_lists()
    out = []
    seqs = []
    for k in range(24):
        h, t = head[int(rng.integers(0, len(head)))], tail[int(rng.integers(0, len(tail)))]
        gh, gt = split(h, "head"), split(t, "tail")
        e = element(rng, h, t, int(rng.integers(200, 400)), hgap=int(rng.integers(gh[0], gh[1] + 1)), tgap=int(rng.integers(gt[0], gt[1] + 1)))
        s = rand_dna(rng, int(rng.integers(0, 300))) + e + rand_dna(rng, int(rng.integers(0, 300)))
        seqs.append(revcomp(s) if k % 2 else s)
    out.append(case("the tool's lists", seqs, head, tail, len_range=(200, 20000)))
    out.append(case("the tool's lists, thresholds 2 and 3", seqs, head, tail, len_range=(150, 500), head_threshold=2, tail_threshold=3))
    out.append(case("65 and 129 patterns", seqs, head[:65], tail[100:229], len_range=(100, 20000)))
    out.append(case("one pattern a side", seqs, head[:1], tail[:1], len_range=(100, 20000)))
    out.append(case("no head pattern", seqs, [], tail, records=[], nonzero=[0, None, 0, None]))
    out.append(case("no tail pattern", seqs, head, [], records=[], nonzero=[None, 0, None, 0]))
    out.append(case("no pattern", seqs, [], [], records=[], nonzero=[0, 0, 0, 0]))
    return out


def random_batch(seed, n, length):
    rng = np.random.default_rng(seed)
    return [rand_dna(rng, length) for _ in range(n)]


def volume(seed=22, n=3000, planted=40):
    """n random sequences of 100 .. 30 000 bases (log-uniform lengths), `planted` elements from the tool's lists among them
    -> (seqs, [(seq, start, end, strand)])"""
    rng = np.random.default_rng(seed)
    head, tail = lcv_lists()
    lens = np.exp(rng.uniform(np.log(100), np.log(30000), n)).astype(int)
    lens[0], lens[1] = 100, 30000
    codes = rng.integers(0, 4, int(lens.sum()), dtype=np.uint8)
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[codes].tobytes().decode()
    off = np.concatenate([[0], np.cumsum(lens)])
    seqs = [text[off[k]:off[k + 1]] for k in range(n)]
    truth = []
    long_enough = [k for k in range(n) if lens[k] >= 3000]
    for k in rng.choice(long_enough, planted, replace=False):
        k = int(k)
        h, t = head[int(rng.integers(0, len(head)))], tail[int(rng.integers(0, len(tail)))]
        e = element(rng, h, t, int(rng.integers(400, 2500)))
        minus = bool(rng.integers(0, 2))
        at = int(rng.integers(0, lens[k] - len(e) + 1))
        seqs[k] = seqs[k][:at] + (revcomp(e) if minus else e) + seqs[k][at + len(e):]
        truth.append((k, at, at + len(e), int(minus)))
    return seqs, truth


def plant_helitron_ends(g, seed=0):
    """a synth_small genome of te_type "helitron": every copy of every family gets an LCV-matching head (the first line of head.lcvs
    that has no gap range, made concrete once per family) written over its first bases and a tail over its last, on the copy's
    strand; the candidates are cut again from the first copy.  -> the genome dict, changed in place"""
    rng = np.random.default_rng(seed)
    head, tail = lcv_lists()
    chroms = [list(c) for c in g["contigs"]]
    for f, fam in enumerate(g["truth"]):
        h = head_site(rng, head[int(rng.integers(0, len(head)))])
        t = tail_site(rng, tail[int(rng.integers(0, len(tail)))])
        for (ci, s1, e1, minus) in fam:
            L = e1 - s1 + 1
            if L < len(h) + len(t):
                continue
            cur = "".join(chroms[ci][s1 - 1:e1])
            cur = revcomp(cur) if minus else cur
            cur = h + cur[len(h):L - len(t)] + t
            chroms[ci][s1 - 1:e1] = list(revcomp(cur) if minus else cur)
    g["contigs"] = ["".join(c) for c in chroms]
    return g


STAGE_SEED = 43


def stage_input(seed=STAGE_SEED, n_fam=12, per_family=4, flank=50):
    """the input of the stage script's test: a synth_small genome of Helitron families with LCV-matching ends, and the flanked repeats
    a coarse stage would hand over -- up to per_family copies of every family with `flank` bases on either side, in genome
    orientation, named c<contig>:<0-based start>-<end>  -> (genome dict, names, sequences)"""
    import synth_small

    g = plant_helitron_ends(synth_small.make(seed, n_fam=n_fam, n_chr=2, chr_len=150_000, te_type="helitron"), seed)
    names, seqs = [], []
    for fam in g["truth"]:
        for (ci, s1, e1, _minus) in fam[:per_family]:
            a, b = s1 - 1 - flank, e1 + flank
            names.append("c%d:%d-%d" % (ci, a, b))
            seqs.append(g["contigs"][ci][a:b])
    return g, names, seqs


def stage_recall(g, cand_names, tol=3):
    """candidate names <source>_<start+1>_<end>_<+|-> of the flanked repeats above -> (families with >= 3 copies, those of them with a
    candidate whose two ends are both within tol bases of one planted copy)"""
    spans = []
    for n in cand_names:
        src, s1, e1, _strand = n.rsplit("_", 3)
        ci, ab = src[1:].split(":")
        a = int(ab.split("-")[0])
        spans.append((int(ci), a + int(s1), a + int(e1)))
    fams = [fam for fam in g["truth"] if len(fam) >= 3]
    hit = 0
    for fam in fams:
        hit += any(ci == c2 and abs(s1 - a) <= tol and abs(e1 - b) <= tol for (ci, s1, e1, _m) in fam for (c2, a, b) in spans)
    return len(fams), hit
