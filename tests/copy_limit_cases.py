"""Genomes and candidates for tests/test_copy_limit_cases.py and tests/test_gpu_copy_limits.py: the copy finder of
hite_amd/csrc/hite_copies.hip outside the part tests/copy_chain_cases.py covers (sorted hits -> chains) -- the candidate minimizers
(cand_minimizer_kernel: the tile of 1024 window starts, fewer than W k-mers, the sampling rule), the occurrence limit of occ_kernel,
the borders of the per-candidate sort classes and the join across chunks of 64 hits, chain_class at EXT_MAXLEN and EXT_LONG, the end
extension on the device (contig ends, N, the band's edge, the refill of idle lanes), the two 95 % filters at equality, both interval
modes at contig ends, and the cap of 300 copies with its order.  Seeded, pure python + numpy; no GPU and no twin in this file.

THE MODEL restates the first half of the definition in the header of oracle/hite_oracle_copies.c with python integers: the
minimizers of seed_limit_cases (K = 15, W = 10), the sampling rule of the candidate's minimizers (kept()), the index as a dict
hs >> 1 -> entries, the hits of every kept minimizer with at most MAXOCC entries, and (for the builders only) the diagonal clusters
with their extreme anchors.  It gives copy_stats_ext()[0] and [1] of a call; clusters [2], copies before the cap [3] and chains
[4] + [5] are carried by the cases as closed forms of their construction.  The twin is the definition of the table: the model only
proves that a case sits on the edge it is named for (every builder asserts it and lists it in `events`).

A unit between runs of N has the same minimizers wherever it stands, and every window of a candidate that IS the unit is a window
of the genome's copy: each of the candidate's m minimizers occurs once per copy (arrays: m n hits, one cluster per copy when the
copies are more than TD apart, ONE cluster when they follow each other within TD)."""
import bisect
import re

import numpy as np

import seed_limit_cases as SC
from seed_limit_cases import rand_seq, revcomp

K, W = SC.K, SC.W
MAXOCC, TD, MINANCH, MAXCOPY = 2000, 64, 3, 300
SUB_EDGE, SUB_UNIT, SUB_MAX = 256, 1024, 4
EXT_B, EXT_MAXLEN, EXT_LONG = 8, 2048, 384
CM_TILE = 1024                         # cand_minimizer_kernel: window starts per tile
HS_SMALL, HS_MID, HS_MEDIUM = 2048, 4096, 8192
BASES = SC.BASES


# ------------------------------------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------------------------------------
def kept(L, pos, hs):
    """cand_minimizer_kept of the twin: is the candidate minimizer (pos, hs) of a candidate of L bases looked up"""
    S = min(SUB_MAX, L // SUB_UNIT)
    if S <= 1 or pos < SUB_EDGE or pos + K > L - SUB_EDGE:
        return True
    return (hs >> 1) % S == 0


def sampled(L, pos):
    """does the hash decide about the minimizer at pos (not: is it kept)"""
    return min(SUB_MAX, L // SUB_UNIT) > 1 and not (pos < SUB_EDGE or pos + K > L - SUB_EDGE)


def kept_minimizers(seq):
    """[(pos, hs)] the candidate's minimizers that are looked up, in position order"""
    return [(p, hs) for p, hs, _w in SC.minimizers(seq) if kept(len(seq), p, hs)]


def window_choice(seq):
    """per window of seq the position of its minimizer (None: no valid k-mer), from the (position, first window) list"""
    nk = len(seq) - K + 1
    nwin = nk - W + 1 if nk >= W else (1 if nk > 0 else 0)
    out, mins, j, cur = [], SC.minimizers(seq), 0, None
    for w in range(nwin):
        while j < len(mins) and mins[j][2] <= w:
            cur = mins[j][0]
            j += 1
        # (a window without a valid k-mer: every k-mer start p .. p + W - 1 overlaps a base outside ACGT)
        out.append(cur if cur is not None and w <= cur < w + W else None)
    return out


_seg_memo = {}
_PAD = K + W - 1


def contig_minimizers(s):
    """[(pos, hs)] == [(p, hs) for p, hs, _ in SC.minimizers(s)].  A run of >= W N's leaves >= W + K - 1 k-mer starts in a row without
    a valid k-mer: no window sees both sides, and every window that sees one side exists whatever the run's length.  The contig is cut
    at such runs and a piece is computed once between pads of N (the arrays of this file repeat one piece thousands of times)."""
    if len(s) < 400 or "N" * W not in s:
        return [(p, hs) for p, hs, _w in SC.minimizers(s)]
    out, a = [], 0
    cuts = [m.span() for m in re.finditer("N{%d,}" % W, s)] + [(len(s), len(s))]
    for lo, hi in cuts:
        if lo > a:
            key = (s[a:lo], a > 0, lo < len(s))
            if key not in _seg_memo:
                t = ("N" * _PAD if key[1] else "") + key[0] + ("N" * _PAD if key[2] else "")
                _seg_memo[key] = [(p - (_PAD if key[1] else 0), hs) for p, hs, _w in SC.minimizers(t)]
            out += [(a + p, hs) for p, hs in _seg_memo[key]]
        a = hi
    return out


def index_of(contigs):
    """-> (coff, {hs >> 1: [(global position, hs)]})"""
    coff = [0]
    for s in contigs:
        coff.append(coff[-1] + len(s))
    idx = {}
    for c, s in enumerate(contigs):
        for p, hs in contig_minimizers(s):
            idx.setdefault(hs >> 1, []).append((coff[c] + p, hs))
    return coff, idx


def hits_of(index, cand):
    """-> (kept minimizers, [(rel, d, qo, gpos)]) of one candidate"""
    _coff, idx = index
    L = len(cand)
    km = kept_minimizers(cand)
    hits = []
    for p, hs in km:
        occ = idx.get(hs >> 1, ())
        if len(occ) > MAXOCC:
            continue
        for gpos, ghs in occ:
            rel = (hs ^ ghs) & 1
            qo = L - p - K if rel else p
            hits.append((rel, gpos - qo, qo, gpos))
    return km, hits


def clusters_of(index, cand):
    """the diagonal clusters of one candidate (for the builders; the kernels' clusters are compared with the twin's tables):
    [dict(rel, contig, na, qlo, glo, qhi, ghi)]"""
    coff = index[0]
    _km, hits = hits_of(index, cand)
    hits.sort(key=lambda h: (h[0], h[1]))
    contig = lambda g: bisect.bisect_right(coff, g, 1, len(coff) - 1) - 1      # noqa: E731
    out = []
    for i, h in enumerate(hits):
        p = hits[i - 1] if i else None
        if p is None or p[0] != h[0] or contig(p[3]) != contig(h[3]) or h[1] - p[1] > TD:
            out.append({"rel": h[0], "contig": contig(h[3]), "na": 0, "lo": (h[2], h[3]), "hi": (h[2], h[3])})
        cl = out[-1]
        cl["na"] += 1
        cl["lo"] = min(cl["lo"], (h[2], h[3]))
        cl["hi"] = max(cl["hi"], (h[2], h[3]))
    for cl in out:
        (cl["qlo"], cl["glo"]), (cl["qhi"], cl["ghi"]) = cl.pop("lo"), cl.pop("hi")
        cl["span_ok"] = (cl["qhi"] + K - cl["qlo"]) * 100 >= 95 * (cl["ghi"] + K - cl["glo"])
    return out


def model(case):
    """-> dict(kept: per candidate count == stats[0] of the candidate searched alone, hits: per candidate == stats[1] alone)"""
    index = index_of(case["contigs"])
    kept_n, hits_n = [], []
    for q in case["cands"]:
        km, hits = hits_of(index, q)
        kept_n.append(len(km))
        hits_n.append(len(hits))
    return {"kept": kept_n, "hits": hits_n}


# ------------------------------------------------------------------------------------------------------------------------------
# building blocks
# ------------------------------------------------------------------------------------------------------------------------------
def unit(rng, n, m, both=True, also=None):
    """n random bases with exactly m minimizers (all looked up: n < 2048), the same for the reverse complement; `also`: a further test"""
    for _try in range(100_000):
        u = rand_seq(rng, n)
        if len(SC.minimizers(u)) == m and (not both or len(SC.minimizers(revcomp(u))) == m) and (also is None or also(u)):
            return u
    raise AssertionError("no unit of %d bases with %d minimizers" % (n, m))


def worn(rng, s, upto, step=14, first=3):
    """s with a substitution every `step` bases below `upto`: no 15-mer of that part survives, the end extension aligns through it"""
    t = list(s)
    for i in range(first, upto, step):
        t[i] = BASES[(BASES.index(t[i]) + 1 + int(rng.integers(0, 3))) % 4]
    return "".join(t)


def other_base(*avoid):
    return next(b for b in BASES if b not in avoid)


def spaced(rng, pieces, gap=600):
    """the pieces in unique sequence, `gap` bases apart"""
    return rand_seq(rng, gap) + "".join(p + rand_seq(rng, gap) for p in pieces)


CASES = {}
_memo = {}


def case(group):
    def reg(fn):
        CASES[fn.__name__] = (group, fn)
        return fn
    return reg


def get(name):
    if ("case", name) not in _memo:
        c = CASES[name][1]()
        c["name"], c["group"] = name, CASES[name][0]
        c.setdefault("aligned", True)
        c.setdefault("alone", [])
        _memo[("case", name)] = c
    return _memo[("case", name)]


def model_of(name):
    if ("model", name) not in _memo:
        _memo[("model", name)] = model(get(name))
    return _memo[("model", name)]


def names(group=None):
    return [n for n, (g, _f) in CASES.items() if group is None or g == group]


def all_cases():
    """[(name, case)] in a fixed order; hit_classes first: HITE_HIT_HIST prints the classes of a process's FIRST call"""
    return [(n, get(n)) for n in names()]


# ---- 2. occurrences and hit classes (first: see all_cases) ----------------------------------------------------------------------
@case("hits")
def hit_classes():
    """six candidates with exactly 2048, 2049, 4096, 4097, 8192 and 8193 hits: units of 8 minimizers in arrays of 256, 512 and 1024
    copies (70 N between two copies: every copy its own cluster), and the unit + N + a 15-mer of unique sequence that is a minimizer
    of the genome (one more minimizer, one more hit).  Classes <= 2048, <= 4096, <= 8192, above: 1, 2, 2, 1 candidates"""
    rng = np.random.default_rng(720)
    uniq = rand_seq(rng, 3000)
    vs = [uniq[p:p + K] for p, _hs, _w in SC.minimizers(uniq)[20:80:20]]
    contigs, cands = [], []
    for n, v in zip((256, 512, 1024), vs):
        u = unit(rng, 60, 8, both=False, also=lambda x: len(SC.minimizers(x + "N" + v)) == 9)
        contigs.append(("N" * 70).join([u] * n))
        cands += [u, u + "N" + v]
    contigs.append(uniq)
    c = {"contigs": contigs, "cands": cands, "alone": list(range(6)), "rows": {0: 256, 2: 300, 4: 300}}
    m = model(c)
    want = [HS_SMALL, HS_SMALL + 1, HS_MID, HS_MID + 1, HS_MEDIUM, HS_MEDIUM + 1]
    assert m["hits"] == want, m["hits"]
    c["events"] = ["hits == %d" % h for h in want]
    return c


def _array(seed, n, gap=70, m=5, ulen=60):
    rng = np.random.default_rng(seed)
    u = unit(rng, ulen, m)
    return u, ("N" * gap).join([u] * n)


def _array_case(n):
    """n copies of a unit of 5 minimizers, 70 N apart (spacing 130 > TD: a cluster per copy): every minimizer of the unit has n index
    entries.  n <= 2000: 5 n hits per strand, n chains, 300 copies; n = 2001: not looked up, nothing"""
    u, contig = _array(730, n)
    c = {"contigs": [contig], "cands": [u, revcomp(u)]}
    ok = n <= MAXOCC
    m = model(c)
    assert m["kept"] == [5, 5] and m["hits"] == ([5 * n] * 2 if ok else [0, 0]), m
    c["rows"] = {0: MAXCOPY if ok else 0, 1: MAXCOPY if ok else 0}
    c["stats"] = {"clusters": 2 * n if ok else 0, "copies": 2 * n if ok else 0, "chains": 2 * n if ok else 0}
    c["events"] = ["occ == %d" % n] + (["a call with >= 2000 chains"] if ok else [])
    return c


@case("hits")
def array_1999():
    return _array_case(MAXOCC - 1)


@case("hits")
def array_2000():
    return _array_case(MAXOCC)


@case("hits")
def array_2001():
    return _array_case(MAXOCC + 1)


def _dense(cut):
    """600 copies of a unit of 54 bases and 8 minimizers, 10 N apart: the 8 hits of a copy share a diagonal and the next copy's lies
    exactly TD = 64 further: ONE cluster of 4800 hits across 75 chunks of 64, whose genome span forbids a chain; `cut`: a contig end
    between copy 300 and 301: two clusters"""
    u, arr = _array(740, 600, gap=10, m=8, ulen=54)
    rng = np.random.default_rng(741)
    head, tail = rand_seq(rng, 500) + "N" * 10, "N" * 10 + rand_seq(rng, 500)
    half = 300 * 64
    contigs = [head + arr[:half], arr[half:] + tail] if cut else [head + arr + tail]
    c = {"contigs": contigs, "cands": [u], "rows": {0: 0}, "stats": {"clusters": 2 if cut else 1, "copies": 0, "chains": 0}}
    cl = clusters_of(index_of(contigs), u)
    assert [x["na"] for x in cl] == ([2400, 2400] if cut else [4800]) and not any(x["span_ok"] for x in cl), cl
    c["events"] = ["one run of 4800 hits cut by a contig end" if cut else "one run of 4800 hits, diagonal steps of exactly TD"]
    return c


@case("hits")
def dense_array():
    return _dense(False)


@case("hits")
def dense_array_cut():
    return _dense(True)


# ---- 1. candidate minimizers ----------------------------------------------------------------------------------------------------
def _sampling_element(rng):
    """an element and a cut (s, L >= 4096) of it with minimizers at 255 (kept by the edge rule, dropped if the hash decided), at
    L - 271 (pos + 15 == L - 256: the hash decides) and at L - 270 (pos + 15 == L - 255: kept by the edge rule, dropped by the hash)"""
    for _try in range(200):
        E = rand_seq(rng, 6400)
        mins = {p: hs for p, hs, _w in SC.minimizers(E)}
        for p in sorted(mins):
            if p < 4600 or p + 1 not in mins or (mins[p + 1] >> 1) % SUB_MAX == 0:
                continue
            for q in sorted(mins):
                s, L = q - 255, p - (q - 255) + 271
                if 255 <= q < 700 and (mins[q] >> 1) % SUB_MAX and q + 1 in mins and s + L <= len(E) - 20 and L >= 4 * SUB_UNIT:
                    return E, s, L
    raise AssertionError("no element with minimizers on the edges of the sampling rule")


MIN_LENGTHS = (14, 15, 16, 23, 24, 25, 1046, 1047, 1048, 2071, 2072, 2047, 2048, 3071, 3072, 4095, 4096, 5119, 5120)


@case("minimizers")
def minimizer_limits():
    """candidates cut from a planted element (copies on both strands): no k-mer, one k-mer, fewer than W k-mers, exactly W, two
    windows; 1023, 1024, 1025, 2048 and 2049 windows against the tile of 1024 window starts; windows 1023 and 1024 choosing the same
    k-mer and different ones; S = 1 -> 2 -> 3 -> 4 -> 4 of the sampling rule; minimizers on both sides of both of its edges; N at
    position 0, at L - 1 and in a run of 15 across window 1024"""
    rng = np.random.default_rng(701)
    E, s_samp, L_samp = _sampling_element(rng)
    contigs = [spaced(rng, [E, revcomp(E)], 1500), spaced(rng, [revcomp(E)], 1200)]
    cands, ev = [], []
    for k, L in enumerate(MIN_LENGTHS):
        o = 40 + 13 * k
        cands.append(E[o:o + L])
        ev.append("candidate of %d bases" % L)
    choice = window_choice(E)
    same = next(s for s in range(100, 3000) if choice[s + CM_TILE - 1] == choice[s + CM_TILE])
    diff = next(s for s in range(100, 3000) if choice[s + CM_TILE - 1] != choice[s + CM_TILE])
    for s, name in ((same, "same"), (diff, "different")):
        q = E[s:s + 1500]
        ch = window_choice(q)
        assert (ch[CM_TILE - 1] == ch[CM_TILE]) == (name == "same") and ch[CM_TILE] is not None
        assert sum(1 for p, _hs, w in SC.minimizers(q) if w == CM_TILE) == (0 if name == "same" else 1)
        cands.append(q)
        ev.append("windows 1023 and 1024 choose %s k-mer" % ("the same" if name == "same" else "different"))
    # the edges of the sampling rule
    q = E[s_samp:s_samp + L_samp]
    L = len(q)
    mins = {p: hs for p, hs, _w in SC.minimizers(q)}
    assert L >= 4 * SUB_UNIT and 255 in mins and not sampled(L, 255) and (mins[255] >> 1) % SUB_MAX
    assert any(p >= 256 and sampled(L, p) for p in mins)
    assert L - 271 in mins and sampled(L, L - 271) and L - 270 in mins and not sampled(L, L - 270) and (mins[L - 270] >> 1) % SUB_MAX
    inner = [kept(L, p, hs) for p, hs in mins.items() if sampled(L, p)]
    assert any(inner) and not all(inner)
    cands.append(q)
    ev += ["minimizer at 255 kept, at >= 256 sampled", "minimizer with pos + 15 == L - 256 sampled, == L - 255 kept",
           "interior minimizers dropped and kept"]
    # N
    qn = list(E[400:2000])
    qn[CM_TILE:CM_TILE + K] = "N" * K
    qn = "".join(qn)
    assert window_choice(qn)[CM_TILE] is None and window_choice(qn)[CM_TILE - 1] is None
    cands += ["N" + E[201:1401], E[300:1500] + "N", qn]
    ev += ["N at position 0", "N at L - 1", "15 N across window 1024"]
    for L in (2047, 2048, 3072, 4096, 5120):
        ev.append("S == %d" % min(SUB_MAX, L // SUB_UNIT))
    c = {"contigs": contigs, "cands": cands, "alone": list(range(len(cands))), "events": ev}
    # every candidate matches the three copies base for base: a row per cluster of >= 3 anchors, with the anchors the MODEL counts
    # (the sampling rule decides how many a copy has)
    index = index_of(contigs)
    c["row_anchors"] = {k: sorted(x["na"] for x in clusters_of(index, q) if x["na"] >= MINANCH) for k, q in enumerate(cands)}
    assert sum(1 for v in c["row_anchors"].values() if len(v) == 3) >= len(cands) - 8
    return c


# ---- 3. chain rules -------------------------------------------------------------------------------------------------------------
def _first_anchor(index, q):
    """qlo of the forward chain with the most anchors"""
    cl = [x for x in clusters_of(index, q) if x["rel"] == 0 and x["na"] >= MINANCH]
    return max(cl, key=lambda x: x["na"])["qlo"]


@case("chains")
def ext_maxlen():
    """an element of 2960 bases, copies on both strands; the candidates' first bases carry a substitution every 14 bases, so that the
    outermost anchor lies at qlo = 2047, 2048 (a chain: found on both strands, through the left end and, against the copy on the
    other strand, through the right end) and 2049 (no chain); the same for the reverse complements"""
    rng = np.random.default_rng(750)
    X = rand_seq(rng, 2960)
    contigs = [spaced(rng, [X, revcomp(X)], 900)]
    index = index_of(contigs)
    w = worn(rng, X, 2085)
    q0 = _first_anchor(index, w[10:])
    cands, ev = [], []
    for t in (EXT_MAXLEN - 1, EXT_MAXLEN, EXT_MAXLEN + 1):
        q = w[10 + q0 - t:]
        cl = [x for x in clusters_of(index, q) if x["na"] >= MINANCH]
        assert len(cl) == 2 and all(x["span_ok"] for x in cl), cl
        assert {x["rel"]: (x["qlo"] if x["rel"] == 0 else len(q) - x["qhi"] - K) for x in cl} == {0: t, 1: t}, (t, cl)
        cands.append(q)
        ev += ["left end of %d bases" % t, "right end of %d bases" % t]
    cands += [revcomp(q) for q in cands]
    rows = {0: 2, 1: 2, 2: 0, 3: 2, 4: 2, 5: 0}
    return {"contigs": contigs, "cands": cands, "alone": list(range(6)), "rows": rows, "events": ev}


@case("chains")
def ext_long():
    """ONE forward copy of an element of 1000 bases; candidates with an end of 383 and of 384 bases beyond the outermost anchor:
    searched alone, the one is listed among the other chains, the second among the long ones"""
    rng = np.random.default_rng(751)
    Y = rand_seq(rng, 1000)
    contigs = [spaced(rng, [Y], 700)]
    index = index_of(contigs)
    w = worn(rng, Y, 425)
    q0 = _first_anchor(index, w[10:])
    cands = []
    for t in (EXT_LONG - 1, EXT_LONG):
        q = w[10 + q0 - t:]
        cl = [x for x in clusters_of(index, q) if x["na"] >= MINANCH]
        assert len(cl) == 1 and cl[0]["qlo"] == t and len(q) - cl[0]["qhi"] - K < 20 and cl[0]["span_ok"], cl
        cands.append(q)
    return {"contigs": contigs, "cands": cands, "alone": [0, 1], "rows": {0: 1, 1: 1}, "alone_stats": {0: {"long": 0, "short": 1}, 1: {"long": 1, "short": 0}},
            "events": ["end of 383 bases", "end of 384 bases"]}


@case("chains")
def anchors_2_and_3():
    """units with 2 and with 3 minimizers, four copies each between N's: clusters of exactly 2 (no copy) and exactly 3 anchors"""
    rng = np.random.default_rng(752)
    u2, u3 = unit(rng, 30, 2), unit(rng, 38, 3)
    contig = rand_seq(rng, 300)
    for k in range(4):
        contig += "N" * 100 + (u2 if k % 2 else revcomp(u2)) + "N" * 100 + (revcomp(u3) if k % 2 else u3)
    contig += "N" * 100 + rand_seq(rng, 300)
    cands = [u2, u3, revcomp(u2), revcomp(u3)]
    index = index_of([contig])
    for q, na in zip(cands, (2, 3, 2, 3)):
        cl = clusters_of(index, q)
        assert [x["na"] for x in cl] == [na] * 4 and all(x["span_ok"] for x in cl), cl
    return {"contigs": [contig], "cands": cands, "alone": [0, 1, 2, 3], "rows": {0: 0, 1: 4, 2: 0, 3: 4},
            "stats": {"clusters": 16, "chains": 8, "copies": 8}, "events": ["clusters of exactly 2 anchors", "clusters of exactly 3 anchors"]}


@case("chains")
def span_rule():
    """(qhi + K - qlo) 100 >= 95 (ghi + K - glo) AT EQUALITY: a candidate whose outermost minimizers span 969 = 19 x 51 bases, a copy
    with ONE insertion of 51 bases between them (96 900 >= 96 900: a chain) and one with 52 (96 900 < 96 995: none), both strands"""
    rng = np.random.default_rng(753)
    q = None
    for _try in range(400):
        E = rand_seq(rng, 985)
        mins = SC.minimizers(E)
        a = mins[0][0]
        b = next((p for p, _hs, _w in mins if p + K - a == 969), None)
        if b is None:
            continue
        # cut behind the first window that chooses the k-mer at b: it is the candidate's last minimizer
        q = next((E[:b + K + x] for x in range(W) if SC.minimizers(E[:b + K + x])[-1][0] == b), None)
        if q is not None:
            break
    mins = SC.minimizers(q)
    assert mins[0][0] == a and mins[-1][0] == b and b + K - a == 969, (a, b, mins[-1])
    g51 = q[:480] + rand_seq(rng, 51) + q[480:]
    g52 = q[:480] + rand_seq(rng, 52) + q[480:]
    contigs = [spaced(rng, [g51, g52], 700), spaced(rng, [revcomp(g52), revcomp(g51)], 700)]
    index = index_of(contigs)
    for cand in (q, revcomp(q)):
        cl = [x for x in clusters_of(index, cand) if x["na"] >= MINANCH]
        gs = sorted((x["ghi"] + K - x["glo"], x["span_ok"]) for x in cl)
        assert gs == [(1020, True), (1020, True), (1021, False), (1021, False)], gs
        assert all(x["qhi"] + K - x["qlo"] == 969 for x in cl)
    return {"contigs": contigs, "cands": [q, revcomp(q)], "alone": [0, 1], "rows": {0: 2, 1: 2}, "stats": {"chains": 4, "copies": 4},
            "events": ["span rule at equality", "span rule one base short"]}


# ---- 4. end extension on the device ----------------------------------------------------------------------------------------------
OVERHANGS = (0, 1, 2, 7, 8, 9, 16, 17, 30, 31)
_OVER_LEN = 600


def _overhang_element():
    if "overhang element" not in _memo:
        rng = np.random.default_rng(760)
        for _try in range(2000):
            E = rand_seq(rng, _OVER_LEN)
            # (the k-mer at 9 is the choice of windows 0, 1 and 2: it stays the first anchor when 1 or 2 bases are cut off)
            if all(m[0][0] == 9 and m[1][2] >= 3 for m in (SC.minimizers(E), SC.minimizers(revcomp(E)))):
                break
        else:
            raise AssertionError("no element with its first minimizers at 9")
        _memo["overhang element"] = E
    return _memo["overhang element"]


def _overhang(v, aligned):
    """a 600-base element whose first minimizers lie at 9 from either end, planted so that v of its bases hang over: the START of contig
    0 (global position 0), an inner contig end whose neighbour contig CONTINUES the element (right side: contigs 1 | 2, left side:
    3 | 4), and the END of the last contig (the other strand).  Nothing lies beyond a contig's end: the clip is exactly v, on the side
    of the genome the contig ends at; 570 x 100 = 95 x 600 keeps v = 30 (the first filter at equality), v = 31 is dropped.  The
    outermost anchor is 9 - v bases from the contig's end for v = 0, 1, 2: the band of +-8 meets the end in its first columns"""
    E = _overhang_element()
    rng = np.random.default_rng(761 + v)
    R = [rand_seq(rng, 700) for _ in range(6)]
    n = _OVER_LEN - v
    contigs = [E[v:] + R[0], R[1] + E[:n], E[n:] + R[2], R[3] + E[:v], E[v:] + R[4], R[5] + revcomp(E)[:n]]
    found = v * 100 <= 5 * _OVER_LEN
    c = {"contigs": contigs, "cands": [E, revcomp(E)], "aligned": aligned, "rows": {0: 4 if found else 0, 1: 4 if found else 0}}
    if found and aligned:
        c["clips"] = {0: v, 1: v << 16, 4: v, 5: v << 16}         # contig -> clip word (left | right << 16, in the genome's orientation)
    index = index_of(contigs)
    cl = [x for x in clusters_of(index, E) if x["na"] >= MINANCH and x["contig"] == 0]
    assert len(cl) == 1
    c["events"] = ["overhang %d, %s interval" % (v, "aligned" if aligned else "whole-candidate")]
    if v <= 2:
        assert cl[0]["glo"] == 9 - v, cl
        c["events"].append("outermost anchor %d bases from the contig's end" % (9 - v))
    if v == 30:
        c["events"].append("first filter at equality")
    if v == 31:
        c["events"].append("first filter one base short")
    return c


def _overhang_builder(v, aligned):
    def build():
        return _overhang(v, aligned)
    build.__name__ = "overhang_%d_%s" % (v, "aligned" if aligned else "whole")
    build.__doc__ = _overhang.__doc__
    return build


for _v in OVERHANGS:
    for _al in (True, False):
        case("extension")(_overhang_builder(_v, _al))


@case("extension")
def band_and_n():
    """a candidate whose first 300 bases are worn (the left extension walks them), against copies with 8 and 9 bases deleted and
    inserted in the middle of that end (the band of +-8 follows 8 and loses 9), with an N in the genome 5, 8 and 9 bases beyond the
    outermost anchor, and intact; the candidate's reverse complement; the candidate with an N inside its worn end"""
    rng = np.random.default_rng(770)
    D = rand_seq(rng, 1500)
    w = worn(rng, D, 300)
    q0 = _first_anchor(index_of([spaced(rng, [D], 200)]), w)
    assert 280 <= q0 <= 320
    copies = [D[:150] + D[150 + EXT_B:], D[:150] + D[150 + EXT_B + 1:], D[:150] + rand_seq(rng, EXT_B) + D[150:],
              D[:150] + rand_seq(rng, EXT_B + 1) + D[150:], D]
    for k in (5, 8, 9):
        copies.append(D[:q0 - 1 - k] + "N" + D[q0 - k:])
    contigs = [spaced(rng, copies[:4], 500), spaced(rng, [revcomp(x) for x in copies[4:]], 500)]
    wn = w[:100] + "N" + w[101:]
    index = index_of(contigs)
    assert sorted(x["qlo"] for x in clusters_of(index, w) if x["na"] >= MINANCH and x["rel"] == 0) == [q0] * 4
    assert sum(1 for x in clusters_of(index, w) if x["na"] >= MINANCH and x["rel"] == 1 and len(w) - x["qhi"] - K == q0) == 4
    return {"contigs": contigs, "cands": [w, revcomp(w), wn], "alone": [0, 1, 2], "rows": {0: 6, 1: 6, 2: 6}, "stats": {"chains": 24, "copies": 18},
            "events": ["indel of 8 bases in an end", "indel of 9 bases in an end", "genome N 5, 8 and 9 bases beyond the outermost anchor",
                       "candidate N inside a worn end"]}


@case("extension")
def chain_counts():
    """calls whose chain table holds exactly 1, 32 and 33 chains (2, 64 and 66 tasks: one wavefront filled once, then refilled):
    elements of 200 bases with that many forward copies, each candidate searched alone"""
    rng = np.random.default_rng(771)
    els = [rand_seq(rng, 200) for _ in range(3)]
    contig = rand_seq(rng, 300)
    for e, n in zip(els, (1, 32, 33)):
        contig += ("N" * 40 + e) * n
    contig += "N" * 40 + rand_seq(rng, 300)
    return {"contigs": [contig], "cands": els, "alone": [0, 1, 2], "rows": {0: 1, 1: 32, 2: 33},
            "alone_stats": {0: {"chains": 1}, 1: {"chains": 32}, 2: {"chains": 33}}, "stats": {"chains": 66, "copies": 66, "clusters": 66},
            "events": ["1 chain", "32 chains", "33 chains"]}


# ---- 5. filters, cap, order -------------------------------------------------------------------------------------------------------
def _stretched(rng, f, per_end=7, step=12):
    """f with one base inserted every 12 bases in its first and last 84: no 15-mer of the ends survives (the anchors lie in the middle)
    and each end extension crosses 7 insertions, inside the band of +-8"""
    out, L = list(f), len(f)
    at = sorted([6 + step * i for i in range(per_end)] + [L - 6 - step * i for i in range(per_end)], reverse=True)
    for p in at:
        out.insert(p, other_base(f[p - 1], f[p]))
    return "".join(out)


@case("filters")
def second_filter():
    """aligned 100 >= 95 (a1 - a0) at equality: a candidate of 266 = 19 x 14 bases against a copy with 14 inserted bases, all beyond
    the outermost anchors (26 600 >= 95 x 280: kept), and one of 265 bases (26 500 < 95 x 279 = 26 505: dropped); both strands"""
    rng = np.random.default_rng(780)
    f, f2 = rand_seq(rng, 266), rand_seq(rng, 265)
    contigs = [spaced(rng, [_stretched(rng, f), _stretched(rng, f2), revcomp(_stretched(rng, f)), revcomp(_stretched(rng, f2))], 500)]
    cands = [f, f2, revcomp(f), revcomp(f2)]
    index = index_of(contigs)
    for q in cands:
        cl = [x for x in clusters_of(index, q) if x["na"] >= MINANCH]
        assert len(cl) == 2 and all(x["span_ok"] and x["qlo"] >= 78 and x["qhi"] + K <= len(q) - 78 for x in cl), cl
    return {"contigs": contigs, "cands": cands, "rows": {0: 2, 1: 0, 2: 2, 3: 0}, "stats": {"chains": 8, "copies": 4},
            "events": ["second filter at equality", "second filter one base short"]}


@case("filters")
def cap_299_300_301():
    """299, 300 and 301 accepted copies of three 200-base elements"""
    rng = np.random.default_rng(781)
    els = [rand_seq(rng, 200) for _ in range(3)]
    contigs = []
    for e, n in zip(els, (MAXCOPY - 1, MAXCOPY, MAXCOPY + 1)):
        contigs.append(rand_seq(rng, 100) + ("N" * 30 + e) * n + "N" * 30 + rand_seq(rng, 100))
    return {"contigs": contigs, "cands": els, "rows": {0: MAXCOPY - 1, 1: MAXCOPY, 2: MAXCOPY},
            "stats": {"chains": 3 * MAXCOPY, "copies": 3 * MAXCOPY, "clusters": 3 * MAXCOPY}, "events": ["299 copies", "300 copies", "301 copies"]}


@case("filters")
def cap_order():
    """320 copies of one 200-base candidate in two contigs: 10 intact (A anchors), 10 with one substitution (A - 1), 300 with two
    (A - 2), mixed: the cut at 300 falls INSIDE the group of A - 2 anchors, where the global start decides (280 of its 300 stay:
    all of contig 0's and the first of contig 1's)"""
    rng = np.random.default_rng(782)
    for _try in range(200):
        C = rand_seq(rng, 200)
        mins = [p for p, _hs, _w in SC.minimizers(C)]
        cover = lambda x: [p for p in mins if p <= x < p + K]        # noqa: E731
        single = [x for x in range(40, 160) if len(cover(x)) == 1]
        pair = next(((x, y) for x in single for y in single if y > x + 2 * K and cover(x) != cover(y)), None)
        if pair is None:
            continue
        sub = lambda s, x: s[:x] + other_base(s[x]) + s[x + 1:]      # noqa: E731
        v1, v2 = sub(C, pair[0]), sub(sub(C, pair[0]), pair[1])
        probe = index_of(["N" * 30 + C + "N" * 30 + v1 + "N" * 30 + v2 + "N" * 30])
        na = [x["na"] for x in clusters_of(probe, C)]
        if na == [len(mins), len(mins) - 1, len(mins) - 2]:
            break
    else:
        raise AssertionError("no candidate with substitutions that cost exactly one and two anchors")
    kinds = [C] * 5 + [v1] * 5 + [v2] * 150
    contigs = []
    for _c in range(2):
        order = rng.permutation(len(kinds))
        contigs.append(rand_seq(rng, 100) + "".join("N" * 30 + kinds[i] for i in order) + "N" * 30 + rand_seq(rng, 100))
    return {"contigs": contigs, "cands": [C], "rows": {0: MAXCOPY}, "stats": {"chains": 320, "copies": 320, "clusters": 320},
            "anchors": (len(mins), len(mins) - 1, len(mins) - 2), "events": ["cut inside a group of equal anchors", "copies in two contigs"]}


# every edge the case set must reach: a builder lists an event only after asserting it with the model
REQUIRED = (["candidate of %d bases" % L for L in MIN_LENGTHS] +
            ["windows 1023 and 1024 choose the same k-mer", "windows 1023 and 1024 choose different k-mer",
             "S == 1", "S == 2", "S == 3", "S == 4", "minimizer at 255 kept, at >= 256 sampled",
             "minimizer with pos + 15 == L - 256 sampled, == L - 255 kept", "interior minimizers dropped and kept",
             "N at position 0", "N at L - 1", "15 N across window 1024",
             "occ == 1999", "occ == 2000", "occ == 2001", "a call with >= 2000 chains"] +
            ["hits == %d" % h for h in (2048, 2049, 4096, 4097, 8192, 8193)] +
            ["one run of 4800 hits, diagonal steps of exactly TD", "one run of 4800 hits cut by a contig end",
             "left end of 2047 bases", "left end of 2048 bases", "left end of 2049 bases", "right end of 2047 bases",
             "right end of 2048 bases", "right end of 2049 bases", "end of 383 bases", "end of 384 bases",
             "clusters of exactly 2 anchors", "clusters of exactly 3 anchors", "span rule at equality", "span rule one base short"] +
            ["overhang %d, %s interval" % (v, m) for v in OVERHANGS for m in ("aligned", "whole-candidate")] +
            ["outermost anchor %d bases from the contig's end" % j for j in (7, 8, 9)] +
            ["first filter at equality", "first filter one base short", "indel of 8 bases in an end", "indel of 9 bases in an end",
             "genome N 5, 8 and 9 bases beyond the outermost anchor", "candidate N inside a worn end", "1 chain", "32 chains", "33 chains",
             "second filter at equality", "second filter one base short", "299 copies", "300 copies", "301 copies",
             "cut inside a group of equal anchors", "copies in two contigs"])


def coverage():
    ev = set()
    for n in names():
        ev.update(get(n)["events"])
    return ev


# ------------------------------------------------------------------------------------------------------------------------------
# checks shared by the CPU test (the twin's tables) and the GPU test (the device's, already compared with the twin's)
# ------------------------------------------------------------------------------------------------------------------------------
def check_closed_forms(name, table):
    """the rows per candidate and the clip words the construction gives; `table`: per candidate list of (contig, start1, end1, minus,
    anchors, clip word)"""
    c = get(name)
    for k, n in c.get("rows", {}).items():
        assert len(table[k]) == n, (name, k, len(table[k]), n)
    if "clips" in c:
        for k in range(len(c["cands"])):
            assert {r[0]: r[5] for r in table[k]} == c["clips"], (name, k, table[k])
    for k, na in c.get("row_anchors", {}).items():
        assert sorted(r[4] for r in table[k]) == na, (name, k, sorted(r[4] for r in table[k]), na)
    if "anchors" in c:
        assert {r[4] for r in table[0]} == set(c["anchors"]), (name, sorted({r[4] for r in table[0]}))


def check_stats(name, stats, what="batch"):
    """stats = copy_stats_ext() of the whole case: [0] and [1] == the model's, the closed forms of [2], [3], [4] + [5]"""
    c, m = get(name), model_of(name)
    assert stats[0] == sum(m["kept"]) and stats[1] == sum(m["hits"]), (name, what, stats, sum(m["kept"]), sum(m["hits"]))
    exp = c.get("stats", {})
    got = {"clusters": stats[2], "copies": stats[3], "chains": stats[4] + stats[5]}
    for k, v in exp.items():
        assert got[k] == v, (name, what, k, got[k], v)


def check_alone(name, k, stats):
    """copy_stats_ext() of candidate k searched alone"""
    c, m = get(name), model_of(name)
    assert stats[0] == m["kept"][k] and stats[1] == m["hits"][k], (name, k, stats, m["kept"][k], m["hits"][k])
    exp = c.get("alone_stats", {}).get(k, {})
    got = {"long": stats[4], "short": stats[5], "chains": stats[4] + stats[5], "clusters": stats[2]}
    for key, v in exp.items():
        assert got[key] == v, (name, k, key, got[key], v)
