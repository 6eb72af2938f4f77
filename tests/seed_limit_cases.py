"""Genomes for tests/test_seed_limit_cases.py and tests/test_gpu_seed_limits.py: stage 3.1, the all-vs-all seeding of
hite_amd/csrc/hite_copies.hip (hite_seed_allvsall[_dev]), at the limits of its own kernels -- the run search of seed_count2_kernel
(index tiles of 2048 entries with a halo of 1024), the cooperative anchor fill (64 seeds per wavefront), the contig cache of
seed_opens, the start bits per tile of 2048 anchors, the piece loop and its select tiles of 4096 clusters, the 16-bit segment ids
and the shard edges.  Pure python + numpy, seeded; no GPU and no twin in this file.

THE MODEL (model()) is the definition in the header above orc_seed_allvsall (oracle/hite_oracle_copies.c) written down with python
integers, lists and sorted(): minimizers (K = 15, W = 10, lowbias32, strand in the low bit) -> index in (hs, position) order -> runs
of equal hs >> 1 -> anchors in generation order -> stable order by (strand, d >> 6) -> clusters -> HSPs -> pieces -> stable order by
(qseg, sseg).  It returns every intermediate; the builders steer on them and the tests compare `stats` with them.

CLOSED FORMS: the designed cases carry the records they must give, worked out from minimizer positions alone (expect_*): they come
from neither the kernels nor the twin, whose loops are restatements of each other.

BEADS: a 15-mer between N's is the only valid k-mer of every window that sees it, hence a minimizer at exactly its position: strings
of beads put shared minimizers at chosen distances (gap 300 / 301, span 59 / 60, 2 / 3 anchors, runs of exactly n entries).

Every builder asserts, with the model alone, the property its case is named for."""
import bisect
import hashlib
import math
import os
import pickle

import numpy as np

K, W = 15, 10
MAXOCC, GAP, MINANCH, MINSPAN, MINPIECE = 1000, 300, 3, 60, 20
IDX_TILE, IDX_HALO = 2048, 1024       # seed_count2_kernel: SC_TILE, SC_HALO
ANC_TILE, ANC_ROW = 2048, 8           # seed_clusters_kernel: SF_TILE, SF_ITEMS
SEL_TILE = 4096                       # seed_piece_select_kernel: 256 x SPS_ITEMS
WAVE = 64
MAXSEG = 65535
KEYS = ("qseg", "sseg", "qs", "qe", "ss", "se")
BASES = "ACGT"
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}

_memo = {}


def cached(key, build):
    if key not in _memo:
        _memo[key] = build()
    return _memo[key]


SLIM = ("records", "stats", "seg_chrom", "seg_off")


def dump_memo(path):
    """what a child process of tests/test_gpu_seed_limits.py needs of the cases and models built so far (the genomes, the records,
    stats and segment tables): it loads them (SEED_LIMIT_MEMO) and does not build and model them a second time"""
    out = {k: ({f: v[f] for f in SLIM} if k[0] in ("model", "degenerate", "guard") else v) for k, v in _memo.items()}
    out["case set"] = case_set_key()
    with open(path, "wb") as f:
        pickle.dump(out, f)


def case_set_key():
    """names the case set and this file: a memo written by another version of either is not taken"""
    with open(__file__, "rb") as f:
        return (tuple(sorted(CASES)), hashlib.sha256(f.read()).hexdigest())


def load_memo():
    """(at the end of the import, when the cases are registered) the memo SEED_LIMIT_MEMO names, if it is this case set's"""
    path = os.environ.get("SEED_LIMIT_MEMO")
    if path and os.path.exists(path):
        with open(path, "rb") as f:
            memo = pickle.load(f)
        assert memo.pop("case set", None) == case_set_key(), "SEED_LIMIT_MEMO names a memo of another case set"
        _memo.update(memo)


def rand_seq(rng, n):
    return "".join(BASES[i] for i in rng.integers(0, 4, size=n))


def revcomp(s):
    return "".join(_COMP.get(c, "N") for c in reversed(s))


# ------------------------------------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------------------------------------
def lowbias32(x):
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xffffffff
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xffffffff
    x ^= x >> 16
    return x


def kmer_hs(kmer):
    """hs of one 15-mer (None with a base outside ACGT): (lowbias32(min(x, rc)) & ~1) | (rc < x), values >= 0xfffffffe lowered by 2"""
    x = rc = 0
    for i, ch in enumerate(kmer):
        c = BASES.find(ch)
        if c < 0:
            return None
        x |= c << (2 * i)
        rc |= (3 - c) << (2 * (K - 1 - i))
    hs = (lowbias32(min(x, rc)) & 0xfffffffe) | (1 if rc < x else 0)
    return hs - 2 if hs >= 0xfffffffe else hs


_BAD = 1 << 40


def minimizers(seq):
    """(W, K) minimizers of one sequence -> list of (position, hs, first window that chose it), in position order: per window of W
    k-mer starts the valid k-mer with the smallest (hs >> 1, position); a sequence with fewer than W k-mers is one window"""
    nk = len(seq) - K + 1
    if nk <= 0:
        return []
    mask = (1 << (2 * K)) - 1
    keys, hss = [], []
    x = rc = 0
    bad = -1
    for i, ch in enumerate(seq):
        c = BASES.find(ch)
        if c < 0:
            bad, c = i, 0
        x = (x >> 2) | (c << (2 * (K - 1)))
        rc = ((rc << 2) & mask) | (3 - c)
        p = i - K + 1
        if p < 0:
            continue
        if bad >= p:
            keys.append((_BAD, p))
            hss.append(None)
            continue
        hs = (lowbias32(min(x, rc)) & 0xfffffffe) | (1 if rc < x else 0)
        if hs >= 0xfffffffe:
            hs -= 2
        keys.append((hs >> 1, p))
        hss.append(hs)
    out, last = [], -1
    for p in range(nk - W + 1 if nk >= W else 1):
        h, best = min(keys[p:p + W])
        if h != _BAD and best != last:
            out.append((best, hss[best], p))
            last = best
    return out


def shard_edge(G, k, world):
    """lower edge of rank k of `world` in lin = strand * 2 G + diagonal (the formula of seed_shard_edge, the same in the twin and in
    hite_copies.hip): equal steps of the triangular distribution of the diagonals, rounded down to a multiple of 64"""
    if k <= 0:
        return 0
    if k >= world:
        return 4 * G + 64
    mass = 2.0 * k / world
    strand = 1 if mass >= 1.0 else 0
    t = mass - strand
    d = G * math.sqrt(2.0 * t) if t <= 0.5 else 2.0 * G - G * math.sqrt(2.0 * (1.0 - t))
    return (2 * G if strand else 0) + (int(max(d, 0.0)) & ~63)


def segments(contigs, seg_len):
    """the 'chr$offset' segment table: per contig ceil(len / seg_len) segments (an empty contig has one)"""
    sc, so = [], []
    for c, s in enumerate(contigs):
        for o in range(0, max(len(s), 1), seg_len):
            sc.append(c)
            so.append(o)
    return sc, so


def model(contigs, seg_len, shard=None):
    """-> dict: M, index [(hs, pos)], runs [(lo, hi)], seeds [(index entry, place in run, run size or 0, partners)] in position order,
    na, anchors [(rel, d, pi, pj)] in sorted order, starts [first anchor of every cluster], hsps [(cluster, rel, q0, q1, s0, s1)],
    records [(qseg, sseg, qs, qe, ss, se)], stats (M, na, clusters, records), coff, seg_chrom, seg_off.  shard = (rank, world)"""
    coff = [0]
    for s in contigs:
        coff.append(coff[-1] + len(s))
    G = coff[-1]
    seg_chrom, seg_off = segments(contigs, seg_len)
    seg_base = [0]
    for s in contigs:
        seg_base.append(seg_base[-1] + max(1, -(-len(s) // seg_len)))
    mins = [(coff[c] + p, hs) for c, s in enumerate(contigs) for p, hs, _w in minimizers(s)]
    M = len(mins)
    index = sorted((hs, pos) for pos, hs in mins)
    runs, run_of = [], {}
    for i, (hs, _pos) in enumerate(index):
        if i == 0 or hs >> 1 != index[i - 1][0] >> 1:
            runs.append([i, i + 1])
            run_of[hs >> 1] = len(runs) - 1
        else:
            runs[-1][1] = i + 1
    entry_of = {pos: i for i, (_hs, pos) in enumerate(index)}
    lo_lin = hi_lin = None
    if shard is not None and shard[1] > 1:
        lo_lin, hi_lin = shard_edge(G, shard[0], shard[1]), shard_edge(G, shard[0] + 1, shard[1])
    anchors, seeds = [], []
    for pos, hs in mins:
        lo, hi = runs[run_of[hs >> 1]]
        n0 = len(anchors)
        if hi - lo <= MAXOCC:
            for ohs, opos in index[lo:hi]:
                if opos == pos:
                    continue
                rel = (hs ^ ohs) & 1
                d = pos + opos if rel else opos - pos + G
                if lo_lin is not None and not lo_lin <= (2 * G if rel else 0) + d < hi_lin:
                    continue
                anchors.append((rel, d, pos, opos))
        i = entry_of[pos]
        seeds.append((i, i - lo, hi - lo if hi - lo <= MAXOCC else 0, len(anchors) - n0))
    anchors = sorted(anchors, key=lambda a: (a[0], a[1] >> 6))
    na = len(anchors)
    contig = lambda g: bisect.bisect_right(coff, g, 1, len(contigs)) - 1     # noqa: E731
    starts = [i for i in range(na) if i == 0 or opens(anchors[i - 1], anchors[i], contig)]
    hsps, pieces = [], []
    for k, b in enumerate(starts):
        e = starts[k + 1] if k + 1 < len(starts) else na
        rel, _d, q0, pf = anchors[b]
        q1, pl = anchors[e - 1][2] + K, anchors[e - 1][3]
        if e - b < MINANCH or q1 - q0 < MINSPAN:
            continue
        s0, s1 = min(pf, pl), max(pf, pl) + K
        hsps.append((k, rel, q0, q1, s0, s1))
        cq, cs = contig(q0), contig(pf)
        pieces += hsp_pieces(rel, (q0, q1), (s0, s1), coff[cq], coff[cs], seg_base[cq], seg_base[cs], seg_len)
    records = sorted(pieces, key=lambda r: (r[0], r[1]))
    return {"M": M, "G": G, "index": index, "runs": [tuple(r) for r in runs], "seeds": seeds, "na": na, "anchors": anchors,
            "starts": starts, "hsps": hsps, "records": records, "stats": (M, na, len(starts), len(records)), "coff": coff,
            "seg_chrom": seg_chrom, "seg_off": seg_off, "mins": mins}


def opens(a, b, contig):
    """does anchor b, behind a in the sorted order, open a cluster: strand, d >> 6, the contig of pi or of pj changes, or pi advances
    by more than GAP"""
    return (a[0], a[1] >> 6) != (b[0], b[1] >> 6) or b[2] - a[2] > GAP or contig(a[2]) != contig(b[2]) or contig(a[3]) != contig(b[3])


def meet(u, v):
    """intersection of two half-open intervals (possibly empty: hi <= lo)"""
    return max(u[0], v[0]), min(u[1], v[1])


def hsp_pieces(rel, q, s, q_origin, s_origin, q_base, s_base, seg_len):
    """The pieces of one HSP (query interval q, subject interval s, global, half open), stated per PAIR of segments and not as the
    two nested cutting loops of the kernel and the twin.  'The other side following linearly (reversed for rel 1)' is ONE map between
    the two axes, anchored where the HSP begins: query position t lies opposite subject position s[0] + (t - q[0]) (rel 0) or
    s[1] - (t - q[0]) (rel 1; the subject INTERVAL opposite [t, t') is then [s[1] - (t' - q[0]), s[1] - (t - q[0]))), 'clamped': only
    inside s.  The piece of (query segment i, subject segment j) is, on the subject side, what of segment j lies opposite the part of
    the HSP's query interval in segment i; on the query side, what of that part lies opposite the subject piece.  It is kept when both
    sides have 20 bases.  (The query side is never the longer one -- it is the image of the subject side, cut once more -- so under
    this definition the 20-base rule bites on the query side first: the subject-side test alone never drops a piece.)"""
    if rel:
        to_s = lambda u: (s[1] - (u[1] - q[0]), s[1] - (u[0] - q[0]))      # noqa: E731
        to_q = lambda v: (q[0] + s[1] - v[1], q[0] + s[1] - v[0])          # noqa: E731
    else:
        to_s = lambda u: (s[0] + u[0] - q[0], s[0] + u[1] - q[0])          # noqa: E731
        to_q = lambda v: (q[0] + v[0] - s[0], q[0] + v[1] - s[0])          # noqa: E731
    out = []
    for i in range((q[0] - q_origin) // seg_len, (q[1] - 1 - q_origin) // seg_len + 1):
        qseg = (q_origin + i * seg_len, q_origin + (i + 1) * seg_len)
        part = meet(q, qseg)
        for j in range((s[0] - s_origin) // seg_len, (s[1] - 1 - s_origin) // seg_len + 1):
            sseg = (s_origin + j * seg_len, s_origin + (j + 1) * seg_len)
            sp = meet(meet(to_s(part), s), sseg)
            if sp[1] <= sp[0]:
                continue
            qp = meet(to_q(sp), part)
            if qp[1] - qp[0] >= MINPIECE and sp[1] - sp[0] >= MINPIECE:
                lo1, hi1 = sp[0] - sseg[0] + 1, sp[1] - sseg[0]
                out.append((q_base + i, s_base + j, qp[0] - qseg[0] + 1, qp[1] - qseg[0], hi1 if rel else lo1, lo1 if rel else hi1))
    return out


def table(m):
    """the model's records as the six arrays of Context.seed_allvsall"""
    r = m["records"]
    return {k: np.asarray([x[i] for x in r], dtype=np.int32 if i < 2 else np.int64) for i, k in enumerate(KEYS)}


# ------------------------------------------------------------------------------------------------------------------------------
# events: what a case makes the kernels meet, counted on the model
# ------------------------------------------------------------------------------------------------------------------------------
def events(m, contigs, sharded=False):
    ev = {}

    def hit(name):
        ev[name] = ev.get(name, 0) + 1

    M, na = m["M"], m["na"]
    coff = m["coff"]
    contig = lambda g: bisect.bisect_right(coff, g, 1, len(contigs)) - 1     # noqa: E731
    if not sharded:
        # 1. seed_count2_kernel
        if 0 < M <= IDX_HALO:
            hit("M<=1024")
        if M > 0 and M % IDX_TILE == 0:
            hit("M%2048==0")
        for lo, hi in m["runs"]:
            n = hi - lo
            if n < 2:
                continue
            ok = n <= MAXOCC
            border = (hi - 1) // IDX_TILE * IDX_TILE          # the last tile border at or below the run's last entry
            if ok and lo < border < hi:
                hit("run straddles an index tile border")
                if border - lo > 64:
                    hit("run begins more than a word into the lower halo")
                if hi - (border - 1) > 64:
                    hit("run ends more than a word into the upper halo")
            if not ok and lo < border < hi:
                hit("uncountable run straddles an index tile border")
            if ok and lo > 0 and lo % IDX_TILE == 0:
                hit("run begins on an index tile border")
            if ok and (hi - 1) % IDX_TILE == 0 and lo < hi - 1:
                hit("run's last entry on an index tile border")
            if ok and lo == 0:
                hit("run touches entry 0")
            if ok and hi == M:
                hit("run touches entry M")
            if n == MAXOCC:
                hit("occ==1000 (place 999, partners 999)")
            if n == MAXOCC + 1:
                hit("occ==1001")
        # 3. seed_anchor_coop_kernel
        cnt = [s[3] for s in m["seeds"]]
        for t0 in range(0, M, WAVE):
            w = cnt[t0:t0 + WAVE]
            tot = sum(w)
            if len(w) < WAVE and tot > 0:
                hit("last wavefront with fewer than 64 seeds")
            if len(w) == WAVE and tot == 0:
                hit("64 seeds without a partner")
            if len(w) == WAVE and tot > 0 and w[0] == 0 and w[-1] == 0:
                hit("empty seeds at both ends of a wavefront")
            if len(w) == WAVE and tot == MAXOCC - 1 and max(w) == MAXOCC - 1:
                hit("one seed of 999 partners among 63 empty ones")
    # 4. seed_opens and 5. the cluster kernels
    an = m["anchors"]
    st = set(m["starts"])
    for i in range(1, na):
        a, b = an[i - 1], an[i]
        same = (a[0], a[1] >> 6) == (b[0], b[1] >> 6)
        if same and b[2] - a[2] <= GAP:
            q, s = contig(a[2]) != contig(b[2]), contig(a[3]) != contig(b[3])
            if q or s:
                hit("contig cut at row place %d" % (i % ANC_ROW))
                if q:
                    hit("query contig cut, strand %d" % a[0])
                if s:
                    hit("subject contig cut, strand %d" % a[0])
            if b[2] - a[2] == GAP:
                hit("gap of exactly 300 inside a cluster")
        if same and b[2] - a[2] == GAP + 1:
            hit("gap of 301 cuts")
        if a[0] == b[0] and a[1] % 64 == 63 and b[1] == a[1] + 1 and b[2] - a[2] <= GAP:
            hit("diagonals 63 | 64 cut")
        if same and a[1] % 64 == 62 and b[1] == a[1] + 1 and i not in st:
            hit("diagonals 62 | 63 stay")
        if i % ANC_TILE == 0:
            hit("cluster continues across an anchor tile border" if i not in st else "cluster starts at anchor 2048 k")
        if i % ANC_TILE == ANC_TILE - 1 and i in st:
            hit("cluster starts at anchor 2048 k - 1")
    if na > 0 and na % ANC_TILE == 0:
        hit("na%2048==0")
    if na % ANC_TILE == 1:
        hit("na%2048==1" if na > 1 else "na==1")
    if 1 < na < ANC_ROW:
        hit("na<8")
    # 6. the piece kernels
    starts = m["starts"] + [na]
    qualified = {h[0] for h in m["hsps"]}
    for k in range(len(starts) - 1):
        b, e = starts[k], starts[k + 1]
        span = an[e - 1][2] + K - an[b][2]
        if e - b == MINANCH - 1 and span >= MINSPAN:
            hit("2 anchors with the span")
        if e - b == MINANCH and span >= MINSPAN:
            hit("3 anchors")
        if e - b >= MINANCH and span == MINSPAN - 1:
            hit("span 59")
        if e - b >= MINANCH and span == MINSPAN:
            hit("span 60")
        if k >= SEL_TILE and k in qualified:
            hit("HSP in the second select tile")
    return ev


# ------------------------------------------------------------------------------------------------------------------------------
# building blocks
# ------------------------------------------------------------------------------------------------------------------------------
def beads(rng, n):
    return [rand_seq(rng, K) for _ in range(n)]


def bead_string(xs, at):
    """N's with bead xs[i] at offset at[i] (at least K + 1 apart); an N before the first and behind the last bead"""
    assert len(xs) == len(at) and all(b - a > K for a, b in zip(at, at[1:]))
    s = ["N"] * (at[-1] + K + 2)
    for x, a in zip(xs, at):
        s[1 + a:1 + a + K] = x
    return "".join(s)


def run_array(x, n):
    """n entries of one hash: (x N) n times behind an N"""
    return "N" + (x + "N") * n


def filler_for(fixed, run_hs, rng, residue=None, total=None, least=0):
    """a contig of unique sequence, cut so that (residue) the run of hash run_hs begins at an index entry = residue mod 2048, or
    (total) the genome has exactly `total` minimizers; at least `least` of the filler's minimizers are kept"""
    base = [hs for s in fixed for _p, hs, _w in minimizers(s)]
    seq = rand_seq(rng, 40_000 + 6 * least)
    fm = minimizers(seq)
    below = sum(1 for hs in base if hs >> 1 < run_hs >> 1) if run_hs is not None else 0
    for j, (_p, hs, _w) in enumerate(fm):
        # the first j minimizers are those of the prefix that ends with the window before the one that chose minimizer j
        if j >= least and ((residue is not None and below % IDX_TILE == residue) or (total is not None and len(base) + j == total)):
            return seq[:fm[j][2] + W + K - 2]
        if run_hs is not None and hs >> 1 < run_hs >> 1:
            below += 1
    raise AssertionError("the filler does not reach the wanted place")


def far_pairs(xs):
    """single beads before and (in reverse order: no two on one diagonal, at most two in one bucket) behind everything else: each
    pair gives ONE anchor in front of all closer pairs in the sorted order and one behind them, and no record"""
    return "".join("N" + x + "N" for x in xs), "".join("N" + x + "N" for x in reversed(xs))


def find_run(m, x):
    """(lo, hi) of the run of 15-mer x in the model's index"""
    h = kmer_hs(x) >> 1
    for lo, hi in m["runs"]:
        if m["index"][lo][0] >> 1 == h:
            return lo, hi
    raise AssertionError("bead without a run")


def extreme_bead(rng, tries, smallest):
    xs = beads(rng, tries)
    return (min if smallest else max)(xs, key=lambda x: kmer_hs(x) >> 1)


# ------------------------------------------------------------------------------------------------------------------------------
# closed forms
# ------------------------------------------------------------------------------------------------------------------------------
def expect_two_copies(m, a, b, n, inverted, seg_len):
    """Two copies of one family of n bases at global a < b of ONE contig that starts at 0 (the second one reverse-complemented when
    `inverted`), far more than GAP apart, seg_len beyond the contig: per direction one HSP from the first to the last shared
    minimizer, [first, last + 15) on the one (sum) diagonal.  Uses the minimizer positions only."""
    pos = {p: hs >> 1 for p, hs in m["mins"]}
    other = (lambda p: b + n - (p - a) - K) if inverted else (lambda p: p - a + b)
    # (a k-mer that hangs over an end of the family is shared when the unique bases beside the two copies happen to agree)
    shared = sorted(p for p in pos if a - K < p < a + n and pos.get(other(p)) == pos[p])
    assert len(shared) >= MINANCH and all(y - x <= GAP for x, y in zip(shared, shared[1:])) and b - a - n > GAP
    f, l = shared[0], shared[-1]
    assert l + K - f >= MINSPAN and b + n < seg_len
    if not inverted:
        # the direction with the query in the second copy has the smaller diagonal (pj - pi + G): its cluster comes first
        return [(0, 0, other(f) + 1, other(l) + K, f + 1, l + K), (0, 0, f + 1, l + K, other(f) + 1, other(l) + K)]
    # one sum diagonal for both directions, seeds in position order: the first copy's come first; ss > se
    return [(0, 0, f + 1, l + K, other(f) + K, other(l) + 1), (0, 0, other(l) + 1, other(f) + K, l + K, f + 1)]


def expect_bead_pieces(a, b, n, seg_len, inverted):
    """Two copies of one string of beads spanning n bases, at a and b of ONE contig that starts at 0 (the second reverse-complemented
    when `inverted`): the records of both directions, worked out in the coordinates of the STRING.  Offset o of the string is base
    a + o of the first copy and base b + o (b + n - 1 - o when inverted) of the second; the string is cut at every offset at which
    either copy meets a segment border; a stretch [lo, hi) of 20 offsets or more is a record in each direction, 1-based inside its
    segments, the subject side the other way round when inverted."""
    second = (lambda o: b + n - 1 - o) if inverted else (lambda o: b + o)
    cuts = {0, n}
    for o in range(1, n):
        if (a + o) % seg_len == 0:
            cuts.add(o)
        if (second(o) % seg_len == 0) if not inverted else (second(o - 1) % seg_len == 0):
            cuts.add(o)
    cuts = sorted(cuts)
    in_seg = lambda g: (g // seg_len, g % seg_len + 1)          # noqa: E731
    first, other = [], []
    for lo, hi in zip(cuts, cuts[1:]):
        if hi - lo < MINPIECE:
            continue
        (s1, x0), (_s, x1) = in_seg(a + lo), in_seg(a + hi - 1)                      # the first copy's side, ascending
        (s2, y0), (_s, y1) = in_seg(second(lo)), in_seg(second(hi - 1))              # the second copy's: descending when inverted
        first.append((s1, s2, x0, x1, y0, y1))
        other.append((s2, s1, y1, y0, x1, x0) if inverted else (s2, s1, y0, y1, x0, x1))
    return sorted(first + other, key=lambda r: (r[0], r[1]))


# ------------------------------------------------------------------------------------------------------------------------------
# the cases: name -> (group, builder); a builder returns dict(contigs, seg_len[, expect][, shards])
# ------------------------------------------------------------------------------------------------------------------------------
CASES = {}


def case(group):
    def reg(fn):
        CASES[fn.__name__] = (group, fn)
        return fn
    return reg


def get(name):
    def build():
        c = CASES[name][1]()
        c["name"], c["group"] = name, CASES[name][0]
        return c
    return cached(("case", name), build)


def model_of(name, shard=None):
    c = get(name)
    return cached(("model", name, shard), lambda: model(c["contigs"], c["seg_len"], shard))


def names(group=None):
    return [n for n, (g, _f) in CASES.items() if group is None or g == group]


def _family_pair(rng, n=400, gap=700):
    """two copies of a random family in unique sequence: something for every case to report"""
    fam = rand_seq(rng, n)
    return rand_seq(rng, 200) + fam + rand_seq(rng, gap) + fam + rand_seq(rng, 200)


# ---- 1. runs of the index against the tiles of seed_count2_kernel ---------------------------------------------------------------
def _run_case(seed, n, residue, least=IDX_TILE + IDX_HALO):
    rng = np.random.default_rng(seed)
    x = beads(rng, 1)[0]
    fixed = [_family_pair(rng), run_array(x, n)]
    contigs = fixed + [filler_for(fixed, kmer_hs(x), rng, residue=residue % IDX_TILE, least=least)]
    m = model(contigs, 1_000_000)
    lo, hi = find_run(m, x)
    assert hi - lo == n and lo % IDX_TILE == residue % IDX_TILE and m["M"] > IDX_TILE + IDX_HALO, (lo, hi, m["M"])
    return {"contigs": contigs, "seg_len": 1_000_000}


@case("runs")
def run_straddles_tile():
    return _run_case(101, 40, IDX_TILE - 17)


@case("runs")
def run_begins_on_tile():
    return _run_case(102, 40, 0)


@case("runs")
def run_last_entry_on_tile():
    return _run_case(103, 40, IDX_TILE - 40 + 1)


@case("runs")
def run_1000_deep_in_halo():
    """a run of exactly 1000 entries, 480 below a tile border and 520 above it, beginning at bit 32 of a word of the run map: its last
    entries find the run's start only in the LAST word the backward search may read (place > 960 + entry mod 64), its first ones the
    run's end only in the last word of the forward search (entries to the end + entry mod 64 >= 1024); 10-bit fields at 999; one of
    its seeds stands alone among unique ones: a wavefront with one seed of 999 partners and 63 empty ones"""
    rng = np.random.default_rng(104)
    x = beads(rng, 1)[0]
    fixed = [run_array(x, MAXOCC - 1), rand_seq(rng, 1200) + "N" + x + "N" + rand_seq(rng, 1200)]
    contigs = fixed + [filler_for(fixed, kmer_hs(x), rng, residue=IDX_TILE - 480, least=IDX_TILE)]
    m = model(contigs, 1_000_000)
    lo, hi = find_run(m, x)
    assert hi - lo == MAXOCC and lo % IDX_TILE == IDX_TILE - 480
    assert any(i - lo > IDX_HALO - 64 + (i & 63) for i in range(lo, hi)), "no entry needs the last word of the backward search"
    assert any(hi - i + (i & 63) >= IDX_HALO for i in range(lo, hi)), "no entry needs the last word of the forward search"
    assert max(s[1] for s in m["seeds"]) == MAXOCC - 1 and max(s[3] for s in m["seeds"]) == MAXOCC - 1
    return {"contigs": contigs, "seg_len": 1_000_000}


@case("runs")
def run_1001_across_tile():
    """1001 entries across a tile border: not seeded from, whichever tile looks"""
    rng = np.random.default_rng(105)
    x = beads(rng, 1)[0]
    fixed = [_family_pair(rng), run_array(x, MAXOCC + 1)]
    contigs = fixed + [filler_for(fixed, kmer_hs(x), rng, residue=IDX_TILE - 300, least=IDX_TILE)]
    m = model(contigs, 1_000_000)
    lo, hi = find_run(m, x)
    assert hi - lo == MAXOCC + 1 and lo % IDX_TILE == IDX_TILE - 300 and all(s[3] == 0 for s in m["seeds"] if lo <= s[0] < hi)
    return {"contigs": contigs, "seg_len": 1_000_000}


def _extreme_run(seed, smallest):
    for attempt in range(8):                     # (deterministic: the first seed whose filler stays on one side of the bead)
        rng = np.random.default_rng(seed + 1000 * attempt)
        x = extreme_bead(rng, 60_000, smallest)
        contigs = [_family_pair(rng), run_array(x, 30), rand_seq(rng, 18_000)]
        m = model(contigs, 1_000_000)
        lo, hi = find_run(m, x)
        if lo == 0 if smallest else hi == m["M"]:
            break
    assert hi - lo == 30 and (lo == 0 if smallest else hi == m["M"]) and m["M"] > IDX_TILE + IDX_HALO, (lo, hi, m["M"])
    return {"contigs": contigs, "seg_len": 1_000_000}


@case("runs")
def run_at_entry_0():
    return _extreme_run(106, True)


@case("runs")
def run_at_entry_M():
    return _extreme_run(107, False)


@case("runs")
def index_all_halo():
    """M <= 1024: one workgroup, every entry's run search ends at entry 0 or M inside the halo; the genome ends with a repeat: the
    last wavefront has fewer than 64 seeds and anchors to write"""
    rng = np.random.default_rng(108)
    x = beads(rng, 1)[0]
    fam = rand_seq(rng, 300)
    contigs = [rand_seq(rng, 300) + fam + rand_seq(rng, 900), run_array(x, 25), rand_seq(rng, 600) + fam]
    m = model(contigs, 1_000_000)
    assert 0 < m["M"] <= IDX_HALO and m["M"] % WAVE and sum(s[3] for s in m["seeds"][m["M"] // WAVE * WAVE:]) > 0
    return {"contigs": contigs, "seg_len": 1_000_000}


@case("runs")
def index_two_full_tiles():
    """M = 4096 exactly: no ragged tile, entry M is the first entry behind the last tile"""
    rng = np.random.default_rng(109)
    x = beads(rng, 1)[0]
    fixed = [_family_pair(rng), run_array(x, 30)]
    contigs = fixed + [filler_for(fixed, None, rng, total=2 * IDX_TILE)]
    m = model(contigs, 1_000_000)
    assert m["M"] == 2 * IDX_TILE
    return {"contigs": contigs, "seg_len": 1_000_000}


# ---- 4. contig borders, gaps and diagonal buckets in seed_opens -------------------------------------------------------------------
def _border_case(seed, inverted, extra):
    """a family whose second copy lies across a contig border (contigs are adjacent in global coordinates: the copy is contiguous on
    its diagonal, minimizers 300 apart at the most: only the contig test cuts it); `extra` pairs of beads far apart put that many
    anchors in front of the family's in the sorted order: the cut moves through the places of a thread's row"""
    rng = np.random.default_rng(seed)
    fam = rand_seq(rng, 500)
    second = revcomp(fam) if inverted else fam
    xs = beads(rng, extra)
    left, right = far_pairs(xs)
    c0 = left + rand_seq(rng, 150) + fam + rand_seq(rng, 400) + second[:260]
    c1 = second[260:] + rand_seq(rng, 150) + right
    m = model([c0, c1], 1_000_000)
    recs = m["records"]
    # each direction is cut in two at the border: four records, none across it
    assert len(recs) == 4 and len(m["hsps"]) == 4, (len(recs), len(m["hsps"]))
    border = len(c0)
    for _k, _rel, q0, q1, s0, s1 in m["hsps"]:
        assert not q0 < border < q1 and not s0 < border < s1
    return {"contigs": [c0, c1], "seg_len": 1_000_000}


def _border_builder(inverted, extra):
    def build():
        return _border_case(200 + extra + (50 if inverted else 0), inverted, extra)
    build.__name__ = "border_%s_%d" % ("inv" if inverted else "fwd", extra)
    return build


for _inv in (False, True):
    for _e in range(ANC_ROW):
        case("contigs")(_border_builder(_inv, _e))


def _bead_pair_genome(rng, at, at2=None, dist=1500, inverted=False, head=300):
    """one contig: unique head, a string of beads at offsets `at`, `dist` bases on the same beads at `at2` (default: the same offsets),
    unique tail.  -> (contig, global position of the first string's offset 0, of the second's)"""
    xs = beads(rng, len(at))
    s1 = bead_string(xs, at)
    s2 = bead_string(xs, at2 or at)
    if inverted:
        s2 = revcomp(s2)
    mid = rand_seq(rng, dist - len(s1))
    c = rand_seq(rng, head) + s1 + mid + s2 + rand_seq(rng, 300)
    return c, head + 1, head + dist + 1


@case("contigs")
def gap_300_and_301():
    """beads 300 apart are one cluster, 301 apart two: (contig 0) 0 30 60 | +300 | 360 390 420: ONE HSP of 6 anchors per direction;
    (contig 1) the same with 301: TWO HSPs per direction; (contig 2) 0 301 602: three single anchors, none"""
    rng = np.random.default_rng(230)
    c0, a0, b0 = _bead_pair_genome(rng, [0, 30, 60, 360, 390, 420])
    c1, a1, b1 = _bead_pair_genome(rng, [0, 30, 60, 361, 391, 421])
    c2, _a2, _b2 = _bead_pair_genome(rng, [0, 301, 602])
    o1 = len(c0)
    exp = []
    for q, s in ((b0, a0), (a0, b0)):
        exp.append((0, 0, q + 1, q + 420 + K, s + 1, s + 420 + K))
    for q, s in ((b1, a1), (a1, b1)):
        exp.append((1, 1, q + 1, q + 60 + K, s + 1, s + 60 + K))
        exp.append((1, 1, q + 361 + 1, q + 421 + K, s + 361 + 1, s + 421 + K))
    m = model([c0, c1, c2], 1_000_000)
    assert o1 == m["coff"][1]
    return {"contigs": [c0, c1, c2], "seg_len": 1_000_000, "expect": exp}


@case("contigs")
def bucket_63_and_64():
    """the second copy has one more N between its third and fourth bead: the diagonal steps by one in the middle.  Contig 0: from
    d = 63 to 64 (mod 64): another bucket, two clusters of 3 anchors; contig 1: from 62 to 63: one cluster of 6.  Only in the
    direction whose diagonal was steered (query in the first copy)"""
    rng = np.random.default_rng(231)
    at, at2 = [0, 30, 60, 90, 120, 150], [0, 30, 60, 91, 121, 151]
    contigs, exp, off = [], [], 0
    for ci, want in enumerate((63, 62)):
        c, a, b = _bead_pair_genome(rng, at, at2)
        G = 2 * len(c)                                # both contigs have the same length
        # d = pj - pi + G = b - a + G for the first three beads: pad the head of the contig until d = want (mod 64)
        pad = (want - (b - a + G)) % 64
        cut_at = b - 1                                # (unique bases in front of the second copy, as many taken off the tail)
        c = c[:cut_at] + rand_seq(rng, pad) + c[cut_at:len(c) - pad]
        b += pad
        contigs.append(c)
        q, s = off + a, off + b
        if want == 63:
            exp.append((ci, ci, q - off + 1, q - off + 60 + K, s - off + 1, s - off + 60 + K))
            exp.append((ci, ci, q - off + 90 + 1, q - off + 150 + K, s - off + 91 + 1, s - off + 151 + K))
        else:
            # (the subject side follows the query's 165 bases from the HSP's subject start; the HSP's own subject end is one further)
            exp.append((ci, ci, q - off + 1, q - off + 150 + K, s - off + 1, s - off + 150 + K))
        off += len(c)
    m = model(contigs, 1_000_000)
    assert len(contigs[0]) == len(contigs[1]) and m["G"] == 2 * len(contigs[0])
    got = [r for r in m["records"] if r[2] < r[4]]                 # query in the first copy
    assert sorted(got) == sorted(exp), (got, exp)
    return {"contigs": contigs, "seg_len": 1_000_000, "expect_subset": exp}


# ---- 5. cluster starts against the tiles of 2048 anchors --------------------------------------------------------------------------
def _tile_case(seed, fam_len, want_start=None, want_na=None):
    """two copies of a family: per direction ONE cluster on one diagonal; pairs of beads further apart than the copies put one anchor
    in front of them (and one behind): the second cluster's start and na are steered through them"""
    rng = np.random.default_rng(seed)
    fam = rand_seq(rng, fam_len)
    core = rand_seq(rng, 100) + fam + rand_seq(rng, 400) + fam + rand_seq(rng, 100)
    m0 = model([core], 1_000_000)
    assert len(m0["starts"]) == 2 or want_na is not None, len(m0["starts"])
    if want_start is not None:
        extra = want_start - m0["starts"][1]
    else:
        assert (want_na - m0["na"]) % 2 == 0
        extra = (want_na - m0["na"]) // 2
    assert 0 <= extra < 400, extra
    left, right = far_pairs(beads(rng, extra))
    contigs = [left + core + right]
    return {"contigs": contigs, "seg_len": 1_000_000}


@case("clusters")
def cluster_longer_than_a_tile():
    rng = np.random.default_rng(301)
    fam = rand_seq(rng, 12_000)
    contigs = [rand_seq(rng, 100) + fam + rand_seq(rng, 400) + fam + rand_seq(rng, 100)]
    m = model(contigs, 1_000_000)
    assert len(m["starts"]) == 2 and m["starts"][1] > ANC_TILE and m["na"] - m["starts"][1] > ANC_TILE, m["starts"]
    return {"contigs": contigs, "seg_len": 1_000_000}


@case("clusters")
def cluster_starts_at_2048():
    c = _tile_case(302, 10_000, want_start=ANC_TILE)
    m = model(c["contigs"], c["seg_len"])
    assert ANC_TILE in m["starts"]
    return c


@case("clusters")
def cluster_starts_at_2047():
    c = _tile_case(303, 10_000, want_start=ANC_TILE - 1)
    m = model(c["contigs"], c["seg_len"])
    assert ANC_TILE - 1 in m["starts"] and ANC_TILE not in m["starts"]
    return c


@case("clusters")
def anchors_fill_two_tiles():
    c = _tile_case(304, 10_000, want_na=2 * ANC_TILE)
    assert model(c["contigs"], c["seg_len"])["na"] == 2 * ANC_TILE
    return c


@case("clusters")
def anchors_six():
    """three beads twice: na = 6 < 8, one thread's row not full; two clusters of 3 anchors with a span of 60: two records"""
    rng = np.random.default_rng(305)
    c, a, b = _bead_pair_genome(rng, [0, 22, 45])
    m = model([c], 1_000_000)
    assert m["na"] == 6
    exp = [(0, 0, b + 1, b + 45 + K, a + 1, a + 45 + K), (0, 0, a + 1, a + 45 + K, b + 1, b + 45 + K)]
    return {"contigs": [c], "seg_len": 1_000_000, "expect": exp}


@case("clusters")
def anchors_one_per_share():
    """one bead twice, 0.6 G apart: na = 2, and in three shares the first holds ONE anchor (G - 0.6 G lies below its edge, G + 0.6 G
    above)"""
    rng = np.random.default_rng(306)
    x = beads(rng, 1)[0]
    c = rand_seq(rng, 200) + "N" + x + "N" + rand_seq(rng, 1800) + "N" + x + "N" + rand_seq(rng, 1000)
    m = model([c], 1_000_000)
    assert m["na"] == 2 and model([c], 1_000_000, (0, 3))["na"] == 1
    return {"contigs": [c], "seg_len": 1_000_000, "expect": [], "worlds": (3,)}


@case("clusters")
def anchors_2049_in_share():
    """rank 0 of 3 holds 2049 anchors: the last tile holds ONE anchor, whose thread closes the list.  (Unsharded anchors come in
    pairs: an odd count exists in a share only.)  The copies are 0.28 G apart: one direction lies below the first edge (1.18 G)."""
    rng = np.random.default_rng(307)
    fam = rand_seq(rng, 10_000)
    core = rand_seq(rng, 100) + fam + rand_seq(rng, 400) + fam + rand_seq(rng, 9000)
    extra = ANC_TILE + 1 - model([core], 1_000_000, (0, 3))["na"]
    assert 0 <= extra < 400, extra
    left, right = far_pairs(beads(rng, extra))
    contigs = [left + core + right]
    assert model(contigs, 1_000_000, (0, 3))["na"] == ANC_TILE + 1
    return {"contigs": contigs, "seg_len": 1_000_000, "worlds": (3,)}


# ---- 6. the piece kernels ---------------------------------------------------------------------------------------------------------
@case("pieces")
def anchors_2_and_3_span_59_and_60():
    """contig 0: beads 0 60 (2 anchors, span 75): none; contig 1: 0 22 44 (3 anchors, span 59): none; contig 2: 0 22 45 (span 60): one
    HSP per direction; contig 3: 0 30 60 90 (4 anchors): one per direction"""
    rng = np.random.default_rng(401)
    contigs, exp = [], []
    for ci, at in enumerate(([0, 60], [0, 22, 44], [0, 22, 45], [0, 30, 60, 90])):
        c, a, b = _bead_pair_genome(rng, at)
        contigs.append(c)
        if ci >= 2:
            exp += [(ci, ci, b + 1, b + at[-1] + K, a + 1, a + at[-1] + K), (ci, ci, a + 1, a + at[-1] + K, b + 1, b + at[-1] + K)]
    return {"contigs": contigs, "seg_len": 1_000_000, "expect": exp}


def _piece_case(seed, inverted, q_left, head_tail):
    """an HSP of 200 bases (beads 0 .. 185) in two copies, seg_len 1000, the first copy placed so that a segment border leaves `q_left`
    bases of it on one side (head_tail: 0 = its first bases, 1 = its last): 19 are dropped on the query side of the one direction and on
    the subject side of the other, 20 are kept"""
    rng = np.random.default_rng(seed)
    at = [0, 37, 74, 111, 148, 185]
    head = 1000 - 1 - q_left if head_tail == 0 else 1000 - 1 - (200 - q_left)
    c, a, b = _bead_pair_genome(rng, at, dist=1400, inverted=inverted, head=head)
    m = model([c], 1000)
    assert len(m["hsps"]) == 2 and all(h[3] - h[2] == 200 and h[5] - h[4] == 200 for h in m["hsps"]), m["hsps"]
    assert m["hsps"][0][2] in (a, b) and (1000 - a) == (q_left if head_tail == 0 else 200 - q_left), (a, b, m["hsps"])
    lens = sorted((r[3] - r[2] + 1, abs(r[5] - r[4]) + 1) for r in m["records"])
    short, rest = q_left, 200 - q_left
    # the second copy lies inside one segment (1400 further on): each direction gives the long piece, and the short one iff >= 20
    assert 1000 < b % 1000 + 1000 and (b % 1000) + 200 < 1000, b
    exp_lens = [(rest, rest)] * 2 + ([(short, short)] * 2 if short >= MINPIECE else [])
    assert lens == sorted(exp_lens), (lens, exp_lens)
    exp = expect_bead_pieces(a, b, 200, 1000, inverted)
    assert len(exp) == len(exp_lens)
    return {"contigs": [c], "seg_len": 1000, "expect": exp}


def _piece_builder(inverted, q_left, head_tail):
    def build():
        return _piece_case(410 + q_left + 3 * head_tail + (7 if inverted else 0), inverted, q_left, head_tail)
    build.__name__ = "piece_%s_%d_%s" % ("inv" if inverted else "fwd", q_left, "head" if head_tail == 0 else "tail")
    return build


for _inv in (False, True):
    for _q in (19, 20):
        for _ht in (0, 1):
            case("pieces")(_piece_builder(_inv, _q, _ht))


@case("pieces")
def piece_query_and_subject_border():
    """the first copy has a border 50 bases in, the second one 100 bases in: the direction first -> second gives [0, 50) [50, 100)
    [100, 200), the other one the same three pieces from its side"""
    rng = np.random.default_rng(430)
    at = [0, 37, 74, 111, 148, 185]
    c, a, b = _bead_pair_genome(rng, at, dist=1950, head=949)
    assert a == 950 and b == 2900
    exp = []
    for q, s in ((b, a), (a, b)):               # pieces [0, 50) [50, 100) [100, 200) of both copies, in either direction
        for lo, hi in ((0, 50), (50, 100), (100, 200)):
            exp.append(((q + lo) // 1000, (s + lo) // 1000, (q + lo) % 1000 + 1, (q + hi - 1) % 1000 + 1, (s + lo) % 1000 + 1,
                        (s + hi - 1) % 1000 + 1))
    assert sorted(exp) == sorted(expect_bead_pieces(a, b, 200, 1000, False))
    return {"contigs": [c], "seg_len": 1000, "expect": exp}


@case("pieces")
def piece_query_and_subject_border_inverted():
    """the same with the second copy reverse-complemented: its border, 100 bases in, lies opposite offset 100 of the first again, but
    the pieces pair up the other way round: the first copy's [0, 50) with the second copy's LAST 50 bases, in the segment behind the border"""
    rng = np.random.default_rng(433)
    c, a, b = _bead_pair_genome(rng, [0, 37, 74, 111, 148, 185], dist=1950, inverted=True, head=949)
    assert a == 950 and b == 2900
    exp = expect_bead_pieces(a, b, 200, 1000, True)
    # written out: first copy [950, 1000) is opposite [3050, 3100): segment 0 against segment 3, 951 .. 1000 against 100 .. 51
    assert (0, 3, 951, 1000, 100, 51) in exp and (1, 3, 1, 50, 50, 1) in exp and (1, 2, 51, 150, 1000, 901) in exp and len(exp) == 6
    assert (3, 0, 51, 100, 1000, 951) in exp and (3, 1, 1, 50, 50, 1) in exp and (2, 1, 901, 1000, 150, 51) in exp
    return {"contigs": [c], "seg_len": 1000, "expect": exp}


@case("pieces")
def piece_three_segments():
    """seg_len 80: an HSP of 200 bases spans three or four segments on either side, the borders of the two sides interleave"""
    rng = np.random.default_rng(431)
    c, a, b = _bead_pair_genome(rng, [0, 37, 74, 111, 148, 185], dist=1010, head=339)
    m = model([c], 80)
    # borders 60 and 140 bases into the first copy, 10, 90 and 170 into the second: pieces of 10 (dropped), 50, 30, 50, 30, 30
    assert a % 80 == 20 and b % 80 == 70 and len(m["records"]) == 10
    assert sorted(r[3] - r[2] + 1 for r in m["records"]) == [30] * 6 + [50] * 4
    assert len(m["hsps"]) == 2 and all((h[3] - 1) // 80 - h[2] // 80 >= 2 and (h[5] - 1) // 80 - h[4] // 80 >= 2 for h in m["hsps"])
    return {"contigs": [c], "seg_len": 80, "expect": expect_bead_pieces(a, b, 200, 80, False)}


@case("pieces")
def piece_three_segments_inverted():
    rng = np.random.default_rng(434)
    c, a, b = _bead_pair_genome(rng, [0, 37, 74, 111, 148, 185], dist=1010, inverted=True, head=339)
    exp = expect_bead_pieces(a, b, 200, 80, True)
    # the second copy's borders 10, 90, 170 bases in lie opposite offsets 190, 110, 30 of the string: 30 30 50 30 50 (10 dropped)
    assert sorted(r[3] - r[2] + 1 for r in exp) == [30] * 6 + [50] * 4
    return {"contigs": [c], "seg_len": 80, "expect": exp}


@case("pieces")
def second_select_tile():
    """2100 beads 32 apart and again in reverse order: every anchor alone in its bucket, 4200 forward clusters; behind them (strand
    1 sorts last) an inverted family: an HSP among the clusters of the second select tile; a forward family for the first tile"""
    rng = np.random.default_rng(432)
    n = 2100
    xs = beads(rng, n)
    fam, fam2 = rand_seq(rng, 400), rand_seq(rng, 400)
    c0 = bead_string(xs, [32 * i for i in range(n)]) + rand_seq(rng, 100) + fam + rand_seq(rng, 500) + revcomp(fam)
    c1 = bead_string(xs[::-1], [32 * i for i in range(n)]) + rand_seq(rng, 100) + fam2 + rand_seq(rng, 500) + fam2
    m = model([c0, c1], 1_000_000)
    ks = [h[0] for h in m["hsps"]]
    assert len(m["starts"]) > SEL_TILE + 1 and min(ks) < SEL_TILE <= max(ks), (len(m["starts"]), ks)
    return {"contigs": [c0, c1], "seg_len": 1_000_000}


# ---- closed forms on real sequence -------------------------------------------------------------------------------------------------
def _two_copies(seed, inverted):
    rng = np.random.default_rng(seed)
    n, a, b = 900, 700, 3100
    fam = rand_seq(rng, n)
    c = rand_seq(rng, a) + fam + rand_seq(rng, b - a - n) + (revcomp(fam) if inverted else fam) + rand_seq(rng, 600)
    m = model([c], 1_000_000)
    return {"contigs": [c], "seg_len": 1_000_000, "expect": expect_two_copies(m, a, b, n, inverted, 1_000_000)}


@case("pieces")
def two_copies_forward():
    return _two_copies(440, False)


@case("pieces")
def two_copies_inverted():
    return _two_copies(441, True)


# ---- 8. shard edges -----------------------------------------------------------------------------------------------------------------
def _shard_case(world, k):
    """G fixed first; two bead families, each twice: the diagonal G + distance of the one lies in the LAST bucket below edge k of
    `world`, that of the other in the FIRST bucket at it (the edge is a multiple of 64)"""
    rng = np.random.default_rng(500 + 10 * world + k)
    G = 40_000
    e = shard_edge(G, k, world)
    assert G + 1000 < e < 2 * G - 3000, (world, k, e)
    at = [0, 30, 60, 90]
    xs1, xs2 = beads(rng, 4), beads(rng, 4)
    s1, s2 = bead_string(xs1, at), bead_string(xs2, at)
    seq = list(rand_seq(rng, G))
    # family 1: first copy at 500, second at 500 + (e - 64 + 5 - G): d = e - 59, the bucket below the edge
    # family 2: first copy at 1000, second at 1000 + (e + 7 - G): d = e + 7, the bucket at the edge
    for s, p, d in ((s1, 500, e - 59), (s2, 1000, e + 7)):
        for q in (p, p + d - G):
            seq[q:q + len(s)] = s
    c = "".join(seq)
    m = model([c], 1_000_000)
    assert m["G"] == G
    d_hi = sorted({a[1] >> 6 for a in m["anchors"] if a[0] == 0 and a[1] > G})
    assert (e >> 6) - 1 in d_hi and e >> 6 in d_hi, (e >> 6, d_hi)
    lo, hi = model([c], 1_000_000, (k - 1, world)), model([c], 1_000_000, (k, world))
    assert any(a[1] >> 6 == (e >> 6) - 1 for a in lo["anchors"]) and not any(a[1] >> 6 == e >> 6 for a in lo["anchors"])
    assert any(a[1] >> 6 == e >> 6 for a in hi["anchors"]) and not any(a[1] >> 6 == (e >> 6) - 1 for a in hi["anchors"])
    assert len(lo["records"]) >= 1 and len(hi["records"]) >= 1
    return {"contigs": [c], "seg_len": 1_000_000, "worlds": (world,)}


def _shard_builder(world, k):
    def build():
        return _shard_case(world, k)
    build.__name__ = "shard_edge_%d_of_%d" % (k, world)
    return build


# world 2 has one inner edge, the strand border 2 G, which no forward diagonal comes near (d < 2 G - 15 - distance to the end) and
# whose first bucket holds only sums of two positions below 64: it is met by every case with both strands, not by a designed one
for _w, _k in ((3, 1), (7, 2), (7, 3)):
    case("shards")(_shard_builder(_w, _k))


# ---- 7. the segment-count guard; degenerate inputs ---------------------------------------------------------------------------------
def guard_genome(extra):
    """65 534 + extra contigs of one base and one contig with a repeat: 65 535 + extra segments"""
    rng = np.random.default_rng(600)
    return ["A"] * (MAXSEG - 1 + extra) + [_family_pair(rng)]


DEGENERATE = {
    "all_N": (["N" * 500, "NNNN"], (0, 0, 0, 0)),
    "one_minimizer": (["ACGTTGCATGCCAGT", "NNN"], (1, 0, 0, 0)),
    "unique": (None, None),            # na = 0: filled in below
    "no_record": (None, None),         # na > 0, np = 0
}


def degenerate(name):
    contigs, stats = DEGENERATE[name]
    if name == "unique":
        contigs = [rand_seq(np.random.default_rng(601), 3000)]
    if name == "no_record":
        rng = np.random.default_rng(602)
        x = beads(rng, 1)[0]
        contigs = [rand_seq(rng, 500) + "N" + x + "N" + rand_seq(rng, 500) + "N" + x + "N" + rand_seq(rng, 200)]
    m = cached(("degenerate", name), lambda: model(contigs, 1_000_000))
    if stats is not None:
        assert m["stats"] == stats, (name, m["stats"])
    if name == "unique":
        assert m["stats"][0] > 0 and m["stats"][1:] == (0, 0, 0)
    if name == "no_record":
        assert m["stats"][1:] == (2, 2, 0)
    return contigs, m


def guard_model():
    return cached(("guard",), lambda: model(guard_genome(0), 1_000_000))


# events every case set must contain (items 1, 3, 4, 5, 6 of the suite's header), with the model's count; sharded ones come from
# the shares of the cases that name `worlds`
REQUIRED = [
    "M<=1024", "M%2048==0", "run straddles an index tile border", "run begins more than a word into the lower halo",
    "run ends more than a word into the upper halo", "uncountable run straddles an index tile border", "run begins on an index tile border",
    "run's last entry on an index tile border", "run touches entry 0", "run touches entry M", "occ==1000 (place 999, partners 999)",
    "occ==1001",
    "last wavefront with fewer than 64 seeds", "64 seeds without a partner", "empty seeds at both ends of a wavefront",
    "one seed of 999 partners among 63 empty ones",
] + ["contig cut at row place %d" % q for q in range(ANC_ROW)] + [
    "query contig cut, strand 0", "query contig cut, strand 1", "subject contig cut, strand 0", "subject contig cut, strand 1",
    "gap of exactly 300 inside a cluster", "gap of 301 cuts", "diagonals 63 | 64 cut", "diagonals 62 | 63 stay",
    "cluster continues across an anchor tile border", "cluster starts at anchor 2048 k", "cluster starts at anchor 2048 k - 1",
    "na%2048==0", "na%2048==1", "na==1", "na<8",
    "2 anchors with the span", "3 anchors", "span 59", "span 60", "HSP in the second select tile",
]


def coverage():
    """event -> count over all cases (unsharded) and over the shares of the cases that name their worlds"""
    tot = {}
    for n in names():
        c = get(n)
        runs = [(model_of(n), False)]
        for w in c.get("worlds", ()):
            runs += [(model_of(n, (r, w)), True) for r in range(w)]
        for m, sh in runs:
            for k, v in events(m, c["contigs"], sh).items():
                tot[k] = tot.get(k, 0) + v
    return tot


# ------------------------------------------------------------------------------------------------------------------------------
# the checks, run with the device (test_gpu_seed_limits.py) or the twin (test_seed_limit_cases.py) behind `ctx`
# ------------------------------------------------------------------------------------------------------------------------------
def same_table(got, exp, what):
    for k in KEYS:
        assert np.array_equal(np.asarray(got[k], dtype=np.int64), np.asarray(exp[k], dtype=np.int64)), \
            (what, k, len(got[k]), len(exp[k]))


def check_case(ctx, name, stats=True):
    """ctx.seed_allvsall on the case == the model's records (and stats), the segment table == the model's"""
    c, m = get(name), model_of(name)
    ctx.genome_pack(c["contigs"])
    ctx.release_copy_index()
    got = ctx.seed_allvsall(seg_len=c["seg_len"])
    same_table(got, table(m), name)
    if stats:
        assert tuple(got["stats"]) == m["stats"], (name, got["stats"], m["stats"])
    sc, so = ctx.seed_segments(c["seg_len"])
    assert list(sc) == m["seg_chrom"] and list(so) == m["seg_off"], name
    return got


def check_closed_form(name):
    c, m = get(name), model_of(name)
    if "expect" in c:
        assert m["records"] == sorted(c["expect"], key=lambda r: (r[0], r[1])), (name, m["records"], c["expect"])
    return "expect" in c or "expect_subset" in c


def check_shares(ctx, name, world, twin=None, stats=True):
    """every rank's table == the model's share (== the twin's, when given); the shares in rank order, stably sorted by (qseg, sseg),
    are the unsharded table"""
    c, whole = get(name), model_of(name)
    ctx.genome_pack(c["contigs"])
    ctx.release_copy_index()
    if twin is not None:
        twin.genome_pack(c["contigs"])
    rows = []
    try:
        for r in range(world):
            ctx.seed_shard(r, world)
            got = ctx.seed_allvsall(seg_len=c["seg_len"])
            m = model_of(name, (r, world))
            same_table(got, table(m), (name, r, world))
            if stats:
                assert tuple(got["stats"]) == m["stats"], (name, r, world, got["stats"], m["stats"])
            if twin is not None:
                twin.seed_shard(r, world)
                same_table(got, twin.seed_allvsall(seg_len=c["seg_len"]), (name, r, world, "twin"))
            rows += list(zip(*[[int(v) for v in got[k]] for k in KEYS]))
    finally:
        ctx.seed_shard(0, 0)
        if twin is not None:
            twin.seed_shard(0, 0)
    assert sorted(rows, key=lambda x: (x[0], x[1])) == whole["records"], (name, world)


load_memo()
