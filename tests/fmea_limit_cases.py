"""HSP tables for tests/test_gpu_fmea_limits.py and tests/test_fmea_limit_cases.py: FMEA (hite_fmea_chain, hite_amd/csrc/hite_fmea.hip)
at the limits of its own kernels -- the block sort of the segment ranks, the 64-wide rounds of the cluster sweep, the 256-wide stride
of the containment filter, the length and key-packing bounds, and the shortcut of the first-appearance kernel on grouped tables.
Pure numpy / python, seeded.  Written once and run twice: every check_* takes a callable with the signature of Context.fmea_chain
and compares it with the CPU twin (oracle_lib.fmea) on the same arrays.

The arrays are built directly (segment ids are NOT numbered by first appearance, as oracle_lib.hsp_arrays would number them: an id
that equals its rank hides a wrong rank).  Every builder asserts the property its case is named for with a plain python sweep of
its own -- next to the twin, a second and independent statement of the rule -- and records the figure in case["claim"].

Coordinates are the table's: 1-based inclusive, a reverse hit has ss > se.  An interval is (chrom id, start, end), 0-based half open,
as the names 'chrom:start-end' of the reference carry it."""
import numpy as np

import oracle_lib as O

SEG_LEN = 1_000_000
SEGS_PER_CHROM = 200
FM_MAXSEG = 4096            # hite_fmea.hip: most segments of one table
SWEEP_LANES = 64            # fm_cluster_kernel: members of the open cluster tested per round
FILTER_STRIDE = 256         # fm_filter_kernel: candidates tested per trip
CLUSTER_GRID_SLOTS = 4096 * 4   # fm_cluster_kernel: slots of one pass of its grid (4096 blocks of 4 wavefronts)
COLS = ("qseg", "sseg", "qs", "qe", "ss", "se")


# ------------------------------------------------------------------------------------------------------------------------------
# cases, the twin, comparison
# ------------------------------------------------------------------------------------------------------------------------------
def layout(nseg):
    """segment id -> (chromosome id, offset): SEGS_PER_CHROM segments of 1 Mbp per chromosome; no two ids share a name"""
    ids = np.arange(nseg)
    return (ids // SEGS_PER_CHROM).astype(np.int32), ((ids % SEGS_PER_CHROM) * SEG_LEN).astype(np.int64)


def make_case(rows, nseg=None, skip_gap=2000, max_len=30000, seg_chrom=None, seg_off=None, **claim):
    r = np.asarray(rows, dtype=np.int64).reshape(-1, 6)
    if seg_chrom is None:
        seg_chrom, seg_off = layout(nseg)
    c = {"qseg": np.ascontiguousarray(r[:, 0], dtype=np.int32), "sseg": np.ascontiguousarray(r[:, 1], dtype=np.int32),
         "seg_chrom": np.ascontiguousarray(seg_chrom, dtype=np.int32), "seg_off": np.ascontiguousarray(seg_off, dtype=np.int64),
         "skip_gap": int(skip_gap), "max_len": int(max_len), "claim": claim}
    for k, name in enumerate(COLS[2:]):
        c[name] = np.ascontiguousarray(r[:, 2 + k])
    return c


def rows_of(c):
    return np.stack([c[k].astype(np.int64) for k in COLS], axis=1)


def with_rows(c, rows, **claim):
    return make_case(rows, skip_gap=c["skip_gap"], max_len=c["max_len"], seg_chrom=c["seg_chrom"], seg_off=c["seg_off"],
                     **dict(c["claim"], **claim))


def run(fmea_chain, c):
    """the intervals fmea_chain emits for the case, in its order"""
    oc, os_, oe = fmea_chain(c["qseg"], c["sseg"], c["qs"], c["qe"], c["ss"], c["se"], c["seg_chrom"], c["seg_off"], c["skip_gap"],
                             c["max_len"])
    return list(zip((int(x) for x in oc), (int(x) for x in os_), (int(x) for x in oe)))


class _ChromNames:
    def __getitem__(self, i):
        return "c%d" % i


def twin_names(c):
    h = {k: c[k] for k in COLS + ("seg_chrom", "seg_off")}
    h["chrom_names"] = _ChromNames()
    return O.fmea(h, c["skip_gap"], c["max_len"])


def parse_names(names):
    out = []
    for nm in names:
        ch, pos = nm.split(":")
        a, b = pos.split("-")
        out.append((int(ch[1:]), int(a), int(b)))
    return out


def twin(c):
    """the twin's intervals; computed once per case object"""
    if "_twin" not in c:
        c["_twin"] = parse_names(twin_names(c))
    return c["_twin"]


_memo = {}


def cached(key, build):
    if key not in _memo:
        _memo[key] = build()
    return _memo[key]


def compare(fmea_chain, c, label):
    got, exp = run(fmea_chain, c), twin(c)
    if got != exp:
        k = next((i for i, (a, b) in enumerate(zip(got, exp)) if a != b), min(len(got), len(exp)))
        raise AssertionError("%s: %d intervals against the twin's %d; first difference at %d: %s / %s"
                             % (label, len(got), len(exp), k, got[k:k + 2], exp[k:k + 2]))
    return got


def absolute(c, seg, st, en):
    """the interval of the 0-based half-open stretch [st, en) of a segment"""
    return int(c["seg_chrom"][seg]), int(c["seg_off"][seg]) + st, int(c["seg_off"][seg]) + en


# ------------------------------------------------------------------------------------------------------------------------------
# group A: segment ranks
# ------------------------------------------------------------------------------------------------------------------------------
RANK_NSEG = (1, 2, 3, 255, 256, 257, 1000, 4095, 4096)


def ranks_case(nseg, swap_rank=None):
    """Queries first appear in a fixed pseudo-random permutation of the ids; each has three or four subjects (fewer where nseg has
    no more) that first appear in a permuted order too, some ids are subjects only and some are never used.  Each subject carries
    ONE HSP; the query intervals of the siblings start at different bases of one 10-bp block and end in one 10-bp block, so all
    share the de-duplication keys and only the chain of the subject that ranks first is new: the interval a query emits names its
    first subject, and the order of the intervals is the order of the query ranks.  The rows come subject round by subject round
    (all first subjects in query order, then all second ones ...): no row follows a row of its own query.
    swap_rank: the first two subject rounds of that query change places (its subjects' first-appearance order is swapped)."""
    rng = np.random.default_rng(4000 + nseg)
    ids = rng.permutation(nseg)
    n_unused = 0 if nseg < 8 else max(1, nseg // 512)
    n_sonly = 0 if nseg < 3 else max(1, nseg // 256)
    nq = nseg - n_unused - n_sonly
    queries, sonly = ids[:nq], ids[nq:nq + n_sonly]
    pool = ids[:nq + n_sonly]
    per_round = [[] for _ in range(4)]
    first = []                                                  # per query rank: (subject, 0-based start, end) of its first subject
    g = 0
    for r, q in enumerate(queries):
        k = min(3 + int(rng.integers(0, 2)), len(pool))
        subj = [int(s) for s in rng.choice(pool, size=k, replace=False)]
        if r < n_sonly and int(sonly[r]) not in subj:
            subj[int(rng.integers(0, k))] = int(sonly[r])       # every subject-only id is used
        base = 100_000 + 10 * int(rng.integers(0, 39_000))
        length = 150 + 10 * int(rng.integers(0, 10))
        d = rng.choice(10, size=k, replace=False)
        for j, s in enumerate(subj):
            st, en = base + int(d[j]), base + length + int(rng.integers(0, 10))
            s0 = 600_000 + 20 * g
            g += 1
            ss, se = s0 + 1, s0 + 120
            if rng.integers(0, 2):
                ss, se = se, ss
            per_round[j].append((int(q), s, st + 1, en, ss, se))
            if j == 0:
                first.append([s, st, en])
    if swap_rank is not None:
        i0 = swap_rank
        i1 = [k for k, row in enumerate(per_round[1]) if row[0] == per_round[0][i0][0]][0]
        per_round[0][i0], per_round[1][i1] = per_round[1][i1], per_round[0][i0]
        row = per_round[0][i0]
        first[i0] = [row[1], row[2] - 1, row[3]]
    rows = [row for rnd in per_round for row in rnd]
    npairs = len(rows)
    np2 = 1
    while np2 < nseg:
        np2 <<= 1
    c = make_case(rows, nseg, segments=nseg, np2=np2, queries=nq, subject_only=n_sonly, unused=n_unused, n_rows=npairs,
                  slots=2 * npairs, top_rank=nq - 1)
    c["predicted"] = [absolute(c, int(q), f[1], f[2]) for q, f in zip(queries, first)]
    c["query_order"] = [int(q) for q in queries]
    return c


def ranks(nseg):
    return cached(("ranks", nseg), lambda: ranks_case(nseg))


def bitonic_order(keys, skip_from=None):
    """the order block_bitonic leaves the ids in: the compare-exchange network over np2 slots on (key, id), padded with 0xffffffff;
    skip_from drops the stages whose partner distance j is at least that (a sort that is only right inside blocks of that size)"""
    n = len(keys)
    np2 = 1
    while np2 < n:
        np2 <<= 1
    key = np.full(np2, 0xFFFFFFFF, dtype=np.int64)
    key[:n] = keys
    idx = np.arange(np2, dtype=np.int64)
    i = np.arange(np2)
    k = 2
    while k <= np2:
        j = k >> 1
        while j > 0:
            if skip_from is None or j < skip_from:
                lo = i[(i ^ j) > i]
                hi = lo ^ j
                up = (lo & k) == 0
                gt = (key[lo] > key[hi]) | ((key[lo] == key[hi]) & (idx[lo] > idx[hi]))
                sw = gt == up
                a, b = lo[sw], hi[sw]
                key[a], key[b] = key[b].copy(), key[a].copy()
                idx[a], idx[b] = idx[b].copy(), idx[a].copy()
            j >>= 1
        k <<= 1
    return idx[:n]


def first_rows(c):
    """first_q[id], first_pair[(q, s)]: the row in which a query / a pair first appears among the kept rows (no exact self hit)"""
    first_q, first_pair = {}, {}
    r = rows_of(c)
    for i, (q, s, qs, qe, ss, se) in enumerate(r.tolist()):
        if q == s and qs == ss and qe == se:
            continue
        first_q.setdefault(q, i)
        first_pair.setdefault((q, s), i)
    return first_q, first_pair


def check_ranks_case(nseg):
    """self-check of one rank case; -> its claim"""
    c = ranks(nseg)
    cl = c["claim"]
    assert twin(c) == c["predicted"], nseg                         # the plain prediction: one interval per query, in rank order
    assert len(set(c["predicted"])) == cl["queries"]
    used_q, used_s = set(c["qseg"].tolist()), set(c["sseg"].tolist())
    assert len(used_q) == cl["queries"] and len(used_s - used_q) == cl["subject_only"]
    assert nseg - len(used_q | used_s) == cl["unused"]
    if nseg >= 255:
        assert cl["unused"] >= 1 and cl["subject_only"] >= 1
        assert c["query_order"] != sorted(c["query_order"])        # id != rank
        # swapping two subjects' first-appearance order changes the answer
        r = cl["queries"] // 2
        sw = ranks_case(nseg, swap_rank=r)
        assert twin(sw) == sw["predicted"] and twin(sw) != twin(c)
        assert [a == b for a, b in zip(twin(sw), twin(c))].count(False) == 1
    if nseg > 256:
        # the block sort needs its stages with a partner 256 or more slots away: without them these keys come out misordered
        fq, _ = first_rows(c)
        keys = np.full(nseg, 0x7FFFFFFF, dtype=np.int64)
        for q, i in fq.items():
            keys[q] = i
        full = bitonic_order(keys)
        assert full[:cl["queries"]].tolist() == c["query_order"]
        assert bitonic_order(keys, skip_from=256).tolist() != full.tolist()
    if nseg == FM_MAXSEG:
        assert 12_000 <= cl["n_rows"] <= 16_000 and cl["slots"] > CLUSTER_GRID_SLOTS, cl
        assert cl["top_rank"] >= 4000                              # 12 bits of query rank in the candidate sort key
    return cl


def check_ranks(fmea_chain, nseg):
    compare(fmea_chain, ranks(nseg), "ranks nseg=%d" % nseg)


def small_case():
    """a table anybody answers: the 3-segment rank case"""
    return ranks(3)


def check_too_many_segments(fmea_chain):
    """FM_MAXSEG + 1 segments are an error, not an answer; the same context then answers a small case"""
    c = ranks(FM_MAXSEG)
    sc, so = layout(FM_MAXSEG + 1)
    over = make_case(rows_of(c), skip_gap=c["skip_gap"], max_len=c["max_len"], seg_chrom=sc, seg_off=so)
    try:
        run(fmea_chain, over)
    except RuntimeError:
        pass
    else:
        raise AssertionError("%d segments did not raise" % (FM_MAXSEG + 1))
    compare(fmea_chain, small_case(), "small case after the refused one")


# ------------------------------------------------------------------------------------------------------------------------------
# group B: rounds of the cluster sweep
# ------------------------------------------------------------------------------------------------------------------------------
SWEEP_FILLERS = (63, 64, 65, 127, 128, 129, 300)
SWEEP_GAP = 10_000


def sweep_members(c):
    """plain sweep of ONE (query, subject, strand) slot: the HSPs in the slot's order (forward: by (ss, se); reverse: by
    (-ss, -se)) and, per HSP, how many places back its qualifying members of the open cluster sit (none: it opens a cluster)"""
    r = rows_of(c).tolist()
    rev = r[0][4] > r[0][5]
    assert len({(x[0], x[1], x[4] > x[5]) for x in r}) == 1
    order = sorted(range(len(r)), key=lambda i: (-r[i][4], -r[i][5]) if rev else (r[i][4], r[i][5]))
    start, back = 0, []
    for k, i in enumerate(order):
        hits = []
        for m in range(k - 1, start - 1, -1):
            o = r[order[m]]
            d = o[5] - r[i][4] if rev else r[i][4] - o[5]
            if d < c["skip_gap"] and r[i][3] > o[3]:
                hits.append(k - m)
        if not hits and k:
            start = k
        back.append(hits)
    return order, back


def sweep_case(fillers, rev, join):
    """anchor, `fillers` HSPs that lie between anchor and probe in the slot's order but whose q_end is not below the probe's (they
    join the anchor's cluster and cannot take the probe in; one of them has the probe's q_end exactly and is within the gap), then
    the probe, whose s_start is skip_gap - 1 (join) or skip_gap (not join) beyond the anchor's s_end.  Anchor and probe chain into
    one interval when they share a cluster.  The fillers' q runs against their s, so that no two of them chain."""
    gap = SWEEP_GAP
    rows = [(0, 1, 1000, 1300, 10_000, 10_300),                    # anchor
            (0, 1, 1650, 1800, 10_150, 10_300)]                    # q_end == the probe's, s_end == the anchor's
    for f in range(fillers - 1):
        qs = 50_000 + 200 * (fillers - f)
        rows.append((0, 1, qs, qs + 150, 10_400 + 30 * f, 10_550 + 30 * f))
    p_ss = 10_300 + (gap - 1 if join else gap)
    rows.append((0, 1, 1400, 1800, p_ss, p_ss + 400))
    if rev:
        rows = [(q, s, a, b, SEG_LEN + 1 - x, SEG_LEN + 1 - y) for (q, s, a, b, x, y) in rows]
    perm = np.random.default_rng(fillers).permutation(len(rows))
    c = make_case([rows[i] for i in perm], 2, skip_gap=gap, fillers=fillers, rev=rev, join=join)
    order, back = sweep_members(c)
    assert int(perm[order[-1]]) == len(rows) - 1 and int(perm[order[0]]) == 0      # the probe comes last, the anchor first
    assert back[-1] == ([fillers + 1] if join else []), (fillers, back[-1])         # the ONLY member that takes the probe in
    assert all(b for b in back[1:-1])                                               # every filler stays in the anchor's cluster
    c["claim"]["members_back"] = fillers + 1 if join else None
    c["claim"]["round"] = fillers // SWEEP_LANES + 1 if join else None             # the round of 64 lanes that decides
    merged, anchor, probe = absolute(c, 0, 999, 1800), absolute(c, 0, 999, 1300), absolute(c, 0, 1399, 1800)
    c["present"], c["absent"] = ([merged], [anchor, probe]) if join else ([anchor, probe], [merged])
    return c


def sweep_cases():
    return cached("sweep", lambda: [("sweep F=%d %s %s" % (f, "rev" if rev else "fwd", "join" if join else "open"), sweep_case(f, rev, join))
                                    for f in SWEEP_FILLERS for rev in (False, True) for join in (True, False)])


def _check_visible(label, c, got):
    assert all(iv in got for iv in c["present"]) and not any(iv in got for iv in c["absent"]), (label, c["present"])


def check_sweep_cases():
    claims = []
    for label, c in sweep_cases():
        _check_visible(label, c, twin(c))
        assert len(twin(c)) == c["claim"]["fillers"] - 1 + len(c["present"])        # every plain filler is an interval of its own
        claims.append((label, c["claim"]))
    assert {cl["round"] for _, cl in claims if cl["join"]} == {1, 2, 3, 5}
    return claims


def check_sweep(fmea_chain):
    for label, c in sweep_cases():
        _check_visible(label, c, compare(fmea_chain, c, label))


# ------------------------------------------------------------------------------------------------------------------------------
# group C: containment filter
# ------------------------------------------------------------------------------------------------------------------------------
FILTER_CANDS = 700
FILTER_LAYOUTS = ((100, 250, 250), (300, 100, 50), (550, 20, 20), (20, 20, 20))     # background candidates: long, middle, short
DROP_PAIRS = ((100, 95), (200, 190), (2000, 1900))     # (length of the inner candidate, bases of it inside the outer one)
KEEP_PAIRS = ((100, 94), (2000, 1899))


def greedy_filter(cands):
    """process_seq_group in plain numpy: cands = [(start, end)] in chain order -> (sorted order, keep flags in that order)"""
    iv = np.asarray(cands, dtype=np.int64)
    order = np.argsort(-(iv[:, 1] - iv[:, 0]), kind="stable")
    s, e = iv[order, 0], iv[order, 1]
    keep = np.ones(len(iv), dtype=bool)
    for i in range(len(iv)):
        if not keep[i]:
            continue
        ov = np.maximum(np.minimum(e[i], e[i + 1:]) - np.maximum(s[i], s[i + 1:]), 0)
        keep[i + 1:] &= ~(ov / (e[i + 1:] - s[i + 1:]).astype(np.float64) >= 0.95)
    return order, keep


class _Axis:
    """hands out disjoint stretches of a query, 50 bases apart"""

    def __init__(self, rng):
        self.pos, self.rng = 1000, rng

    def take(self, span):
        x = self.pos + int(self.rng.integers(0, 10))
        self.pos = x + span + 50
        return x


def _filter_specials(ax, rng):
    """-> [(tag, start, end)] in chain order, [(tag of the tested candidate, dropped?)]"""
    items, verdict = [], []
    for fam, dropped in ((DROP_PAIRS, True), (KEEP_PAIRS, False)):
        for ln, ov in fam:
            lo = 4000 + int(rng.integers(0, 2000))
            x = ax.take(lo + ln)
            o = x + ln
            items += [("outer", o, o + lo), ("inner %d/%d" % (ov, ln), o - (ln - ov), o + ov)]
            verdict.append(("inner %d/%d" % (ov, ln), dropped))
    # equal lengths: the earlier chain stays, whichever starts first on the query
    x = ax.take(2200)
    items += [("equal B", x + 100, x + 2100), ("equal A 1900/2000", x, x + 2000)]
    verdict += [("equal B", False), ("equal A 1900/2000", True)]
    x = ax.take(2200)
    items += [("equal D", x + 101, x + 2101), ("equal C 1899/2000", x, x + 2000)]
    verdict += [("equal D", False), ("equal C 1899/2000", False)]
    # i holds 95 % of j, j all of k, i almost none of k: j goes, and k -- examined when j is gone -- stays
    x = ax.take(3200)
    items += [("chain k", x + 2990, x + 3100), ("chain j", x + 1100, x + 3100), ("chain i", x, x + 3000)]
    verdict += [("chain i", False), ("chain j", True), ("chain k", False)]
    return items, verdict


def _filter_query(rng, n_long, n_mid, n_short, total):
    ax = _Axis(rng)
    items, verdict = _filter_specials(ax, rng)
    nsp = len(items)
    fill = total - len(items) - n_long - n_mid - n_short
    assert fill >= 0
    lens = ([2050 + k % 150 for k in range(n_long)] + [1999 - (k * 1798) // max(n_mid, 1) for k in range(n_mid)] +
            [101 + k % 99 for k in range(n_short)] + [80 + k % 20 for k in range(fill)])
    for ln in lens:
        x = ax.take(ln)
        items.append(("", x, x + ln))
    # chain order: shuffled, the specials keep their order among themselves
    slots = np.sort(rng.choice(len(items), size=nsp, replace=False))
    rest = [k for k in rng.permutation(np.arange(nsp, len(items)))]
    out, sp, bg = [None] * len(items), 0, 0
    for pos in range(len(items)):
        if sp < nsp and pos == slots[sp]:
            out[pos] = items[sp]
            sp += 1
        else:
            out[pos] = items[rest[bg]]
            bg += 1
    return out, verdict


def filter_case(layouts=FILTER_LAYOUTS, total=FILTER_CANDS, seed=31):
    """one query per layout, each with `total` candidates after de-duplication: every candidate is one HSP whose subject stretch
    (50 bases, 100 apart, all on one subject segment, skip_gap 20) is a cluster and a chain of its own, so the chain order is the
    order of the subject stretches.  Pairs on the 95 % threshold, equal lengths, and a chain of containments sit between disjoint
    background candidates whose numbers per length class move the pairs through the sorted list."""
    rng = np.random.default_rng(seed)
    nq = len(layouts)
    rows, per_query = [], []
    g = 0
    for q, (nl, nm, ns) in enumerate(layouts):
        items, verdict = _filter_query(rng, nl, nm, ns, total)
        for _tag, st, en in items:
            rows.append((q, nq, st + 1, en, 1000 + 100 * g + 1, 1000 + 100 * g + 50))
            g += 1
        per_query.append((items, verdict))
    perm = rng.permutation(len(rows))
    c = make_case([rows[i] for i in perm], skip_gap=20, seg_chrom=np.arange(nq + 1), seg_off=np.zeros(nq + 1))
    predicted, figures = [], []
    qorder = sorted(range(nq), key=lambda q: int(np.flatnonzero(c["qseg"] == q)[0]))        # the queries' first appearance
    for q in qorder:
        items, verdict = per_query[q]
        order, keep = greedy_filter([(st, en) for _t, st, en in items])
        where = {items[i][0]: (pos, bool(keep[pos])) for pos, i in enumerate(order.tolist()) if items[i][0] not in ("", "outer")}
        for tag, dropped in verdict:
            assert where[tag][1] == (not dropped), (q, tag)
        predicted += [absolute(c, q, items[i][1], items[i][2]) for pos, i in enumerate(order.tolist()) if keep[pos]]
        figures.append({"candidates": len(items), "kept": int(keep.sum()), "position": {t: p for t, (p, _k) in where.items()}})
    c["predicted"], c["claim"]["queries"] = predicted, figures
    return c


def filter_full():
    return cached("filter", filter_case)


def filter_pairs():
    """the threshold pairs, the equal lengths and the containment chain alone (the fixture's form of the group)"""
    return cached("filter_pairs", lambda: filter_case(layouts=((0, 0, 0),), total=17, seed=32))


def check_filter_case():
    c = filter_full()
    assert twin(c) == c["predicted"]
    pos = {}
    for fig in c["claim"]["queries"]:
        assert fig["candidates"] == FILTER_CANDS and FILTER_STRIDE < fig["kept"] < FILTER_CANDS, fig
        for tag, p in fig["position"].items():
            pos.setdefault(tag, set()).add(0 if p < FILTER_STRIDE else 1 if p < 2 * FILTER_STRIDE else 2)
    for ln, ov in DROP_PAIRS + KEEP_PAIRS:
        assert pos["inner %d/%d" % (ov, ln)] == {0, 1, 2}, (ln, ov, pos)            # below 256, between 256 and 512, above 512
    assert pos["equal A 1900/2000"] == {0, 1, 2} and pos["chain k"] >= {0, 2}
    p = filter_pairs()
    assert twin(p) == p["predicted"] and p["claim"]["queries"][0]["kept"] == 17 - 5
    return c["claim"]


def check_filter(fmea_chain):
    compare(fmea_chain, filter_full(), "containment filter, %d candidates per query" % FILTER_CANDS)
    compare(fmea_chain, filter_pairs(), "containment filter, threshold pairs")


# ------------------------------------------------------------------------------------------------------------------------------
# group D: length and key limits
# ------------------------------------------------------------------------------------------------------------------------------
MAX_LEN = 30000


def fl10(x):
    return (x // 10) * 10


def pack_key_ok(chrom, a, b):
    """pack_key of hite_fmea.hip: chromosome in 18 bits, a / 10 in 28 bits, (b - a) / 10 + 2^17 in 18 bits (C division)"""
    q = abs(b - a) // 10 * (1 if b >= a else -1)
    d = q + (1 << 17)
    return 0 <= chrom < (1 << 18) and a >= 0 and a // 10 < (1 << 28) and 0 <= d < (1 << 18)


def keys_ok(chrom, st, en):
    """all four rounded keys of the stretch [st, en) (en < st: a reverse subject stretch) can be packed"""
    s1, e1 = fl10(st), fl10(en)
    return all(pack_key_ok(chrom, a, b) for a in (s1, s1 + 10) for b in (e1, e1 + 10))


# the first value on the bad side of each bound, from the expression above (check_key_bounds recomputes them)
SPAN_FIRST_BAD = 1_310_710          # rounded end - rounded start of a forward stretch; 1 310 700 is packed
SPAN_REV_FIRST_BAD = -1_310_720     # the same for a reverse subject stretch; -1 310 710 is packed
START_FIRST_BAD = 2_684_354_550     # rounded start (segment offset + start); 2 684 354 540 is packed
CHROM_FIRST_BAD = 1 << 18


def check_key_bounds():
    span = next(d for d in range(0, 2_000_000, 10) if not keys_ok(0, 0, d))
    rspan = next(-d for d in range(0, 2_000_000, 10) if not keys_ok(0, 1_500_000, 1_500_000 - d))
    lo, hi = 0, 1 << 33
    while hi - lo > 10:                                            # keys_ok is monotone in the start
        mid = fl10((lo + hi) // 2)
        lo, hi = (mid, hi) if keys_ok(0, mid, mid + 200) else (lo, mid)
    assert (span, rspan, hi) == (SPAN_FIRST_BAD, SPAN_REV_FIRST_BAD, START_FIRST_BAD), (span, rspan, hi)
    assert keys_ok(CHROM_FIRST_BAD - 1, 0, 200) and not keys_ok(CHROM_FIRST_BAD, 0, 200)
    return {"span": span, "reverse span": rspan, "start": hi, "chromosome": CHROM_FIRST_BAD}


def _ordinary_rows(rng, n=18, hi=900_000):
    rows = []
    for k in range(n):
        q, s = ((0, 1), (0, 1), (1, 0))[k % 3]
        ln = int(rng.integers(200, 3000))
        qs, ss = int(rng.integers(2000, hi)), int(rng.integers(2000, hi))
        rows.append((q, s, qs, qs + ln, ss + ln, ss) if rng.integers(0, 2) else (q, s, qs, qs + ln, ss, ss + ln))
    return rows


def length_edges():
    """query lengths 79 / 80 / 81 and max_len - 1 / max_len / max_len + 1: 80, 81 and max_len - 1 are emitted"""
    lens = (79, 80, 81, MAX_LEN - 1, MAX_LEN, MAX_LEN + 1)
    at = (10_000, 20_000, 30_000, 100_000, 200_000, 300_000)
    rows = [(0, 1, st + 1, st + ln, 2 * st + 1, 2 * st + ln) for ln, st in zip(lens, at)]
    c = make_case(rows, 2, max_len=MAX_LEN, lengths=lens)
    c["predicted"] = [absolute(c, 0, at[k], at[k] + lens[k]) for k in (3, 2, 1)]
    return c


def whole_segment():
    """the longest HSP a 1 Mbp segment holds, forward and reverse, beside ordinary rows: dropped by max_len, no error, and the
    other rows' intervals are what they are without it"""
    rng = np.random.default_rng(41)
    rows = _ordinary_rows(rng)
    plain = make_case(rows, 2)
    big = [(0, 1, 1, SEG_LEN, 1, SEG_LEN), (0, 1, 1, SEG_LEN, SEG_LEN, 1)]
    c = make_case(rows[:7] + big[:1] + rows[7:] + big[1:], 2, longest=SEG_LEN)
    c["predicted"] = twin(plain)
    assert len(c["predicted"]) >= 6
    return c


RESIDUES = (0, 1, 9)
SHIFTS = (-20, -11, -10, -1, 1, 10, 11, 19, 20)


def rounding():
    """stretches whose two ends are = 0, 1 and 9 mod 10 (query side of nine base rows), and followers from another query whose SUBJECT
    stretch is a base row's query stretch moved by up to 20 bases (SHIFTS) at either end or at both: a follower is new exactly when the
    move takes a rounded end out of reach of the base row's keys.  The followers' own query stretches lie 3 000 apart."""
    rows, bases = [], []
    for a in RESIDUES:
        for b in RESIDUES:
            st, en = 10_000 + 5_000 * len(bases) + a, 10_000 + 5_000 * len(bases) + 200 + b
            bases.append((st, en))
            rows.append((0, 2, st + 1, en, 500_000 + 1_000 * len(bases) + 1, 500_000 + 1_000 * len(bases) + 200))
    stretches = sorted((st + ds + 1, en + de) for st, en in bases
                       for ds, de in [(d, 0) for d in SHIFTS] + [(0, d) for d in SHIFTS] + [(d, d) for d in SHIFTS])
    k = len(stretches)
    for n, (ss, se) in enumerate(stretches):                       # q runs against s: every follower is a cluster of its own
        fq = 20_000 + 3_000 * (k - n)
        rows.append((1, 0, fq + 1, fq + 150, ss, se))
    c = make_case(rows, 3, bases=len(bases), followers=k)
    return c


def check_rounding_case():
    """plain statement of the first-come rule on this table: chains in order (query 0's rows, then query 1's in subject order),
    a chain is new when none of its eight keys was seen"""
    c = rounding()
    r = rows_of(c).tolist()
    nb = c["claim"]["bases"]
    seen, out = set(), []
    chains = r[:nb] + sorted(r[nb:], key=lambda x: (x[4], x[5]))
    for q, s, qs, qe, ss, se in chains:
        keys = set()
        for seg, st, en in ((s, ss - 1, se), (q, qs - 1, qe)):
            ch, a, b = absolute(c, seg, st, en)
            keys |= {(ch, x, y) for x in (fl10(a), fl10(a) + 10) for y in (fl10(b), fl10(b) + 10)}
        if not keys & seen:
            out.append(absolute(c, q, qs - 1, qe))
        seen |= keys
    new = set(out)
    assert set(twin(c)) == new and len(twin(c)) == len(out)
    nf = len([iv for iv in out if iv[0] == c["seg_chrom"][1] and iv[1] >= SEG_LEN])
    assert 0 < nf < c["claim"]["followers"]                        # some followers are new, some are not
    c["claim"]["new_followers"] = nf
    return c["claim"]


def one_rounded_subject(n_query=1000, per_query=5, seed=43):
    """n_query x per_query chains from different queries whose subject stretches differ base by base but share one rounded
    interval: every chain but the earliest meets its keys in the table (5 000 chains on the same four slots of the hash table)"""
    rng = np.random.default_rng(seed)
    nseg = n_query + 2
    ids = rng.permutation(nseg)
    subject = int(ids[n_query])
    rows = []
    for q in ids[:n_query]:
        for t in range(per_query):
            qs = 10_000 + 5_000 * t + int(rng.integers(0, 1000))
            rows.append((int(q), subject, qs, qs + 199, 500_001 + int(rng.integers(0, 10)), 500_300 + int(rng.integers(0, 10))))
    perm = rng.permutation(len(rows))
    c = make_case([rows[i] for i in perm], nseg, chains=len(rows))
    return c


def single_chain():
    c = make_case([(1, 0, 501, 900, 7001, 7400)], 2)
    c["predicted"] = [absolute(c, 1, 500, 900)]
    return c


def _guard_table(extra, seg_chrom=None, seg_off=None):
    rows = _ordinary_rows(np.random.default_rng(47), 9, hi=300_000)
    if seg_chrom is None:
        return make_case(rows[:4] + [extra] + rows[4:], 2)
    return make_case(rows[:4] + [extra] + rows[4:], seg_chrom=seg_chrom, seg_off=seg_off)


def guard_cases():
    """[(label, case inside the bound, case at the bound)]: the key-packing limits of pack_key, 10 bp apart"""
    far = START_FIRST_BAD - 354_550                                # offset of a segment that reaches the start bound
    out = []
    for label, mk in (
            ("subject span", lambda d: _guard_table((0, 1, 5001, 5200, 1, SPAN_FIRST_BAD + d))),
            ("query span", lambda d: _guard_table((0, 1, 1, SPAN_FIRST_BAD + d, 5001, 5200))),
            ("reverse subject span", lambda d: _guard_table((0, 1, 5001, 5200, 1 - SPAN_REV_FIRST_BAD + 10 + d, 10))),
            ("subject start", lambda d: _guard_table((0, 1, 5001, 5200, 354_551 + d, 354_750 + d), [0, 1], [0, far])),
            ("query start", lambda d: _guard_table((1, 0, 354_551 + d, 354_750 + d, 5001, 5200), [0, 1], [0, far])),
            ("chromosome id", lambda d: _guard_table((0, 1, 5001, 5200, 7001, 7200), [0, CHROM_FIRST_BAD + d // 10], [0, 0]))):
        out.append((label, mk(-10), mk(0)))
    return out


def _case_keys_ok(c):
    return all(keys_ok(*absolute(c, seg, st - 1, en)) for q, s, qs, qe, ss, se in rows_of(c).tolist()
               for seg, st, en in ((q, qs, qe), (s, ss, se)))


def limit_cases():
    return cached("limits", lambda: [("lengths", length_edges()), ("whole segment", whole_segment()), ("rounding", rounding()),
                                     ("one rounded subject", one_rounded_subject()), ("single chain", single_chain())])


def guards():
    return cached("guards", guard_cases)


def check_limit_cases():
    check_key_bounds()
    check_rounding_case()
    for label, c in limit_cases():
        if "predicted" in c:
            assert twin(c) == c["predicted"], label
        assert _case_keys_ok(c), label
    many = dict(limit_cases())["one rounded subject"]
    assert many["claim"]["chains"] == 5000 and len(twin(many)) == 1
    for label, inside, at in guards():
        assert _case_keys_ok(inside) and not _case_keys_ok(at), label
        assert len(twin(inside)) >= 5, label


def check_limits(fmea_chain):
    for label, c in limit_cases():
        compare(fmea_chain, c, label)


def check_guards(fmea_chain):
    """at a bound of pack_key the whole table is an error (RuntimeError), never a wrong interval; 10 bp inside it is answered, and
    so is a small case after every refused one"""
    for label, inside, at in guards():
        compare(fmea_chain, inside, label + ", 10 bp inside")
        try:
            got = run(fmea_chain, at)
        except RuntimeError:
            pass
        else:
            raise AssertionError("%s at the bound: no error, %d intervals" % (label, len(got)))
        compare(fmea_chain, small_case(), "small case after " + label)


# ------------------------------------------------------------------------------------------------------------------------------
# group E: table order
# ------------------------------------------------------------------------------------------------------------------------------
ORDERS = ("shuffled", "grouped", "grouped, self hits before new queries and pairs", "grouped, self hit first")


def _self_hit(q, k):
    a = 3_000 + 37 * k
    return (q, q, a, a + 400, a, a + 400)


def order_cases(seed=51):
    """one multiset of HSPs -- the rank case of 257 segments and a make_hsp_table table on the same segments -- in four orders;
    the exact self hits (dropped by the rule of Util.py:4138) sit where the shortcut of fm_first_kernel looks: directly before the
    first row of a query or of a pair, with that row's query"""
    import casegen

    base = ranks(257)
    seg_id = {}
    for i, (ch, off) in enumerate(zip(base["seg_chrom"].tolist(), base["seg_off"].tolist())):
        seg_id[("chr%d" % (ch + 1), off)] = i
    extra = []
    for qn, sn, qs, qe, ss, se in casegen.make_hsp_table(21, n_seg=3, n_fam=6, noise=30):
        (qc, qo), (sc, so) = qn.split("$"), sn.split("$")
        extra.append((seg_id[(qc, int(qo))], seg_id[(sc, int(so))], qs, qe, ss, se))
    rows = rows_of(base).tolist() + [list(r) for r in extra]
    rng = np.random.default_rng(seed)
    shuffled = [rows[i] for i in rng.permutation(len(rows))]
    fq, fp = {}, {}
    for i, r in enumerate(rows):                                   # grouped in the order the unshuffled table names them first
        fq.setdefault(r[0], i)
        fp.setdefault((r[0], r[1]), i)
    grouped = sorted(shuffled, key=lambda r: (fq[r[0]], fp[(r[0], r[1])]))
    with_self, n_q, n_p, n_own = [], 0, 0, 0
    for i, r in enumerate(grouped):
        new_q = i == 0 or grouped[i - 1][0] != r[0]
        new_p = not new_q and grouped[i - 1][1] != r[1]
        if new_q or (new_p and (i % 3 == 0 or r[1] == r[0])):
            with_self.append(_self_hit(r[0], i))                   # the self hit goes in front of its row
            n_q, n_p, n_own = n_q + new_q, n_p + new_p, n_own + (r[1] == r[0])
        with_self.append(r)
    self_first = [_self_hit(grouped[0][0], 0)] + grouped
    out = []
    for label, rws in zip(ORDERS, (shuffled, grouped, with_self, self_first)):
        out.append((label, with_rows(base, rws, order=label)))
    out[2][1]["claim"].update(self_before_query=n_q, self_before_pair=n_p, self_before_own_pair=n_own)
    out[3][1]["claim"].update(self_before_own_pair=int(grouped[0][1] == grouped[0][0]))
    return out


def orders():
    return cached("orders", order_cases)


def shortcut_first_rows(c, self_counts_as_kept=False):
    """first_q / first_pair as fm_first_kernel finds them: the minimum over the rows that do not skip the atomic -- a row skips it
    for the query (pair) when its predecessor is a KEPT row of the same query (pair).  self_counts_as_kept: the wrong kernel that
    does not look whether the predecessor is an exact self hit."""
    r = rows_of(c).tolist()
    is_self = [q == s and qs == ss and qe == se for q, s, qs, qe, ss, se in r]
    first_q, first_pair = {}, {}
    for i, row in enumerate(r):
        if is_self[i]:
            continue
        same_q = same_p = False
        if i > 0 and (self_counts_as_kept or not is_self[i - 1]):
            same_q = r[i - 1][0] == row[0]
            same_p = same_q and r[i - 1][1] == row[1]
        if not same_q:
            first_q[row[0]] = min(first_q.get(row[0], i), i)
        if not same_p:
            first_pair[(row[0], row[1])] = min(first_pair.get((row[0], row[1]), i), i)
    return first_q, first_pair


def check_order_cases():
    cases = orders()
    answers = [twin(c) for _label, c in cases]
    assert answers[0] != answers[1] and answers[1] == answers[2] == answers[3]      # order changes first appearance; self hits do not
    kept = [sorted(tuple(r) for r in rows_of(c).tolist() if not (r[0] == r[1] and r[2] == r[4] and r[3] == r[5])) for _l, c in cases]
    assert kept[0] == kept[1] == kept[2] == kept[3]                                  # one multiset
    skipped = []
    for label, c in cases:
        true = first_rows(c)
        assert shortcut_first_rows(c) == true, label
        wrong = shortcut_first_rows(c, self_counts_as_kept=True)
        skipped.append((len(true[0]) - len(wrong[0]), len(true[1]) - len(wrong[1])))
    cl = cases[2][1]["claim"]
    assert cl["self_before_query"] >= 250 and cl["self_before_pair"] >= 100 and cl["self_before_own_pair"] >= 3, cl
    # a kernel that took a self hit for a kept predecessor would lose these first appearances: every query whose first row follows
    # a self hit, and every pair (q, q) whose first row does (the self hit's own pair is (q, q))
    assert skipped[0] == skipped[1] == (0, 0) and skipped[3] == (1, cases[3][1]["claim"]["self_before_own_pair"]), skipped
    assert skipped[2][0] == cl["self_before_query"] and 3 <= skipped[2][1] <= cl["self_before_own_pair"], (skipped, cl)
    # the shortcut fires on the grouped tables and almost never on the shuffled one
    fires = []
    for _label, c in cases[:2]:
        r = rows_of(c)
        fires.append(int((r[1:, 0] == r[:-1, 0]).sum()))
    assert fires[0] * 20 < fires[1]
    return {"self hits before a query": cl["self_before_query"], "before a pair": cl["self_before_pair"], "same-query successors": fires}


def check_orders(fmea_chain):
    for label, c in orders():
        compare(fmea_chain, c, "order: " + label)


# ------------------------------------------------------------------------------------------------------------------------------
# the cases small enough for a fixture recorded from the reference's own python (oracle/gen_golden.py: gen_fmea_limits)
# ------------------------------------------------------------------------------------------------------------------------------
def fixture_cases():
    out = [(label, c) for label, c in sweep_cases()]
    out += [(label, c) for label, c in limit_cases() if label != "one rounded subject"]
    out.append(("one rounded subject, 100 x 3", one_rounded_subject(100, 3)))
    out += [("%s, 10 bp inside" % label, inside) for label, inside, _at in guards() if label != "chromosome id"]
    out.append(("filter pairs", filter_pairs()))
    out += [("ranks nseg=%d" % n, ranks(n)) for n in (3, 257)]
    return out


def segment_names(c):
    """the names 'chrom$offset' the reference reads the segments' places from"""
    return ["c%d$%d" % (ch, off) for ch, off in zip(c["seg_chrom"].tolist(), c["seg_off"].tolist())]


def fixture_record(label, c, expected):
    return {"label": label, "rows": rows_of(c).tolist(), "seg_chrom": c["seg_chrom"].tolist(), "seg_off": c["seg_off"].tolist(),
            "skip_gap": c["skip_gap"], "max_len": c["max_len"], "expected": list(expected)}


def case_of_record(rec):
    return make_case(rec["rows"], skip_gap=rec["skip_gap"], max_len=rec["max_len"], seg_chrom=rec["seg_chrom"], seg_off=rec["seg_off"])


def check_fixture(fmea_chain, records):
    """the recorded tables are today's tables, and fmea_chain gives what the reference gave"""
    today = dict(fixture_cases())
    assert sorted(today) == sorted(r["label"] for r in records)
    for rec in records:
        c = case_of_record(rec)
        assert np.array_equal(rows_of(c), rows_of(today[rec["label"]])), rec["label"]
        got = run(fmea_chain, c)
        assert got == parse_names(rec["expected"]), rec["label"]
