"""Inputs of the star alignment's layout / fill edge tests, shared by the CPU check of the cases themselves (test_star_layout_cases.py)
and the device tests (test_gpu_star_layout.py): groups of windows (row 0 = the centre) built to cross the fixed capacities of
hite_msa.hip / hite_fill.h -- the kept-block list of a layout round (LAY_KW_LIST), the deferred-block list of a fill workgroup
(FILL_DEFER_CAP), the rows cached in LDS (MSA_MAXR), the 64-row trips of the k-th-largest loop, the 1024- / 256-position rounds of
the layout kernels, dropped rows and pads on the 64-position trips of ops_pad_fix_kernel.  Every case carries the figures the TWIN
(oracle/hite_oracle_msa.c) gave for it -- measured with layout_profile below from the twin's full alignment, plain numpy -- so that a
changed generator cannot silently turn a case into one that stays on the near side of its limit.  No GPU import here."""
import numpy as np

import casegen

# the capacities the cases are built around (hite_amd/csrc/hite_msa.hip)
LAY_KW_LIST = 256        # kept-block positions of one sparse layout round that go through the LDS list
LAY_ROUND = 1024         # positions per round of star_layout_sparse_kernel (256 of star_layout_kernel)
FILL_DEFER_CAP = 1024    # deferred (row, position) items per workgroup of star_fill_sparse_kernel
FILL_GRID_Y = 4          # workgroups that share the rows of a candidate: a workgroup owns the rows y, y + 4, ...
MSA_MAXR = 128           # rows whose lengths are cached in LDS
LONG_WIN = 1536          # a window longer than this selects star_fill_sparse_kernel<8> for the whole launch

GAP = ord("-")


# ---- measurements on the twin's full alignment -------------------------------------------------------------------------------------
def layout_profile(full, R=None):
    """From a FULL alignment (R x cols, row 0 = the centre): m, per centre position p = 0..m the number of rows r >= 1 with a base in
    the insertion block in front of p (`count`), the widest and the h-th largest insertion there (h = (R + 1) >> 1: the fewest rows
    for a column to survive), the kept-block positions (count >= h) and their number per round p // 1024, and whether block m has an
    extra last column (widest insertion > h-th largest)."""
    full = np.asarray(full)
    if R is None:
        R = full.shape[0]
    assert full.shape[0] == R and R >= 1
    centre = full[0] != GAP
    m = int(centre.sum())
    h = (R + 1) >> 1
    icols = np.flatnonzero(~centre)                                      # the insertion columns
    block = (np.cumsum(centre) - centre)[icols]                          # and the block (0..m) each belongs to: centre columns in front of it
    ins = np.zeros((m + 1, max(R - 1, 0)), np.int64)
    np.add.at(ins, block, (full[1:, icols] != GAP).T.astype(np.int64))
    ins = ins.T                                                          # (R - 1) x (m + 1): bases of row r in the block in front of p
    count = (ins > 0).sum(axis=0)
    widest = ins.max(axis=0) if R > 1 else np.zeros(m + 1, np.int64)
    kth = np.sort(ins, axis=0)[R - 1 - h] if R - 1 >= h else np.zeros(m + 1, np.int64)
    kept = np.flatnonzero(count >= h) if R > 1 else np.zeros(0, np.int64)
    per_round = np.bincount(kept // LAY_ROUND, minlength=m // LAY_ROUND + 1).tolist()
    return dict(m=m, R=R, h=h, ins=ins, count=count, widest=widest, kth=kth, kept=kept, per_round=per_round,
                last_widest=int(widest[m]), last_kth=int(kth[m]), extra_last=bool(widest[m] > kth[m]))


def plain_sparse_keep(full):
    """remove_sparse_col_in_align_file's rule itself: a column is kept iff it is the first, the last, or 2 * gaps <= rows"""
    full = np.asarray(full)
    keep = 2 * (full == GAP).sum(axis=0) <= full.shape[0]
    keep[0] = keep[-1] = True
    return keep.astype(np.uint8)


def defer_items(prof):
    """(row, position) items the fullest workgroup of star_fill_sparse_kernel collects: its rows x the positions that keep insertion
    columns (the kept blocks, block 0 where the first column is an insertion column, block m where there is an extra last column)"""
    m = prof["m"]
    pos = set(prof["kept"].tolist())
    if prof["widest"][0] > 0:
        pos.add(0)
    if prof["extra_last"]:
        pos.add(m)
    return -(-prof["R"] // FILL_GRID_Y) * len(pos)


def lead_gap_positions(full, r):
    """centre positions in front of the first base of row r (what ops_pad_fix_kernel's front loop rewrites for a padded row)"""
    cols = np.flatnonzero(full[0] != GAP)
    nz = np.flatnonzero(full[r] != GAP)
    return int((cols < nz[0]).sum()) if len(nz) else len(cols)


def trail_gap_positions(full, r):
    cols = np.flatnonzero(full[0] != GAP)
    nz = np.flatnonzero(full[r] != GAP)
    return int((cols > nz[-1]).sum()) if len(nz) else len(cols)


def ungapped(row):
    return bytes(row[row != GAP])


def strip_pads(w):
    """the window without the pad bytes it begins and ends with ('.' or a base in lower case, include/hite_gpu.h)"""
    return w.strip(".acgtn")


# ---- generators ----------------------------------------------------------------------------------------------------------------------
def thinned(F, start, k):
    """F without every third base over F[start : start + 3 k]"""
    return F[:start] + "".join(F[start + i] for i in range(3 * k) if i % 3 != 2) + F[start + 3 * k:]


def kwlist_group(seed, k, R, tail=0, head=0, k_head=0):
    """a. the centre lacks every third base of the family over 3 k bases: (nearly) every second centre position has an insertion block
    that ALL rows share -- more kept-block positions in one round than LAY_KW_LIST holds.  head > 0: that stretch begins behind
    `head` bases (of which the first 3 k_head are thinned as well): the full list falls into a later round."""
    rng = np.random.default_rng(seed)
    F = casegen.rand_seq(rng, head + 3 * k + tail)
    centre = thinned(thinned(F, head, k), 0, k_head)
    return [centre] + [F] * (R - 1)


def defer_group(seed, R, n_del=52, every=12, tail=76, sub=0.02):
    """b. the centre lacks one base of the family every 12, 52 of them; R - 1 rows of the family at 2 % substitutions: blocks that
    every row shares, rows x blocks items in each fill workgroup"""
    rng = np.random.default_rng(seed)
    F = casegen.rand_seq(rng, n_del * every + tail)
    centre = "".join(c for i, c in enumerate(F) if not (i < n_del * every and i % every == every - 1))
    return [centre] + [casegen.mutate(rng, F, sub) for _ in range(R - 1)]


def rows_group(seed, R, m, n_pos=40, ins_max=6, lead_max=2, trail="random", lo=3, hi=None, also=()):
    """c / d. rows = the centre with insertions of random length 0..ins_max at n_pos positions the rows share (so the h-th largest is a
    real order statistic), a leading insertion of 0..lead_max bases and a trailing one: trail = "random" (0..4 per row), "none"
    (block m stays empty), "one" (a single row: widest > h-th largest = 0), "ragged" (every row 1, one row 3: widest > h-th > 0),
    "pivot" (below); also = positions that are among the shared ones whatever the draw (those beside a round edge).

    "pivot": exactly h = (R + 1) >> 1 rows end with 3 bases (one of them with 4), the others with 1: the h-th largest insertion
    behind the last centre position is 3 only if EVERY one of the h rows is counted, the widest is 4 through one row alone.  The h
    rows include all rows from MSA_MAXR on (whose lengths the layout reads from global memory, not from LDS), the single row is
    row MSA_MAXR (the last row below that): a wrong length of any such row moves the last columns.  The odd rows from MSA_MAXR on
    carry no shared insertions: they are far shorter than the row whose cached length a wrong index would take."""
    rng = np.random.default_rng(seed)
    centre = casegen.rand_seq(rng, m)
    hi = m - 3 if hi is None else hi
    pos = np.sort(rng.choice(np.arange(lo, hi), size=min(n_pos, max(hi - lo, 0)), replace=False)) if hi > lo else np.zeros(0, np.int64)
    pos = np.unique(np.concatenate([pos, np.asarray([p for p in also if 0 < p < m], np.int64)]))
    rows = [centre]
    h, beyond = (R + 1) >> 1, max(R - MSA_MAXR, 0)
    for r in range(1, R):
        parts, at = [], 0
        parts.append(casegen.rand_seq(rng, int(rng.integers(0, lead_max + 1))))
        short = trail == "pivot" and r >= MSA_MAXR and r % 2 == 1
        for i, p in enumerate(pos):
            parts.append(centre[at:p])
            n = 0 if short else int(rng.integers(0, ins_max + 1))
            # every other position: a run of one base that neither neighbour in the centre has -- the aligner cannot slide or split it, the
            # block keeps the drawn lengths; the others: random bases, which the unit-cost alignment spreads over the neighbouring positions
            parts.append(casegen.rand_seq(rng, n) if i % 2 else [b for b in "ACGT" if b not in (centre[p - 1], centre[p])][0] * n)
            at = int(p)
        parts.append(centre[at:])
        t = int(rng.integers(0, 5))
        if trail == "none":
            t = 0
        elif trail == "one":
            t = 2 if r == 1 else 0
        elif trail == "ragged":
            t = 3 if r == 1 else 1
        elif trail == "pivot":
            t = 4 if r == min(MSA_MAXR, R - 1) else 3 if (r >= MSA_MAXR or r <= h - beyond - (R <= MSA_MAXR)) else 1
        parts.append(casegen.rand_seq(rng, t) if trail == "random" else not_last(centre, rng, t))
        rows.append("".join(parts))
    return rows


def not_last(centre, rng, n):
    """n random bases, none of which is the centre's last base (a trailing insertion that cannot slide into the last centre column)"""
    alt = [b for b in "ACGT" if b != centre[-1]]
    return "".join(alt[i] for i in rng.integers(0, 3, n))


def tiny_group(seed, R, m, trail):
    """d. degenerate centres of 1..3 bases: every row is the centre between a leading and (trail) a trailing insertion"""
    rng = np.random.default_rng(seed)
    centre = casegen.rand_seq(rng, m)
    alt = [b for b in "ACGT" if b != centre[0]]
    rows = [centre]
    for r in range(1, R):
        lead = "".join(alt[i] for i in rng.integers(0, 3, int(rng.integers(0, 3))))
        t = 0 if trail == "none" else (3 if r == 1 else 1)
        rows.append(lead + centre + not_last(centre, rng, t))
    return rows


def dropped_groups(seed):
    """e. ONE call: 140 rows of which rows 1, 64, 129 and the last are shorter than half the centre (dropped by the aligner: one of
    them beyond row 128, where the row map is read from global memory), a group that loses no row (its candidate is not compacted),
    and a group whose rows are ALL too short: the centre alone is left"""
    big = rows_group(seed, 136, 300, trail="pivot")             # the rows that stay: row 128 of the alignment is row 130 of the input
    for r in (1, 64, 129, 139):
        big.insert(r, big[r - 1][-100:])
    whole = rows_group(seed + 1, 9, 300)
    alone = rows_group(seed + 2, 6, 300)
    alone = [alone[0]] + [w[:100 + 3 * i] for i, w in enumerate(alone[1:])]
    return [big, whole, alone]


PAD_LENS = (63, 64, 65, 128, 130)


def pad_groups(seed):
    """f. the rows of a rows_group (7 rows) with front pads '.' of 63, 64, 65, 128 and 130 bytes in place of that many of their bases --
    the 64-position trips of ops_pad_fix_kernel end exactly on, one short of and one past the pad -- and a sixth row that carries
    the centre's own first 64 bases in lower case instead; a second group with the same pads behind; a third with pads at both
    ends.  No leading / trailing insertions and no shared insertion within 140 positions of either end: the pad of n bytes faces
    exactly n centre positions."""
    base = rows_group(seed, 7, 420, n_pos=30, lead_max=0, trail="none", lo=140, hi=280)
    c = base[0]
    front = [c] + ["." * n + w[n:] for n, w in zip(PAD_LENS, base[1:6])] + [c[:64].lower() + base[6][64:]]
    back = [c] + [w[:len(w) - n] + "." * n for n, w in zip(PAD_LENS, base[1:6])] + [base[6][:len(base[6]) - 64] + c[-64:].lower()]
    both = [c] + ["." * a + w[a:len(w) - b] + "." * b for (a, b), w in zip([(64, 128), (128, 64), (64, 64), (65, 63), (1, 130)], base[1:6])]
    both.append(c[:128].lower() + base[6][128:len(base[6]) - 128] + c[-128:].lower())
    return [front, back, both]


def long_group(seed=4100):
    """a group with a window longer than LONG_WIN: its presence makes the whole launch run star_fill_sparse_kernel<8>"""
    return rows_group(seed, 4, 1600, n_pos=25)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
# label -> builder of the groups of ONE call (a group of its own, or its own small family)
EDGES = (255, 256, 1023, 1024, 2047, 2048)          # shared insertion positions beside the round edges of both layout kernels
SPARSE_M = (1022, 1023, 1024, 1025, 1027, 2047, 2048, 2049)
FULL_M = (255, 256, 257)
ROWS_R = (63, 64, 65, 66, 127, 128, 129, 130, 200)
KW_EXACT = {255: (2266, 266), 256: (1268, 268), 257: (5267, 267), 258: (1274, 274)}      # kept blocks in round 0 -> (seed, k), R = 3


def _edge_pair(m, i):
    """two groups with a centre of m bases: one with an extra last column, one whose block m is empty"""
    return [rows_group(5000 + m, 3 + i % 6, m, trail=("one", "ragged")[i % 2], also=EDGES + (m - 1,)),
            rows_group(6000 + m, 8 - i % 6, m, trail="none", also=EDGES + (m - 1,))]


BUILDERS = {}
for _R in (2, 3, 5):
    BUILDERS["kwlist_R%d" % _R] = lambda R=_R: [kwlist_group(300 + R, 300, R)]
for _n, (_s, _k) in KW_EXACT.items():
    BUILDERS["kwlist_%d" % _n] = lambda s=_s, k=_k: [kwlist_group(s, k, 3, tail=60)]
BUILDERS["kwlist_round1"] = lambda: [kwlist_group(77, 300, 3, tail=40, head=1030, k_head=30)]
for _R in (101, 77, 73):
    BUILDERS["defer_R%d" % _R] = lambda R=_R: [defer_group(500 + R, R)]
for _R in ROWS_R:
    BUILDERS["rows_R%d" % _R] = lambda R=_R: [rows_group(2000 + R, R, 300, trail="pivot")]
for _i, _m in enumerate(SPARSE_M + FULL_M):
    BUILDERS["edge_m%d" % _m] = lambda m=_m, i=_i: _edge_pair(m, i)
BUILDERS["edge_R129_m1024"] = lambda: [rows_group(7000, 129, 1024, trail="pivot", also=EDGES)]
BUILDERS["tiny"] = lambda: [tiny_group(8001, 3, 1, "ragged"), tiny_group(8002, 2, 1, "none"), tiny_group(8003, 4, 2, "ragged"),
                            tiny_group(8004, 3, 2, "none"), tiny_group(8005, 3, 3, "ragged"), tiny_group(8006, 4, 3, "none"),
                            tiny_group(8007, 2, 3, "ragged")]
BUILDERS["dropped"] = lambda: dropped_groups(3000)
BUILDERS["pads"] = lambda: pad_groups(3100)
LABELS = list(BUILDERS)

_GROUPS = {}


def groups(label):
    if label not in _GROUPS:
        _GROUPS[label] = BUILDERS[label]()
    return _GROUPS[label]


# What the twin gave, per group of each case: (rows kept, m, columns of the full alignment, kept-block positions per round,
# (widest, h-th largest) insertion behind the last centre position, defer_items).  A record of the reference.
TWIN = {
    "kwlist_R2": [(2, 600, 900, [281], (1, 1), 281)],
    "kwlist_R3": [(3, 600, 900, [286], (1, 1), 286)],
    "kwlist_R5": [(5, 600, 900, [284], (1, 1), 568)],
    "kwlist_255": [(3, 592, 858, [255], (0, 0), 255)],
    "kwlist_256": [(3, 596, 864, [256], (0, 0), 256)],
    "kwlist_257": [(3, 594, 861, [257], (0, 0), 257)],
    "kwlist_258": [(3, 608, 882, [258], (0, 0), 258)],
    "kwlist_round1": [(3, 1640, 1970, [39, 272], (0, 0), 311)],
    "defer_R101": [(101, 648, 823, [52], (0, 0), 1352)],
    "defer_R77": [(77, 648, 807, [52], (0, 0), 1040)],
    "defer_R73": [(73, 648, 801, [52], (0, 0), 988)],
    "rows_R63": [(63, 300, 882, [42], (4, 3), 672)],
    "rows_R64": [(64, 300, 848, [45], (4, 3), 720)],
    "rows_R65": [(65, 300, 844, [44], (4, 3), 748)],
    "rows_R66": [(66, 300, 861, [45], (4, 3), 765)],
    "rows_R127": [(127, 300, 936, [43], (4, 3), 1376)],
    "rows_R128": [(128, 300, 924, [45], (4, 3), 1440)],
    "rows_R129": [(129, 300, 911, [44], (4, 3), 1452)],
    "rows_R130": [(130, 300, 894, [45], (4, 3), 1485)],
    "rows_R200": [(200, 300, 920, [40], (4, 3), 2000)],
    "edge_m1022": [(3, 1022, 1231, [33], (2, 0), 34), (8, 1022, 1380, [49], (0, 0), 98)],
    "edge_m1023": [(4, 1023, 1260, [43], (3, 1), 44), (7, 1023, 1358, [43], (0, 0), 86)],
    "edge_m1024": [(5, 1024, 1311, [35, 0], (2, 0), 72), (6, 1024, 1336, [44, 0], (0, 0), 90)],
    "edge_m1025": [(6, 1025, 1330, [47, 2], (3, 1), 98), (5, 1025, 1307, [36, 1], (0, 0), 74)],
    "edge_m1027": [(7, 1027, 1373, [40, 2], (2, 0), 88), (4, 1027, 1280, [39, 1], (0, 0), 41)],
    "edge_m2047": [(8, 2047, 2405, [18, 34], (3, 1), 104), (3, 2047, 2216, [15, 15], (0, 0), 30)],
    "edge_m2048": [(3, 2048, 2276, [16, 21, 0], (2, 0), 38), (8, 2048, 2394, [23, 25, 0], (0, 0), 96)],
    "edge_m2049": [(4, 2049, 2280, [23, 32, 2], (3, 1), 57), (7, 2049, 2428, [28, 11, 0], (0, 0), 78)],
    "edge_m255": [(5, 255, 499, [36], (2, 0), 76), (6, 255, 508, [38], (0, 0), 76)],
    "edge_m256": [(6, 256, 554, [43], (3, 1), 86), (5, 256, 523, [36], (0, 0), 74)],
    "edge_m257": [(7, 257, 590, [39], (2, 0), 80), (4, 257, 511, [43], (0, 0), 43)],
    "edge_R129_m1024": [(129, 1024, 1674, [44, 1], (4, 3), 1485)],
    "tiny": [(3, 1, 5, [1], (3, 1), 2), (2, 1, 1, [0], (0, 0), 0), (4, 2, 7, [2], (3, 1), 2), (3, 2, 4, [1], (0, 0), 1), (3, 3, 7, [1], (3, 1), 2), (4, 3, 5, [1], (0, 0), 1), (2, 3, 8, [2], (3, 3), 2)],
    "dropped": [(136, 300, 885, [47], (4, 3), 1598), (9, 300, 634, [41], (4, 1), 123), (1, 300, 300, [0], (0, 0), 0)],
    "pads": [(7, 420, 663, [21], (0, 0), 42), (7, 420, 663, [21], (0, 0), 42), (7, 420, 663, [21], (0, 0), 42)],
}

LONG_TWIN = (4, 1600, 1733, [14, 14], (1, 0), 29)      # long_group(), as above
# the cases whose own call holds a window above LONG_WIN already (star_fill_sparse_kernel<8> in both runs); all others run <4> alone
OWN_CALL_LONG = ["kwlist_round1", "edge_m2047", "edge_m2048", "edge_m2049"]

_TWIN_RUN = {}


def twin_full(group):
    """oracle_lib.star_msa(group) from ONE run of the twin (star_msa asks for the size first and aligns every pair twice): the buffer
    holds the widest alignment the windows can give -- a column is the centre's or holds a base of some row"""
    import ctypes as C

    import oracle_lib as O

    wb = [w.encode() for w in group]
    off = np.zeros(len(wb) + 1, dtype=np.int64)
    np.cumsum([len(w) for w in wb], out=off[1:])
    buf = np.frombuffer(b"".join(wb), dtype=np.uint8)
    out = np.empty(len(wb) * int(off[-1]), dtype=np.uint8)
    cols, kept = C.c_int(0), C.c_int(0)
    rc = O.lib().orc_star_msa2(O._ptr(buf, O.u8p), O._ptr(off, O.i64p), len(wb), C.byref(cols), C.byref(kept), O._ptr(out, O.u8p), C.c_int64(out.size))
    assert rc == 0, rc
    return out[:kept.value * cols.value].reshape(kept.value, cols.value).copy()


def twin(label):
    """[(full alignment, layout_profile)] of the case's groups from the twin, computed once and left unchanged"""
    if label not in _TWIN_RUN:
        res = []
        for g in groups(label):
            full = twin_full(g)
            full.setflags(write=False)
            res.append((full, layout_profile(full)))
        _TWIN_RUN[label] = res
    return _TWIN_RUN[label]


def measured(prof, full):
    return (full.shape[0], prof["m"], full.shape[1], prof["per_round"], (prof["last_widest"], prof["last_kth"]), defer_items(prof))


def order_statistic_positions(prof):
    """kept-block positions where the h-th largest insertion is neither the widest nor 1: the k-th-largest loop has to count"""
    k = prof["kept"]
    return int(((prof["kth"][k] > 1) & (prof["kth"][k] < prof["widest"][k])).sum())


def pivot_last_block(prof):
    """rows_group(trail="pivot") came through the aligner as built: behind the last centre position exactly h rows hold more than one
    base (3, one of them 4) and, beyond MSA_MAXR rows, row MSA_MAXR is the widest and every later row is among the h"""
    last = prof["ins"][:, prof["m"]]                       # (row r is entry r - 1)
    ok = (prof["last_widest"], prof["last_kth"]) == (4, 3) and int((last > 1).sum()) == prof["h"] and int((last == 4).sum()) == 1
    if prof["R"] > MSA_MAXR:
        ok = ok and last[MSA_MAXR - 1] == 4 and bool((last[MSA_MAXR - 1:] >= 3).all())
    return bool(ok)


def check_precondition(label, run=None):
    """the limit the case exists for, measured on the twin alone -- asserted with the recorded figures (TWIN) and as the relation to
    the capacity it is about.  Both test files call this: the device never runs a weaker case than the CPU run checked."""
    run = twin(label) if run is None else run
    gs = groups(label)
    got = [measured(p, f) for f, p in run]
    assert got == TWIN[label], (label, got)
    profs = [p for _, p in run]
    fulls = [f for f, _ in run]
    kind = label.split("_")[0]
    if kind == "kwlist":
        p = profs[0]
        assert fulls[0].shape[0] == len(gs[0])
        if label == "kwlist_round1":
            assert p["m"] > 1300 and 0 < p["per_round"][0] < LAY_KW_LIST < p["per_round"][1]
        elif label[7:].isdigit():
            assert p["per_round"] == [int(label[7:])]
        else:
            assert p["m"] == 600 and fulls[0].shape[1] == 900 and p["per_round"][0] > LAY_KW_LIST
    elif kind == "defer":
        p = profs[0]
        R = int(label[7:])
        assert p["R"] == R and p["m"] == 648 and len(p["kept"]) == 52
        assert defer_items(p) == {101: 1352, 77: 1040, 73: 988}[R] and (defer_items(p) > FILL_DEFER_CAP) == (R != 73)
    elif kind == "rows":
        p = profs[0]
        assert p["R"] == int(label[6:]) == len(gs[0]) and p["m"] == 300
        assert order_statistic_positions(p) >= 15 and p["extra_last"] and p["widest"][0] > 0 and pivot_last_block(p)
    elif kind == "edge":
        if label == "edge_R129_m1024":
            assert profs[0]["R"] == 129 and profs[0]["m"] == 1024 and len(profs[0]["per_round"]) == 2 and order_statistic_positions(profs[0]) >= 15
            assert pivot_last_block(profs[0])
        else:
            m = int(label[6:])
            assert [p["m"] for p in profs] == [m, m] and all(p["R"] == len(g) <= 8 for p, g in zip(profs, gs))
            assert profs[0]["extra_last"] and profs[1]["last_widest"] == 0
    elif kind == "tiny":
        assert [(p["m"], p["R"]) for p in profs] == [(1, 3), (1, 2), (2, 4), (2, 3), (3, 3), (3, 4), (3, 2)]
        assert [p["extra_last"] for p in profs] == [True, False, True, False, True, False, False]
        assert [p["last_widest"] for p in profs] == [3, 0, 3, 0, 3, 0, 3]
    elif kind == "dropped":
        assert [f.shape[0] for f in fulls] == [136, len(gs[1]), 1] and len(gs[0]) == 140 and len(gs[2]) > 1
        assert pivot_last_block(profs[0])                      # rows 128 .. 135 of the alignment are rows 130 .. 138 of the input
    elif kind == "pads":
        for f, g in zip(fulls, gs):
            assert f.shape[0] == len(g) and not (f & 0x20)[f != GAP].any()
        lead = [[lead_gap_positions(f, r) for r in range(1, 7)] for f in fulls]
        trail = [[trail_gap_positions(f, r) for r in range(1, 7)] for f in fulls]
        assert lead == [list(PAD_LENS) + [64], [0] * 6, [64, 128, 64, 65, 1, 128]]
        assert trail == [[0] * 6, list(PAD_LENS) + [64], [128, 64, 64, 63, 130, 128]]
    else:
        raise AssertionError(label)
