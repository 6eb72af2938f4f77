"""Inputs of the tile form of the sparse fill (hite_fill_tile.h, star_fill_tile_kernel) at ITS limits, shared by the CPU check of the
per-tile body (test_host_fill_tiles.py) and the device test (test_gpu_fill_tiles.py): centres that end beside a tile edge, kept
insertion blocks at a tile's first and last position and at position 0, rows that are all gaps over a whole tile or begin / end
exactly at a tile edge, a row whose window range for one tile is one short of, equal to and one past the LDS slot, tiles that keep
no column or exactly one, output rows at every residue mod 16 with 1 .. 33 kept columns, row counts around the rows a workgroup
takes per trip, front pads whose first real base lies in the second tile.

The limits (T = positions of a tile, SLOT = bytes of the slot, ROWS = rows per trip, Z = row slices) are arguments: the tests read
them from the build.  Every case carries a precondition that is checked on the TWIN's alignment alone (derive / tile_widths /
row_ranges below mirror the layout words and the ops, not the kernel): a case must not pass because it missed its limit.
No GPU import here."""
import numpy as np

import casegen
import star_layout_cases as SC

GAP = SC.GAP


# ---- what the fill reads, derived from the twin's FULL alignment ------------------------------------------------------------------------
def derive(full):
    """rows (without gaps), ops (R x m, row 0 unused), the op before position 0, layout words, last_extra, the kept columns and the
    sparse alignment -- from the twin's full alignment and the twin's column selection"""
    import oracle_lib as O

    full = np.ascontiguousarray(full)
    R = full.shape[0]
    centre = full[0] != GAP
    m = int(centre.sum())
    ccols = np.flatnonzero(centre)
    keep = O.sparse_cols(full).astype(bool)
    assert np.array_equal(keep, SC.plain_sparse_keep(full).astype(bool))
    isb = full != GAP
    before_b = np.cumsum(isb, axis=1) - isb                       # bases of the row in front of each column
    ops = np.zeros((R, m), np.uint16)
    for r in range(1, R):
        ops[r] = before_b[r, ccols] | ((~isb[r, ccols]).astype(np.uint16) << 15)
    blk = (np.cumsum(centre) - centre)[~centre]                   # block (0..m) of every insertion column
    mx = np.bincount(blk, minlength=m + 1)
    fs = np.concatenate([[0], np.cumsum(mx + (np.arange(m + 1) < m))])
    assert fs[-1] == full.shape[1]
    before = np.concatenate([[0], np.cumsum(keep)])
    lay = np.zeros(m + 1, np.uint32)
    le = -1
    for p in range(m + 1):
        b = keep[fs[p]:fs[p] + mx[p]]
        kw = int(b.sum())
        if p == m and mx[p] > 0 and not b[:kw].all():
            kw -= 1                                               # the forced last column is not part of the prefix
        if p == m and mx[p] > 0 and kw < mx[p] and keep[fs[p] + mx[p] - 1]:
            le = int(mx[p]) - 1
        assert b[:kw].all() and not b[kw:mx[p] - (1 if (p == m and le >= 0) else 0)].any(), p
        keepc = int(keep[fs[p] + mx[p]]) if p < m else 0
        lay[p] = kw | (keepc << 15) | (int(before[fs[p]]) << 16)
    return dict(R=R, m=m, rows=[SC.ungapped(full[r]) for r in range(R)], ops=ops, lay=lay, le=le, C=int(keep.sum()),
                exp=np.ascontiguousarray(full[:, keep]), prof=SC.layout_profile(full), full=full)


def tile_widths(d, T):
    """kept columns of every tile of T positions"""
    m, first = d["m"], (d["lay"] >> 16).astype(np.int64)
    edges = [int(first[P0]) for P0 in range(0, m + 1, T)] + [d["C"]]
    return [edges[i + 1] - edges[i] for i in range(len(edges) - 1)]


def _end(o):
    return int(o & 0x7fff) + (0 if (o >> 15) else 1)


def row_ranges(d, r, T):
    """bytes of row r that each tile needs: from the end of the op before the tile to the end of its last op (the row's end behind
    the last position)"""
    m, o, n = d["m"], d["ops"][r], len(d["rows"][r])
    out = []
    for P0 in range(0, m + 1, T):
        pl = min(P0 + T - 1, m)
        a = P0 if r == 0 else (0 if P0 == 0 else _end(o[P0 - 1]))
        e = (pl + 1 if pl < m else m) if r == 0 else (_end(o[pl]) if pl < m else n)
        out.append(e - a)
    return out


# ---- generators ----------------------------------------------------------------------------------------------------------------------------
def _foreign(centre, p):
    """a base that neither neighbour of the insertion point p has: a run of it can neither slide nor split"""
    near = {centre[p - 1] if p > 0 else centre[0], centre[p] if p < len(centre) else centre[-1]}
    return [b for b in "ACGT" if b not in near][0]


def ins_group(seed, R, m, at, n=2):
    """every row but the last = the centre with a run of n foreign bases in front of each position of `at`: kept insertion blocks"""
    rng = np.random.default_rng(seed)
    centre = casegen.rand_seq(rng, m)
    rows = [centre]
    for r in range(1, R):
        s, last = [], 0
        for p in sorted(at):
            s.append(centre[last:p])
            if r < R - 1 or R <= 3:
                s.append(_foreign(centre, p) * n)
            last = p
        s.append(centre[last:])
        rows.append("".join(s))
    return rows


def cut_group(seed, m, cuts, copies):
    """the centre, one row per (a, b) of `cuts` = centre[a:b] between a pads in front and m - b pads behind (a pad never matches: the
    row stays on the diagonal and its pads become gaps), and `copies` rows equal to the centre with 2 % substitutions"""
    rng = np.random.default_rng(seed)
    centre = casegen.rand_seq(rng, m)
    return [centre] + ["." * a + centre[a:b] + "." * (m - b) for a, b in cuts] + [casegen.mutate(rng, centre, 0.02) for _ in range(copies)]


def slot_group(seed, T, SLOT, d, R=6):
    """m = T + 100; row 2 carries ONE run of SLOT - T + d foreign bases in the middle of tile 0: its range for that tile is SLOT + d"""
    rng = np.random.default_rng(seed)
    centre = casegen.rand_seq(rng, T + 100)
    at = T // 2
    rows = [centre] + [casegen.mutate(rng, centre, 0.01) for _ in range(R - 1)]
    rows[2] = centre[:at] + _foreign(centre, at) * (SLOT - T + d) + centre[at:]
    return rows


def hole_group(seed, T):
    """m = 3 T - 1, 5 rows: three end with pads from position T - 8 on, one equals the centre: the second tile keeps no column, the
    third only the last column of the alignment (which is kept whatever it holds)"""
    rng = np.random.default_rng(seed)
    centre = casegen.rand_seq(rng, 3 * T - 1)
    return [centre] + [centre[:T - 8] + "." * (2 * T + 7)] * 3 + [centre]


def width_groups(seed, R=17):
    """33 candidates of R rows without a gap, C = 1 .. 33 kept columns: row r begins at r C mod 16"""
    rng = np.random.default_rng(seed)
    out = []
    for C in range(1, 34):
        centre = casegen.rand_seq(rng, C)
        rows = [centre]
        for r in range(1, R):
            s = list(centre)
            if C > 6:
                k = int(rng.integers(1, C - 1))
                s[k] = "ACGT"[("ACGT".index(s[k]) + 1) % 4]
            rows.append("".join(s))
        out.append(rows)
    return out


def pad_group(seed, T):
    """m = 2 T + 100, 8 rows: rows 1 .. 3 begin with 63, 64 and 65 pad bytes and then face the centre from position T + 10 on"""
    rng = np.random.default_rng(seed)
    centre = casegen.rand_seq(rng, 2 * T + 100)
    return [centre] + ["." * n + centre[T + 10:] for n in (63, 64, 65)] + [casegen.mutate(rng, centre, 0.02) for _ in range(4)]


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
def builders(T, SLOT, ROWS, Z):
    """label -> (builder of the groups of one call, precondition on [derive(twin's alignment)] of these groups)"""
    B = {}

    def add(label, build, pre):
        B[label] = (build, pre)

    # centre length at the tile edges, with and without an extra last column
    for i, m1 in enumerate((T - 1, T, T + 1, 2 * T, 2 * T + 1)):
        m = m1 - 1

        def pre_edge(ds, m=m):
            assert [d["m"] for d in ds] == [m, m] and ds[0]["le"] >= 0 and ds[1]["le"] < 0 and ds[1]["prof"]["last_widest"] == 0
            assert len(tile_widths(ds[0], T)) == m // T + 1
        add("edge_m%d" % m, lambda m=m, i=i: [SC.rows_group(9000 + m, 3 + i, m, trail=("one", "ragged")[i % 2], also=(T - 1, T, 2 * T - 1, 2 * T)),
                                             SC.rows_group(9100 + m, 7 - i, m, trail="none", also=(T - 1, T, 2 * T - 1, 2 * T))], pre_edge)

    # kept insertion blocks at the first position of the second tile, at position 0 and at a tile's last position
    def pre_ins(at):
        def pre(ds):
            d = ds[0]
            kept = set(d["prof"]["kept"].tolist())
            assert d["m"] == T + 60 and all(p in kept and (d["lay"][p] & 0x7fff) == 2 for p in at), (at, sorted(kept))
            assert d["prof"]["widest"][0] == (2 if 0 in at else 0)
        return pre
    for name, at in (("second_tile", (T,)), ("pos0", (0,)), ("tile_last", (T - 1,)), ("all", (0, T - 1, T))):
        add("ins_" + name, lambda at=at: [ins_group(9200 + len(at) + at[0], 6, T + 60, at)], pre_ins(at))

    # rows against tiles: all gaps over a whole tile, first / last base at a tile's first / last position
    def pre_rows(ds):
        d = ds[0]
        assert d["R"] == 11 and d["m"] == 3 * T and not (d["full"] & 0x20)[d["full"] != GAP].any()
        assert [SC.lead_gap_positions(d["full"], r) for r in (1, 3, 4)] == [T + 40, T, T - 1]
        assert [SC.trail_gap_positions(d["full"], r) for r in (2, 5, 6)] == [T + 40, 2 * T, 2 * T - 1]
        assert row_ranges(d, 1, T)[0] == 0 and row_ranges(d, 2, T)[2:] == [0, 0] and row_ranges(d, 5, T) == [T, 0, 0, 0]
        assert row_ranges(d, 6, T) == [T, 1, 0, 0] and row_ranges(d, 3, T)[:2] == [0, T] and row_ranges(d, 4, T)[:2] == [1, T]
    add("rows_tiles", lambda: [cut_group(9300, 3 * T, [(T + 40, 3 * T), (0, 2 * T - 40), (T, 3 * T), (T - 1, 3 * T), (0, T), (0, T + 1)], 4)], pre_rows)

    # the window slot: a range of SLOT - 1, SLOT and SLOT + 1 bytes beside ordinary rows
    for dd in (-1, 0, 1):
        def pre_slot(ds, dd=dd):
            d = ds[0]
            assert d["R"] == 6 and d["m"] == T + 100
            assert row_ranges(d, 2, T)[0] == SLOT + dd and all(max(row_ranges(d, r, T)) < SLOT - 100 for r in (0, 1, 3, 4, 5))
        add("slot_%+d" % dd, lambda dd=dd: [slot_group(9400 + dd, T, SLOT, dd)], pre_slot)

    # tiles that keep no column / exactly one
    def pre_hole(ds):
        assert ds[0]["R"] == 5 and ds[0]["m"] == 3 * T - 1 and tile_widths(ds[0], T) == [T - 8, 0, 1], tile_widths(ds[0], T)
    add("keep_none_one", lambda: [hole_group(9500, T)], pre_hole)

    # output rows at every residue mod 16, 1 .. 33 kept columns
    def pre_width(ds):
        assert [(d["R"], d["C"], d["m"]) for d in ds] == [(17, C, C) for C in range(1, 34)]
    add("widths", lambda: width_groups(9600), pre_width)

    # row counts around the rows of a trip and of all slices; 129 rows over three tiles
    # (and around the 64 rows whose windows a wavefront looks up at a time)
    for R in sorted(x for x in {1, 2, ROWS - 1, ROWS, ROWS + 1, ROWS * Z - 1, ROWS * Z, ROWS * Z + 1, 64 * ROWS * Z, 64 * ROWS * Z + 1} if x >= 1):
        def pre_R(ds, R=R):
            assert ds[0]["R"] == R and ds[0]["m"] == T + 50
        add("rows_R%d" % R, lambda R=R: [SC.rows_group(9700 + R, R, T + 50, n_pos=12, also=(T,))], pre_R)

    def pre_129(ds):
        assert ds[0]["R"] == 129 and ds[0]["m"] == 2 * T + 1 and len(tile_widths(ds[0], T)) == 3
    add("rows_R129", lambda: [SC.rows_group(9729, 129, 2 * T + 1, trail="pivot", also=(T - 1, T, 2 * T))], pre_129)

    # front pads whose first real base lies in the second tile
    def pre_pads(ds):
        d = ds[0]
        assert d["R"] == 8 and d["m"] == 2 * T + 100 and not (d["full"] & 0x20)[d["full"] != GAP].any()
        assert [SC.lead_gap_positions(d["full"], r) for r in (1, 2, 3)] == [T + 10] * 3
    add("pads", lambda: [pad_group(9800, T)], pre_pads)
    return B


_CACHE = {}


def case(limits, label):
    """(groups, [derive(twin's alignment)]) of a case, computed once per limits and left unchanged; the precondition is asserted"""
    key = (tuple(limits), label)
    if key not in _CACHE:
        build, pre = builders(*limits)[label]
        gs = build()
        ds = [derive(SC.twin_full(g)) for g in gs]
        for d, g in zip(ds, gs):
            assert d["R"] == len(g), (label, "the twin dropped a row", d["R"], len(g))
        pre(ds)
        _CACHE[key] = (gs, ds)
    return _CACHE[key]


def labels(limits):
    return list(builders(*limits))
