"""The checker of the pairwise aligner's GPU tests (test_gpu_align.py, test_gpu_align_limits.py): HIP against the twin
(oracle/hite_oracle_msa.c) and the band-free definition (oracle/hite_oracle_nw.c) through the C ABI.  The CPU side of a pair -- the
twin's run at a cap, the definition's ops and cost, the matrices of both -- is computed once per process and shared by every run
that meets the pair again (three kernel mixes, four caps, lists that are prefixes of one another)."""
from typing import NamedTuple

import numpy as np

import oracle_lib as O

FALLBACK = 64 | 0x100          # band words of a pair kept from the 64-word fall-back, as the info reports them
LANE_MODES = (-2, 0, 400)      # thread-per-pair kernels alone; every pair in the lane-parallel kernels; the two side by side


class Checked(NamedTuple):
    n_cert: int
    n_opt: int
    n_drop: int
    classes: tuple       # per pair: (band words of the run kept, status, certified)


def pair_matrix(a, b, ops):
    """2 x cols alignment from the ops of one pair (insertion blocks left-justified, as the star layout does)"""
    rows = ([], [])
    nxt = 0
    for p in range(len(a)):
        q, gap = int(ops[p]) & 0x7FFF, int(ops[p]) >> 15
        for x in range(nxt, q):
            rows[0].append(ord("-"))
            rows[1].append(b[x])
        rows[0].append(a[p])
        if gap:
            rows[1].append(ord("-"))
            nxt = q
        else:
            rows[1].append(b[q])
            nxt = q + 1
    for x in range(nxt, len(b)):
        rows[0].append(ord("-"))
        rows[1].append(b[x])
    return np.array(rows, dtype=np.uint8)


def matrix_cost(m):
    """cost of a 2-row alignment under the definition: gap 3, mismatch 1, a byte outside ACGT matches nothing, a row byte in lower
    case is its base"""
    row = np.where((m[1] >= ord("a")) & (m[1] <= ord("z")), m[1] & 0xDF, m[1])
    gap = (m[0] == ord("-")) | (m[1] == ord("-"))
    return 3 * int(gap.sum()) + int(((m[0] != row) & ~gap).sum()) + int(((m[0] == row) & ~np.isin(m[0], list(b"ACGT"))).sum())


_twin, _nwd, _nwp = {}, {}, {}


def _key(a, b):
    return bytes(a), bytes(b)


def twin(a, b, cap):
    """(ops or None, info, matrix or None) of the twin's schedule at exact_cap = cap"""
    k = _key(a, b) + (cap,)
    if k not in _twin:
        ops, ti = O.align_pair(a, b, cap)
        _twin[k] = (ops, ti, None if ops is None else pair_matrix(a, b, ops))
    return _twin[k]


def nw_distance(a, b):
    k = _key(a, b)
    if k not in _nwd:
        _nwd[k] = O.nw_distance(a, b)
    return _nwd[k]


def nw_pair(a, b):
    """(cost, matrix) of the definition's canonical alignment"""
    k = _key(a, b)
    if k not in _nwp:
        nops, nd = O.nw_pair(a, b)
        _nwp[k] = (nd, pair_matrix(a, b, nops))
    return _nwp[k]


def twin_class(ti):
    return ti["nw"], ti["status"], ti["cert"] if ti["status"] == 0 else 0


def expected_stats(results):
    """the counters of hite_align_stats from the twin's per-pair results: results = [(info of the twin, columns of the row)]"""
    return {"pairs": len(results),
            "certified": sum(ti["status"] == 0 and ti["cert"] == 1 for ti, _ in results),
            "wide": sum(ti["status"] == 0 and (ti["nw"] & 0xFF) > 4 for ti, _ in results),
            "fallback": sum((ti["nw"] & 0x100) != 0 for ti, _ in results),
            "dropped": sum(ti["status"] != 0 for ti, _ in results),
            "cost": sum(ti["U"] for ti, _ in results if ti["status"] == 0),
            "columns": sum(n for _, n in results)}


def assert_stats(ctx, results, cap):
    st = ctx.align_stats()
    exp = expected_stats(results)
    exp["exact_cap"] = cap
    assert st == exp, (st, exp)


def assert_info(inf, ti):
    """one row of the info table == the twin: cost, certificate, status, k*, band words"""
    U, cert, status, kst, nw = (int(x) for x in inf)
    assert (U, cert, status, kst, nw) == (ti["U"], ti["cert"] if ti["status"] != 2 else 0, ti["status"], ti["kstar"], ti["nw"]), (inf, ti)


def check_pairs(ctx, pairs, cap, no_nw_pair=()):
    """pairs: list of (a, b) uint8 arrays; runs them as two-row groups with exact_cap = cap -- three times: through the
    thread-per-pair kernels alone, with EVERY pair in the lane-parallel kernels (hite_align_lanes; 4 / 8 lanes per pair in the
    forward passes, a wavefront per pair in the traceback), and with the two kinds side by side"""
    res = []
    for lanes in LANE_MODES:
        ctx.align_lanes(lanes)
        try:
            res.append(check_pairs_once(ctx, pairs, cap, no_nw_pair))
        finally:
            ctx.align_lanes(-1)
    assert res[0] == res[1] == res[2]
    return res[0]


def check_pairs_once(ctx, pairs, cap, no_nw_pair=()):
    """no_nw_pair: indices of the pairs whose full matrix is too large for the definition's traceback (only the cost bound then)"""
    ctx.align_config(cap)
    prev = O.set_align_exact(cap)
    try:
        groups = [[bytes(a), bytes(b)] for a, b in pairs]
        ctx.align_stats(reset=True)
        got, info = ctx.star_msa(groups, info=True)
        n_cert = n_opt = n_drop = 0
        classes, results = [], []
        for i, ((a, b), m, inf) in enumerate(zip(pairs, got, info)):
            ops, ti, exp = twin(a, b, cap)
            assert_info(inf[1], ti)
            U, cert = int(inf[1][0]), int(inf[1][1])
            results.append((ti, len(b)))
            classes.append(twin_class(ti))
            if ops is None:
                n_drop += 1
                assert m is not None and m.shape[0] == 1 and bytes(m[0]) == bytes(a)
                continue
            assert m is not None and m.shape == exp.shape and np.array_equal(m, exp)
            assert matrix_cost(m) == U
            d = nw_distance(a, b)
            assert U >= d
            n_opt += U == d
            if cert:
                n_cert += 1
                if i in no_nw_pair:
                    assert U == d
                else:
                    nd, nm = nw_pair(a, b)
                    assert U == nd and np.array_equal(m, nm)
        assert_stats(ctx, results, cap)
        return Checked(n_cert, n_opt, n_drop, tuple(classes))
    finally:
        O.set_align_exact(prev)
        ctx.align_config(8)


_star = {}


def twin_star(wins, cap):
    k = tuple(bytes(w) for w in wins) + (cap,)
    if k not in _star:
        prev = O.set_align_exact(cap)
        try:
            _star[k] = O.star_msa(wins, rows=True)
        finally:
            O.set_align_exact(prev)
    return _star[k]


def check_groups(ctx, groups, cap):
    """groups of many rows around one centre, in ONE call, through the three kernel mixes: every row's info == the twin's, every
    group's alignment == the twin's star alignment (dropped rows absent), the counters == the sums over the twin's rows.
    -> per group the classes of its rows"""
    res = []
    for lanes in LANE_MODES:
        ctx.align_lanes(lanes)
        ctx.align_config(cap)
        try:
            ctx.align_stats(reset=True)
            got, info = ctx.star_msa([[bytes(w) for w in g] for g in groups], info=True)
            classes, results = [], []
            for g, m, inf in zip(groups, got, info):
                assert not inf[0].any()
                rows = [twin(g[0], w, cap) for w in g[1:]]
                for (ops, ti, _), w, x in zip(rows, g[1:], inf[1:]):
                    assert_info(x, ti)
                    results.append((ti, len(w)))
                classes.append(tuple(twin_class(ti) for _, ti, _ in rows))
                exp, kept = twin_star(g, cap)
                assert kept == 1 + sum(ops is not None for ops, _, _ in rows)
                assert m is not None and m.shape == exp.shape and np.array_equal(m, exp)
            assert_stats(ctx, results, cap)
            res.append(tuple(classes))
        finally:
            ctx.align_lanes(-1)
            ctx.align_config(8)
    assert res[0] == res[1] == res[2]
    return res[0]
