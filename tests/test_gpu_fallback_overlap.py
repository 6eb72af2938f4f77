"""The star alignment with its fall-back alignment BESIDE the pad fix and the layout of the candidates the fall-back does not touch
(hite_amd/csrc/hite_msa.hip star_msa_launch, hite_align_begin / hite_align_finish; the switch Context.fallback_overlap) against the
serial route and against the twin (oracle/hite_oracle_msa.c).

Every comparison runs ctx.star_msa(groups, sparse=True, info=True) and once more with sparse=False, with the switch at 1 and at 0,
under the three kernel mixes of align_check.LANE_MODES, and asserts: alignments and info of the two routes equal byte for byte, the
counters of hite_align_stats equal one by one, both equal to the twin's star alignment (the sparse form: under the twin's column
selection).  align_check.check_groups then repeats the twin comparison row by row (info, kept rows, counters) with the switch on.
The inputs are the pairs of tests/align_limit_cases.py; which of them reach the fall-back is asserted on the twin's classes."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import align_limit_cases as AC  # noqa: E402
import oracle_lib as O  # noqa: E402
from align_check import LANE_MODES, check_groups, twin, twin_class, twin_star  # noqa: E402

pytestmark = pytest.mark.gpu

CAP = 8


@pytest.fixture(scope="module")
def ctx():
    import hite_amd

    c = hite_amd.Context(0)
    yield c
    c.close()


def layout_stage(sparse, groups):
    if not sparse:
        return "star_layout_kernel"
    return "star_layout_sparse_kernel_long" if max(len(w) for g in groups for w in g) > 1000 else "star_layout_sparse_kernel_short"


def run_once(ctx, groups, cap, lanes, sparse, mode):
    """-> (alignments, info, counters, profile) of one call with the switch at `mode`"""
    ctx.fallback_overlap(mode)
    ctx.align_lanes(lanes)
    ctx.align_config(cap)
    try:
        ctx.align_stats(reset=True)
        ctx.profile(on=True, reset=True)
        got, info = ctx.star_msa([[bytes(w) for w in g] for g in groups], sparse=sparse, info=True)
        prof = ctx.profile(on=False)
        return got, info, ctx.align_stats(), prof
    finally:
        ctx.fallback_overlap(None)
        ctx.align_lanes(-1)
        ctx.align_config(8)


def expected(groups, cap, sparse):
    out = []
    for g in groups:
        exp, _ = twin_star(g, cap)
        if sparse:
            exp = np.ascontiguousarray(exp[:, O.sparse_cols(exp).astype(bool)])
        out.append(exp)
    return out


def same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and a.shape == b.shape and np.array_equal(a, b))


def both_routes(ctx, groups, cap, fallback_rows):
    """the comparison of the module's docstring; fallback_rows = rows of the call the twin sends to the fall-back (0: the call must
    not fork: no stage align_fallback and ONE launch of the layout on either route; else the overlap route launches the layout twice)"""
    n_fb = sum((twin(g[0], w, cap)[1]["nw"] & 0x100) != 0 for g in groups for w in g[1:])
    assert n_fb == fallback_rows
    for lanes in LANE_MODES:
        infos = []
        for sparse in (True, False):
            on, off = run_once(ctx, groups, cap, lanes, sparse, 1), run_once(ctx, groups, cap, lanes, sparse, 0)
            exp = expected(groups, cap, sparse)
            what = "lanes %d, sparse %d" % (lanes, sparse)
            assert len(on[0]) == len(off[0]) == len(groups), what
            for i, (a, b, e) in enumerate(zip(on[0], off[0], exp)):
                assert same(a, b), (what, "group %d: the routes differ" % i)
                assert same(a, e), (what, "group %d: not the twin's alignment" % i)
            for i, (a, b) in enumerate(zip(on[1], off[1])):
                assert a.tobytes() == b.tobytes(), (what, "group %d: info differs" % i)
            assert on[2] == off[2], (what, on[2], off[2])
            assert on[2]["fallback"] == fallback_rows, (what, on[2])
            stage = layout_stage(sparse, groups)
            assert ("align_fallback" in on[3]) == ("align_fallback" in off[3]) == (fallback_rows > 0), (what, on[3], off[3])
            assert off[3][stage][1] == 1 and on[3][stage][1] == (2 if fallback_rows else 1), (what, on[3], off[3])
            if fallback_rows:
                assert on[3]["align_fallback"][1] == off[3]["align_fallback"][1] == 1
            infos.append(on[1])
        for a, b in zip(*infos):
            assert a.tobytes() == b.tobytes(), "info of the sparse and the plain form differ"
    ctx.fallback_overlap(1)
    try:
        return check_groups(ctx, groups, cap)
    finally:
        ctx.fallback_overlap(None)


def fb_case(name):
    c = [c for c in AC.class_c() if c.name == name][0]
    assert c.cls[CAP][0] == AC.FB and c.cls[CAP][1] == 0
    return c


def clean_group(seed, rows):
    a = AC.rnd(1000 + seed, 200 + 13 * (seed % 17))
    return [a] + [AC.subs(a, 3 + 2 * r + seed % 5) for r in range(rows)]


def test_fallback_rows_among_clean_groups(ctx):
    """70 groups in one call: fall-back rows in group 0, in the middle (two rows of one candidate: one entry of the pending list) and
    in the last group; a group that is not pending drops a row before the fall-back; the others are clean"""
    n = 70
    groups = [clean_group(i, 2 + i % 2) for i in range(n)]
    c = fb_case("C_m60_long_row")
    groups[0] = [c.a, AC.subs(c.a, 2), c.b]
    c = fb_case("C_m900_long_row")
    second = AC.insert(AC.subs(c.a, 5), 450, 9, 45)
    groups[n // 2] = [c.a, c.b, AC.subs(c.a, 40), second]
    c = fb_case("C_m63_long_row")
    groups[n - 1] = [c.a, c.b, AC.subs(c.a, 1)]
    short = groups[20][0]
    groups[20] = groups[20] + [short[:len(short) // 4]]
    classes = both_routes(ctx, groups, CAP, 4)
    fb_groups = [i for i, cl in enumerate(classes) if any(k[0] == AC.FB for k in cl)]
    assert fb_groups == [0, n // 2, n - 1]
    assert [k[0] for k in classes[n // 2]].count(AC.FB) == 2
    assert classes[20][-1] == (4, 2, 0)                                   # dropped by a forward kernel, in a candidate that is not pending
    assert sum(k[1] != 0 for cl in classes for k in cl) == 1


def test_one_centre_many_fates(ctx):
    """a pending candidate with a row dropped BY the fall-back and rows dropped before it, beside one that loses nothing; each alone"""
    groups, exp_classes = AC.one_centre_many_fates()
    n_fb = [sum(k[0] == AC.FB for k in cl) for cl in exp_classes]
    assert n_fb == [3, 1] and (AC.FB, 1, 0) in exp_classes[0] and (4, 2, 0) in exp_classes[0]
    got = both_routes(ctx, groups, AC.F_CAP, sum(n_fb))
    assert [list(g) for g in got] == [list(c) for c in exp_classes]
    for g, cl, k in zip(groups, exp_classes, n_fb):
        assert both_routes(ctx, [g], AC.F_CAP, k) == (tuple(cl),)


def test_no_fallback_pair(ctx):
    """nothing forks: the stage align_fallback is absent and the layout runs once, as on the serial route"""
    groups = [clean_group(100 + i, 2 + i % 3) for i in range(12)]
    short = groups[5][0]
    groups[5] = groups[5] + [short[:len(short) // 4]]       # a dropped row, and still no fork
    classes = both_routes(ctx, groups, CAP, 0)
    assert classes[5][-1] == (4, 2, 0)


def test_every_group_pending(ctx):
    """the window has nothing to do: every candidate waits for the fall-back; a single pending group; a lone centre beside one"""
    names = ("C_m60_long_row", "C_m63_long_row", "C_m900_long_row", "C_m945_long_centre", "C_k0_long_row")
    cases = [fb_case(x) for x in names]
    groups = [[c.a, c.b] for c in cases]
    classes = both_routes(ctx, groups, CAP, len(groups))
    assert all(cl == ((AC.FB, 0, 1),) for cl in classes)
    assert both_routes(ctx, groups[2:3], CAP, 1) == (((AC.FB, 0, 1),),)
    assert both_routes(ctx, [[cases[0].a], groups[2]], CAP, 1) == ((), ((AC.FB, 0, 1),))
    assert both_routes(ctx, [groups[2], [cases[0].a]], CAP, 1) == (((AC.FB, 0, 1),), ())


# ---- the fine stage end to end ---------------------------------------------------------------------------------------------------
def _family(rng, L, copies, gap_copy):
    """a TIR family: `copies` copies of a consensus of L bases (2 % substitutions), copy `gap_copy` with 45 random bases in its middle"""
    import casegen

    tir = "CA" + casegen.rand_seq(rng, 12)
    cons = tir + casegen.rand_seq(rng, L - 28) + casegen.revcomp(tir)
    out = []
    for k in range(copies):
        s = casegen.mutate(rng, cons, 0.02 if k else 0.0)
        if k == gap_copy:
            s = s[:L // 2] + casegen.rand_seq(rng, 45) + s[L // 2:]
        out.append(s)
    return out


def _genome(seed):
    """one contig of ~36 kb with two families: 700 bases (whole windows in the only pass) and 1 500 bases (truncated windows first,
    whole windows in the second pass), each with one copy that carries a 45-base insertion -- a row for the fall-back"""
    import casegen

    rng = np.random.default_rng(seed)
    parts, cands, copies, pos = [], [], [], 0
    for L, ncopy in ((700, 6), (1500, 8)):
        fam, cp = _family(rng, L, ncopy, 2), []
        for s in fam:
            tsd = casegen.rand_seq(rng, 8)
            spacer = casegen.rand_seq(rng, 1200)
            parts += [spacer, tsd, s, tsd]
            pos += len(spacer) + len(tsd)
            cp.append((0, pos + 1, pos + len(s), 0))
            pos += len(s) + len(tsd)
        cands.append(fam[0])
        copies.append(cp)
    parts.append(casegen.rand_seq(rng, 1200))
    return "".join(parts), cands, copies


def test_fine_stage_end_to_end(ctx):
    """flank_region_align on a small genome whose whole-window passes hold fall-back rows: calls and consensus bytes of the two
    routes are equal, and the serial route alone already shows the fall-back"""
    contig, cands, copies = _genome(17)
    assert 20_000 < len(contig) < 60_000
    ctx.genome_pack([contig])
    res = []
    for mode in (0, 1):
        ctx.fallback_overlap(mode)
        try:
            ctx.align_stats(reset=True)
            calls, _ = ctx.flank_region_align("tir", cands, copies, plant=1)
            st = ctx.align_stats()
        finally:
            ctx.fallback_overlap(None)
        assert st["fallback"] > 0, (mode, st)
        res.append((calls, st))
    assert res[0][1] == res[1][1], (res[0][1], res[1][1])
    assert len(res[0][0]) == len(res[1][0]) == len(cands)
    for a, b in zip(res[0][0], res[1][0]):
        assert tuple(a) == tuple(b), (a, b)
