"""The cases of the pairwise aligner's limit tests (tests/align_limit_cases.py), checked on the CPU alone: every pair lands in the class
it is named for -- by the twin's schedule (O.align_pair), by the same schedule restated here from single runs of the banded aligner
(O.bp_pair), and against the band-free definition (O.nw_pair) -- and the classes that the GPU test (test_gpu_align_limits.py) exists
for are all there, often enough and in both orientations.  Without this the GPU test could pass on pairs that never leave the
4-word band.

No pair but the two at the window limit of 32 767 columns is excused from the comparison with the definition's canonical alignment.

No sub-class that was searched for with the twin is missing: pairs kept uncertified from 16 words at cap 16, which run 16 and then 32
words at cap 32, exist within a centre of 4 000 columns (B_s8_k900 and its kin)."""
import numpy as np
import pytest

import align_limit_cases as AC
import oracle_lib as O
from align_check import FALLBACK, twin_class

assert FALLBACK == AC.FB

GROUPS = {"A": AC.class_a, "B": AC.class_b, "C": AC.class_c, "D": AC.class_d, "D_window_limit": AC.class_d_window_limit,
          "E8": AC.grains_8, "E16": AC.grains_16, "E32": AC.grains_32, "E_mixed": AC.mixed_wave}
_cases, _bp, _nw = {}, {}, {}


def cases(group):
    if group not in _cases:
        _cases[group] = GROUPS[group]()
    return _cases[group]


def bp(c, nw, full=False):
    k = (c.name, nw, full)
    if k not in _bp:
        _bp[k] = O.bp_pair(c.a, c.b, nw, full)[1]
    return _bp[k]


def definition(c):
    if c.name not in _nw:
        _nw[c.name] = O.nw_pair(c.a, c.b)
    return _nw[c.name]


def replay(c, cap):
    """orc_align_pair's schedule from single runs: -> [(band words, result)] of the runs before any fall-back, and the class"""
    runs = [(4, bp(c, 4))]
    r = runs[0][1]
    if r["status"] == 2:
        return runs, (4, 2, 0)
    if cap >= 8 and not r["cert"] and r["U"] + 3 * 48 <= 96 * cap:
        lvl = 8
        while 96 * lvl < r["U"] + 3 * 48:
            lvl *= 2
        while lvl <= cap:
            r = bp(c, lvl)
            runs.append((lvl, r))
            if r["cert"]:
                break
            lvl *= 2
    lvl, r = runs[-1]
    if r["status"] == 1:
        lvl, r = AC.FB, bp(c, 64, True)
    return runs, (lvl, r["status"], r["cert"] if r["status"] == 0 else 0)


def test_the_certificate_bounds_the_classes_are_named_by():
    """k* of an equal-length pair whose band follows the main diagonal, whatever the length; the level thresholds 96 level - 144"""
    for L in (1200, 4200, 9000):
        a = AC.rnd(5, L)
        b = AC.subs(a, 300)
        assert {nw: O.bp_pair(a, b, nw)[1]["kstar"] for nw in (4, 8, 16, 32)} == AC.KSTAR
    assert AC.LEVEL_MAX_U == {lvl: 96 * lvl - 3 * 48 for lvl in (8, 16, 32)}
    assert AC.class_of_u(365) == {0: (4, 0, 1), 8: (4, 0, 1), 16: (4, 0, 1), 32: (4, 0, 1)}
    assert AC.class_of_u(625) == {0: (4, 0, 0), 8: (4, 0, 0), 16: (16, 0, 1), 32: (16, 0, 1)}
    assert AC.class_of_u(2929) == {0: (4, 0, 0), 8: (4, 0, 0), 16: (4, 0, 0), 32: (4, 0, 0)}


@pytest.mark.parametrize("group", list(GROUPS))
def test_every_case_lands_in_its_class(group):
    names = set()
    for c in cases(group):
        assert c.name not in names
        names.add(c.name)
        assert c.nw_pair or group == "D_window_limit"          # the one omission
        d = O.nw_distance(c.a, c.b) if not c.nw_pair else definition(c)[1]
        for cap, want in c.cls.items():
            ops, ti = O.align_pair(c.a, c.b, cap)
            assert twin_class(ti) == want, (c.name, cap, ti, want)
            if group in ("A", "B", "C"):
                assert replay(c, cap)[1] == want, (c.name, cap)
            if ops is None:
                assert ti["status"] in (1, 2)
                continue
            assert O.ops_cost(c.a, c.b, ops) == ti["U"] >= d, (c.name, cap)
            if c.U is not None:
                assert ti["U"] == c.U == d, (c.name, cap, ti["U"], d)
            if ti["cert"]:
                assert ti["U"] == d, (c.name, cap)
                if c.nw_pair:
                    assert np.array_equal(ops, definition(c)[0]), (c.name, cap)


def test_both_sides_of_every_threshold():
    by = {c.name: c for c in cases("A")}
    assert AC.THRESHOLDS == ((AC.KSTAR[4], AC.KSTAR[4] + 1),) + tuple((u, u + 1) for u in AC.LEVEL_MAX_U.values())
    for lo, hi in AC.THRESHOLDS:
        a, b = by["A_u%d" % lo], by["A_u%d" % hi]
        assert hi - lo == 1 and len(a.a) == len(b.a) == len(a.b) == len(b.b)
        ua, ub = (O.align_pair(c.a, c.b, 32)[1]["U"] for c in (a, b))
        assert (ua, ub) == (lo, hi) == (definition(a)[1], definition(b)[1])
        differ = [cap for cap in AC.CAPS if a.cls[cap] != b.cls[cap]]
        assert differ, (lo, hi)
        for cap in AC.CAPS:          # every cap takes both sides: where the classes agree, the threshold belongs to another cap
            assert a.cls[cap] == AC.class_of_u(lo)[cap] and b.cls[cap] == AC.class_of_u(hi)[cap]
    # which caps tell the sides apart
    tell = {lo: [cap for cap in AC.CAPS if AC.class_of_u(lo)[cap] != AC.class_of_u(hi)[cap]] for lo, hi in AC.THRESHOLDS}
    assert tell == {365: [0, 8, 16, 32], 624: [8, 16, 32], 1392: [16, 32], 2928: [32]}


def test_pairs_escalated_twice():
    by = {c.name: c for c in cases("B")}
    assert sorted(AC.ESCALATED_TWICE) == sorted(n for n, c in by.items() if c.cls[8] == (8, 0, 0) or c.cls[16] == (16, 0, 0))
    for name, (cap, levels) in AC.ESCALATED_TWICE.items():
        runs, cls = replay(by[name], cap)
        assert tuple(lvl for lvl, _ in runs) == (4,) + levels and cls == (levels[1], 0, 1) == by[name].cls[cap]
        assert [r["cert"] for _, r in runs] == [0, 0, 1] and all(r["status"] == 0 for _, r in runs)
        # the drift costs the certificate diagonals, not the path its slice: every level finds the same, optimal, cost
        assert len({r["U"] for _, r in runs}) == 1 and runs[0][1]["U"] == definition(by[name])[1]
        assert runs[1][1]["kstar"] < runs[1][1]["U"] <= runs[2][1]["kstar"]
    assert sum(cap == 16 for cap, _ in AC.ESCALATED_TWICE.values()) >= 2 and sum(cap == 32 for cap, _ in AC.ESCALATED_TWICE.values()) >= 2


def test_fall_back_from_every_level():
    seen = {}
    for c in cases("C"):
        for cap in AC.CAPS:
            runs, cls = replay(c, cap)
            lvl, r = runs[-1]
            assert r["status"] == 1 and lvl == c.fb_from[cap] and cls[0] == AC.FB, (c.name, cap)
            seen.setdefault((cap, lvl), []).append(np.sign(len(c.b) - len(c.a)))
    for lvl in (4, 8, 16, 32):
        assert len(seen[(32, lvl)]) >= 2 and {-1, 1} <= set(seen[(32, lvl)]), lvl          # both orientations
    assert len(seen[(8, 8)]) >= 2 and len(seen[(16, 16)]) >= 2
    small = [c for c in cases("C") if len(c.a) < 1024]
    assert len(small) >= 3 and sum(len(c.a) < 64 for c in small) >= 2


def test_the_fall_backs_own_limit():
    """the longest insertion the 64-word band still aligns, and the next: found with the twin, both orientations"""
    by = {c.name: c for c in cases("C")}
    a = AC.rnd(5, 2500)
    for x in range(AC.FB_LONGEST_ROW - 3, AC.FB_LONGEST_ROW + 4):
        assert O.align_pair(a, AC.insert(a, 1200, 8, x), 8)[1]["status"] == (0 if x <= AC.FB_LONGEST_ROW else 1)
    for x in range(AC.FB_LONGEST_CENTRE - 3, AC.FB_LONGEST_CENTRE + 4):
        assert O.align_pair(AC.insert(a, 1200, 8, x), a, 8)[1]["status"] == (0 if x <= AC.FB_LONGEST_CENTRE else 1)
    for name in ("C_limit_long_row", "C_limit_long_centre"):
        kept, dropped = by[name + "_kept"], by[name + "_dropped"]
        assert abs(len(dropped.a) + len(dropped.b) - len(kept.a) - len(kept.b)) == 1
        assert kept.cls[8][1] == 0 and dropped.cls[8] == (AC.FB, 1, 0)


def test_the_classes_the_gpu_test_exists_for_are_all_there():
    abc = cases("A") + cases("B") + cases("C")
    d = cases("D")

    def orient(pred, cap, among=abc):
        return [int(np.sign(len(c.b) - len(c.a))) for c in among if pred(c.cls[cap])]

    for cap, cls in ((8, (8, 0, 1)), (16, (16, 0, 1)), (32, (32, 0, 1)), (8, (8, 0, 0)), (16, (16, 0, 0))):
        o = orient(lambda x: x == cls, cap)
        assert len(o) >= 2 and {-1, 1} <= set(o), (cap, cls, o)
    o = orient(lambda x: x[0] == AC.FB and x[1] == 1, 32)             # dropped after the fall-back
    assert len(o) >= 2 and {-1, 1} <= set(o)
    o = orient(lambda x: x == (AC.FB, 0, 0), 32)                       # kept from the fall-back without a certificate
    assert len(o) >= 1
    o = orient(lambda x: x[1] == 2, 8, d)                              # infeasible: only a row far shorter than the centre can be
    assert len(o) >= 2 and set(o) == {-1}
    # geometry: every combination of the lengths around a strip, two strips, 32 strips and the 64-strip round, at caps 0 and 8
    names = {c.name for c in d}
    assert {"D_m%d_n%d" % (m, n) for g in AC.EDGES for m in g for n in g} <= names and AC.EDGES[3] == (1023, 1024, 1025)
    by = {c.name: c for c in d}
    assert all(by["D_u380_m%d" % L].cls[8] == (8, 0, 1) and len(by["D_u380_m%d" % L].a) == L for L in (1024, 1025))
    for name in ("D_n_run_in_row", "D_n_run_in_centre", "D_dots", "D_lower_case", "D_all_of_them"):
        c = by[name]
        assert c.cls[8] == (8, 0, 1) and c.cls[0] == (4, 0, 0)
        assert not (c.b[0] & 0x20) and not (c.b[-1] & 0x20)            # the pads are INSIDE: none that the layout would take off again
    assert (by["D_dots"].b == ord(".")).sum() == 10 and ((by["D_lower_case"].b & 0x20) != 0).sum() == 40
    big = cases("D_window_limit")
    assert [(len(c.a), len(c.b)) for c in big] == [(32767, 32767), (32767, 32764)]


def test_the_launch_grains():
    e8, e16, e32 = cases("E8"), cases("E16"), cases("E32")
    assert len(e8) == max(AC.GRAINS_8) == 129 and len(e16) == len(e32) == max(AC.GRAINS_WIDE) == 65
    assert {1, 31, 32, 33, 63, 64, 65, 129} == set(AC.GRAINS_8) and {1, 63, 64, 65} == set(AC.GRAINS_WIDE)
    for lst in (e8, e16, e32):
        n = [len(c.b) for c in lst]
        assert max(n) - min(n) >= 40 and {int(np.sign(len(c.b) - len(c.a))) for c in lst} == {-1, 0, 1}
        for k in (31, 63, len(lst)):                  # every list the test cuts is out of length order: the sort interleaves it
            if k <= len(lst):
                assert sorted(n[:k], reverse=True) != n[:k]
        assert len({(bytes(c.a), bytes(c.b)) for c in lst}) == len(lst)
    mix = cases("E_mixed")
    strips = {(len(c.b) + 15) // 16 for c in mix}
    assert min(strips) == 3 and max(strips) == 188 and AC.tally(mix, 8) == {(8, 0, 1): 3, (4, 0, 1): 6}


def test_one_centre_many_fates():
    groups, classes = AC.one_centre_many_fates()
    for g, cl in zip(groups, classes):
        got = tuple(twin_class(O.align_pair(g[0], w, AC.F_CAP)[1]) for w in g[1:])
        assert got == cl
    c0, c1 = classes
    assert {(4, 0, 1), (8, 0, 1), (16, 0, 1), (32, 0, 1), (4, 0, 0), (AC.FB, 0, 1), (AC.FB, 0, 0), (AC.FB, 1, 0), (4, 2, 0)} == set(c0)
    assert all(st == 0 for _, st, _ in c1)
    prev = O.set_align_exact(AC.F_CAP)
    try:
        m0, kept0 = O.star_msa(groups[0], rows=True)
        m1, kept1 = O.star_msa(groups[1], rows=True)
    finally:
        O.set_align_exact(prev)
    assert kept0 == 1 + sum(st == 0 for _, st, _ in c0) < len(groups[0]) and kept1 == len(groups[1])
    left = [w for w, (_, st, _) in zip(groups[0][1:], c0) if st == 0]
    assert [bytes(r[r != ord("-")]) for r in m0] == [bytes(groups[0][0])] + [bytes(w) for w in left]
