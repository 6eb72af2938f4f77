"""The inputs of tests/test_gpu_align_stages.py by the twin alone (no GPU): every input takes, at every cap, the route that the table
of tests/align_stage_cases.py is there to pin -- a call where nothing escalates and nothing falls back, one with escalated, final,
dropped and fall-back rows side by side, and one whose rows escalate one cap after the other until no row is final."""
import pytest

import align_limit_cases as AC
import align_stage_cases as SC
from align_check import twin, twin_class

# (input, cap) -> (rows that escalate, rows final after the 4-word run, rows of the fall-back), from how the inputs are made:
#   clean:  37 rows with 3 .. 12 substitutions in 200 .. 420 columns: certified by the 4-word run (k* = 365); the quarter row is infeasible
#   fates:  16 rows.  A row of k substitutions has U4 = k, and is certified up to k* = 365: in group 0 the rows of 500, 1000 and 1450
#           substitutions and the two drifted rows (U4 = 530 and 1256) escalate where 96 cap - 144 reaches their U4 -- 500 and 530 at
#           cap 8, 1000 and 1256 at cap 16, 1450 at cap 32 -- and subs(A, 3000) never; group 1 adds subs(B, 400) and subs(B, 366)[:-1]
#           (U4 = 369) from cap 8 on.  The rows with an insertion of 45 or 1 100 bases and the half row A[:2300] leave the 4-word
#           slice (status 1): four rows of the fall-back at every cap
#   grains: U4 = 700 (ends at 16 words), 380 (8 words), about 1 690 (32 words): one more row escalates with every cap
ROUTES = {("clean", 0): (0, 37, 0), ("clean", 8): (0, 37, 0), ("clean", 16): (0, 37, 0), ("clean", 32): (0, 37, 0),
          ("fates", 0): (0, 16, 4), ("fates", 8): (4, 12, 4), ("fates", 16): (6, 10, 4), ("fates", 32): (7, 9, 4),
          ("grains", 0): (0, 3, 0), ("grains", 8): (1, 2, 0), ("grains", 16): (2, 1, 0), ("grains", 32): (3, 0, 0)}
U4 = {"fates": [[100, 500, 1000, 1450, None, None, None, 530, 1256, None, None, 2996], [30, 400, None, 369]]}


@pytest.mark.parametrize("name", list(SC.INPUTS))
def test_every_input_takes_its_route(name):
    groups = SC.groups_of(name)
    for cap in SC.CAPS:
        assert SC.route(groups, cap) == ROUTES[(name, cap)], (name, cap)


def test_the_classes_behind_the_routes():
    clean = SC.groups_of("clean")
    assert len(clean) == 12 and sum(len(g) - 1 for g in clean) == 37
    for cap in SC.CAPS:
        cls = [twin_class(twin(g[0], w, cap)[1]) for g in clean for w in g[1:]]
        assert sorted(set(cls)) == [(4, 0, 1), (4, 2, 0)] and cls.count((4, 2, 0)) == 1
    fates, classes = AC.one_centre_many_fates()
    for g, cl in zip(fates, classes):
        assert tuple(twin_class(twin(g[0], w, AC.F_CAP)[1]) for w in g[1:]) == tuple(cl)
    for g, us in zip(fates, U4["fates"]):           # None: the 4-word run is not kept (dropped, or left to the fall-back)
        t4 = [twin(g[0], w, 0)[1] for w in g[1:]]
        assert [t["U"] if t["nw"] == 4 and t["status"] == 0 else None for t in t4] == us
    grains = SC.groups_of("grains")
    assert [twin_class(twin(g[0], g[1], 32)[1]) for g in grains] == [(16, 0, 1), (8, 0, 1), (32, 0, 1)]
    assert [twin_class(twin(g[0], g[1], 0)[1]) for g in grains] == [(4, 0, 0)] * 3


def test_the_tags():
    """the stage names carry _short only for the clean groups: the other two inputs hold windows of more than 1000 bytes"""
    assert {n: SC.tag_of(SC.groups_of(n)) for n in SC.INPUTS} == {"clean": "_short", "fates": "_long", "grains": "_long"}
    assert max(len(w) for g in SC.groups_of("clean") for w in g) <= 1000


def test_the_tables():
    """the cells of the table that differ between the inputs, spelled out once"""
    e = SC.expected_stages
    assert e(SC.groups_of("clean"), 8, -2) == {"align_prep": 1, "align_fwd4_short": 1, "align_fwd_wide_short": 1, "align_tb_short": 1}
    assert e(SC.groups_of("clean"), 32, 0) == {"align_prep": 1, "align_fwd4_lanes_short": 1, "align_tb_strips_short": 1}
    assert e(SC.groups_of("fates"), 8, 0) == {"align_prep": 1, "align_fwd4_lanes_long": 1, "align_fwd_wide_long": 1, "align_fwd_wide_lanes_long": 1,
                                              "align_tb_strips_long": 1, "align_fallback": 1}
    assert e(SC.groups_of("fates"), 16, 0) == {"align_prep": 1, "align_fwd4_lanes_long": 1, "align_fwd_wide_long": 1, "align_tb_long": 2, "align_fallback": 1}
    assert e(SC.groups_of("grains"), 16, -2) == {"align_prep": 1, "align_fwd4_long": 1, "align_fwd_wide_long": 1, "align_tb_long": 2}
    assert e(SC.groups_of("grains"), 32, -2) == {"align_prep": 1, "align_fwd4_long": 1, "align_fwd_wide_long": 1, "align_tb_long": 1}
    assert e(SC.groups_of("grains"), 0, 0) == {"align_prep": 1, "align_fwd4_lanes_long": 1, "align_tb_strips_long": 1}
