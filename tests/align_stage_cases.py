"""Inputs of tests/test_gpu_align_stages.py, and the profiler stages that one call of the star alignment must begin, worked out from
the twin's results alone (checked on the CPU by tests/test_align_stage_cases.py).

The route of hite_align_begin (hite_amd/csrc/hite_align.hip), restated:
  * align_prep once; the 4-word forward pass over every row: with the lane-parallel kernels off (lanes -2) one stage align_fwd4<tag>,
    with every pair in them (lanes 0) one stage align_fwd4_lanes<tag> and no thread-per-pair launch at all;
  * a pair ESCALATES at exact_cap = cap when its 4-word run ended with status 0, without a certificate, and with a cost U4 that a
    band of `cap` words may still hold: U4 + 3 * 48 <= 96 * cap (align_flag_kernel, what == 2);
  * cap 8: one stage align_fwd_wide<tag> around the level loop, whether or not a pair escalates; inside it, with lanes 0, one stage
    align_fwd_wide_lanes<tag> per level that has pairs -- cap 8 has the one level 8, which has pairs when any pair escalates;
  * cap >= 16 and a pair escalates: the traceback of the rows that are FINAL after the 4-word run (align_tb<tag>, when there is such
    a row), beside it the wider levels as one stage align_fwd_wide<tag>, then the traceback of the escalated rows (align_tb<tag>
    again); no lane-parallel traceback.  FINAL (align_flag_kernel, what == 3) is every row with strips > 0 -- every non-empty row
    that is not a centre -- that does not escalate: the rows the 4-word run dropped or sent to the fall-back are among them;
  * every other call: one traceback over every row, align_tb<tag> with lanes -2, align_tb_strips<tag> with lanes 0;
  * align_fallback once when a row goes to the 64-word fall-back, on either setting of Context.fallback_overlap.
<tag> is "_long" when a window of the call has more than 1000 bytes, else "_short" (hite_msa.hip, star_msa_launch)."""
import align_limit_cases as AC
from align_check import twin, twin_class

CAPS = (0, 8, 16, 32)
LANES = (-2, 0)


def clean_group(seed, rows):
    a = AC.rnd(1000 + seed, 200 + 13 * (seed % 17))
    return [a] + [AC.subs(a, 3 + 2 * r + seed % 5) for r in range(rows)]


def clean_groups():
    """the 12 groups of test_gpu_fallback_overlap.py::test_no_fallback_pair: certified at once, and one row dropped as too short"""
    groups = [clean_group(100 + i, 2 + i % 3) for i in range(12)]
    short = groups[5][0]
    groups[5] = groups[5] + [short[:len(short) // 4]]
    return groups


def grain_pairs():
    return [[c.a, c.b] for c in AC.grains_16()[:1] + AC.grains_8()[:1] + AC.grains_32()[:1]]


INPUTS = {"clean": clean_groups, "fates": lambda: AC.one_centre_many_fates()[0], "grains": grain_pairs}
_inputs = {}


def groups_of(name):
    if name not in _inputs:
        _inputs[name] = INPUTS[name]()
    return _inputs[name]


def tag_of(groups):
    return "_long" if max(len(w) for g in groups for w in g) > 1000 else "_short"


def route(groups, cap):
    """-> (rows that escalate, rows that are final after the 4-word run, rows of the fall-back) of one call, by the twin"""
    n_esc = n_fin = n_fb = 0
    for g in groups:
        for w in g[1:]:
            assert len(w) > 0
            t4 = twin(g[0], w, 0)[1]                   # cap 0: the 4-word run is the only one, its result is what the info reports
            esc = twin_class(t4) == (4, 0, 0) and t4["U"] + 3 * 48 <= 96 * cap
            n_esc += esc
            n_fin += not esc
            n_fb += (twin(g[0], w, cap)[1]["nw"] & 0x100) != 0
    return n_esc, n_fin, n_fb


def expected_stages(groups, cap, lanes):
    """{stage: times begun} of the stages align_* of one ctx.star_msa(groups) at exact_cap = cap with Context.align_lanes(lanes)"""
    assert cap in CAPS and lanes in LANES
    tag = tag_of(groups)
    n_esc, n_fin, n_fb = route(groups, cap)
    t = {"align_prep": 1, ("align_fwd4" if lanes == -2 else "align_fwd4_lanes") + tag: 1}
    if cap == 8:
        t["align_fwd_wide" + tag] = 1
        if lanes == 0 and n_esc:
            t["align_fwd_wide_lanes" + tag] = 1
    if cap >= 16 and n_esc:
        t["align_fwd_wide" + tag] = 1
        t["align_tb" + tag] = 2 if n_fin else 1
    else:
        t[("align_tb" if lanes == -2 else "align_tb_strips") + tag] = 1
    if n_fb:
        t["align_fallback"] = 1
    return t
