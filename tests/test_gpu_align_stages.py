"""The route of the pairwise aligner's driver (hite_amd/csrc/hite_align.hip, hite_align_begin / hite_align_finish), pinned by the
profiler stages that one call of the star alignment begins: for every exact cap, with the lane-parallel kernels off and with every
pair in them, with the fall-back beside the layout and before it, the whole table {stage: times begun} of the stages align_* equals
the table of tests/align_stage_cases.py, which follows from the twin's results alone (tests/test_align_stage_cases.py checks on the
CPU that the inputs take the routes the table tells apart).

The rows that count as final after the 4-word run -- the ones whose traceback runs beside the wider levels at a cap of 16 or 32 --
are, by align_flag_kernel (what == 3), all rows with strips > 0 that do not escalate: every non-empty row other than a centre whose
4-word run was certified, dropped, left to the fall-back, or too costly for the cap.

The stage names end in _short for a call whose windows all have at most 1000 bytes, else in _long: the clean groups are such a call
(asserted), the other two inputs hold windows of 1 300 to 5 700 bytes."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import align_stage_cases as SC  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import hite_amd

    c = hite_amd.Context(0)
    yield c
    c.close()


def stages_once(ctx, groups, cap, lanes, overlap):
    """{stage: times begun} of the stages align_* of one call (profiling on and reset)"""
    ctx.fallback_overlap(overlap)
    ctx.align_lanes(lanes)
    ctx.align_config(cap)
    try:
        ctx.profile(on=True, reset=True)
        ctx.star_msa([[bytes(w) for w in g] for g in groups], info=True)
        prof = ctx.profile(on=False)
    finally:
        ctx.fallback_overlap(None)
        ctx.align_lanes(-1)
        ctx.align_config(8)
    return {k: v[1] for k, v in prof.items() if k.startswith("align_")}


@pytest.mark.parametrize("name", list(SC.INPUTS))
def test_the_stages_of_a_call(ctx, name):
    groups = SC.groups_of(name)
    longest = max(len(w) for g in groups for w in g)
    assert (longest <= 1000) == (name == "clean") and SC.tag_of(groups) == ("_short" if name == "clean" else "_long")
    for cap in SC.CAPS:
        for lanes in SC.LANES:
            exp = SC.expected_stages(groups, cap, lanes)
            for overlap in (1, 0):
                got = stages_once(ctx, groups, cap, lanes, overlap)
                print(name, cap, lanes, overlap, got)
                assert got == exp, (name, cap, lanes, overlap, got, exp)
