"""GPU: FiLTR's steps 1 and 2 on the lines of a `.scn` candidate table (util.ltr_scn_filter) with the searches on the device
(Context.pair_hsps): the same files as through the CPU twin and the planted decision for every kind of element, the searches of the
golden fixture (tests/golden/ltr_scn_filter.json.gz) equal to its tables, and the step's third result handed on to
util.ltr_flank_filter (step 3), which closes the chain from the `.scn` file to the is_LTR table."""
import os

import pytest

import pairhsp_twin as T
from ltr_scn_cases import PLAN, SEED, load_fixture, pair_key, table_of, write_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from hite_amd import synth, util

    g = synth.make_ltr_element_genome(PLAN, seed=SEED)
    d = str(tmp_path_factory.mktemp("ltr_scn"))
    scn_path, ref_path = write_inputs(d, g["contigs"], g["scn"])
    ctx = util.set_reference(ref_path)
    return dict(g=g, d=d, scn=scn_path, ref=ref_path, ctx=ctx)


def test_planted_elements_device_equals_twin_equals_truth(world):
    from hite_amd import synth, util

    seconds = {}
    final, dirty, terminals = util.ltr_scn_filter(world["scn"], world["ref"], os.path.join(world["d"], "gpu"), ctx=world["ctx"], seconds=seconds)
    final_t, dirty_t, terminals_t = util.ltr_scn_filter(world["scn"], world["ref"], os.path.join(world["d"], "twin"), hsps=T.pair_hsps)
    for name in ("remove_recomb.scn", "filter_terminal_align.scn", "all_potential_ltr.json"):
        got = open(os.path.join(world["d"], "gpu", name), "rb").read()
        assert got == open(os.path.join(world["d"], "twin", name), "rb").read() and got, name
    assert dirty == dirty_t and terminals == terminals_t and os.path.basename(final) == "filter_terminal_align.scn"
    recomb_lines = open(os.path.join(world["d"], "gpu", "remove_recomb.scn")).read().splitlines()
    table, wrong = synth.ltr_element_decisions(world["g"]["truth"], recomb_lines, open(final).read().splitlines(), dirty)
    assert not wrong, (table, wrong)
    assert {k: v[1] for k, v in table.items()} == dict(PLAN, inner=3)
    assert {"recombination", "potential_lines", "flank_align"} <= set(seconds)
    world["terminals"] = terminals


def test_searches_of_the_golden_fixture(world, tmp_path):
    """every search the reference made on the fixture's genome, through the device: the fixture's HSP tables, and so its outputs"""
    from hite_amd import util

    fx = load_fixture()
    scn_path, ref_path = write_inputs(tmp_path, fx["contigs"], fx["scn"])
    tabs = fx["hsp_tables"]
    by_key = table_of(tabs["recombination"] + tabs["potential_lines"] + tabs["flank_align"])
    seen = set()

    def checked(seqs, pairs, diag_min=None):
        res = world["ctx"].pair_hsps(seqs, pairs, diag_min)
        for pair, r in zip(pairs, res):
            key = pair_key(seqs, pair, diag_min)
            assert r == by_key[key], key
            seen.add(key)
        return res

    final, dirty, _terminals = util.ltr_scn_filter(scn_path, ref_path, os.path.join(str(tmp_path), "out"), hsps=checked)
    assert seen == set(by_key) and len(seen) >= 60
    assert open(final).read() == fx["filter_terminal_align_scn"] and dirty == fx["dirty_dicts"]


def test_terminals_go_on_to_the_flank_filter(world):
    """the `.scn` -> is_LTR chain: the left terminals of the kept lines through step 3 on the same genome"""
    from hite_amd import util

    terminals = world.get("terminals") or util.ltr_scn_filter(world["scn"], world["ref"], os.path.join(world["d"], "again"), ctx=world["ctx"])[2]
    table, _high = util.ltr_flank_filter(terminals, world["ref"], 100, ctx=world["ctx"])
    assert set(table) == set(terminals) and len(table) >= 20
    assert all(isinstance(v[0], bool) and v[1] in ("low", "high", None) for v in table.values())
