"""CPU-only: the host layer of FiLTR's steps 1 and 2 (hite_amd/util.py: read_scn, get_recombination_ltr,
get_all_potential_ltr_lines, remove_dirty_LTR, filter_ltr_by_flank_seq_v2, ltr_scn_filter).
  - The rules around the search are pinned to the REFERENCE's own code: tests/golden/ltr_scn_filter.json.gz
    (tools/gen_ltr_scn_fixture.py) holds a planted genome, the HSP table of every search the reference made on it and what the
    reference's functions wrote; util's functions, with hsps= fed from those tables, must write the same.
  - ltr_scn_filter with the twin (tests/pairhsp_twin.py) on synth.make_ltr_element_genome gives the planted decision for every kind."""
import os
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pairhsp_twin as T  # noqa: E402
from hite_amd import synth, util  # noqa: E402
from ltr_scn_cases import PLAN, SEED, load_fixture, table_hsps, write_inputs  # noqa: E402


class Log:
    def __init__(self):
        self.lines = []
        self.logger = types.SimpleNamespace(info=self.lines.append, debug=self.lines.append, error=self.lines.append)


def test_read_scn_as_the_reference(tmp_path):
    fx = load_fixture()
    scn_path, _ = write_inputs(tmp_path, fx["contigs"], fx["scn"])
    for key, dup in (("read_scn", False), ("read_scn_remove_dup", True)):
        cand, lines = util.read_scn(scn_path, None, remove_dup=dup)
        assert list(cand) == list(range(len(cand))) == list(lines)
        assert [list(cand[k]) for k in cand] == fx[key]["candidates"] and [lines[k] for k in lines] == fx[key]["lines"]
    assert len(fx["read_scn"]["lines"]) == len(fx["read_scn_remove_dup"]["lines"]) + 2
    out = os.path.join(str(tmp_path), "copy.scn")
    util.store_scn(fx["read_scn"]["lines"], out)
    assert open(out).read() == "".join(x + "\n" for x in fx["read_scn"]["lines"])


def test_steps_with_the_reference_tables_give_the_reference_outputs(tmp_path):
    fx = load_fixture()
    scn_path, ref_path = write_inputs(tmp_path, fx["contigs"], fx["scn"])
    tabs = fx["hsp_tables"]
    _names, ref_contigs = util.read_fasta(ref_path)
    cand, lines = util.read_scn(scn_path, None, remove_dup=True)
    used = set()
    recomb = util.get_recombination_ltr(cand, ref_contigs, 1, str(tmp_path), None, hsps=table_hsps(tabs["recombination"], used))
    assert recomb == fx["recombination_candidates"] and len(recomb) == 3 and len(used) == len(tabs["recombination"])
    confident = [lines[k] for k in cand if k not in recomb]
    side = os.path.join(str(tmp_path), "all_potential_ltr.json")
    used = set()
    potential = util.get_all_potential_ltr_lines(confident, ref_path, 1, side, str(tmp_path), None, hsps=table_hsps(tabs["potential_lines"], used))
    assert potential == fx["potential_lines"] and len(potential) > len(confident) and len(used) == len(tabs["potential_lines"])
    assert open(side, encoding="utf-8").read() == fx["potential_json"]
    dirty = util.remove_dirty_LTR(potential, None)
    assert dirty == fx["dirty_dicts"] and len(dirty) >= 4
    recomb_scn, final_scn = os.path.join(str(tmp_path), "remove_recomb.scn"), os.path.join(str(tmp_path), "final.scn")
    util.store_scn(potential, recomb_scn)
    assert open(recomb_scn).read() == fx["remove_recomb_scn"]
    used = set()
    kept = util.filter_ltr_by_flank_seq_v2(recomb_scn, final_scn, ref_path, 1, str(tmp_path), None, hsps=table_hsps(tabs["flank_align"], used))
    assert open(final_scn).read() == fx["filter_terminal_align_scn"] == "".join(x + "\n" for x in kept)
    assert len(used) == len(tabs["flank_align"]) and kept and kept != potential


def test_driver_with_the_reference_tables(tmp_path):
    fx = load_fixture()
    scn_path, ref_path = write_inputs(tmp_path, fx["contigs"], fx["scn"])
    tabs = fx["hsp_tables"]
    seconds = {}
    final, dirty, terminals = util.ltr_scn_filter(scn_path, ref_path, os.path.join(str(tmp_path), "out"), seconds=seconds,
                                                  hsps=table_hsps(tabs["recombination"] + tabs["potential_lines"] + tabs["flank_align"]))
    assert open(final).read() == fx["filter_terminal_align_scn"] and dirty == fx["dirty_dicts"]
    assert open(os.path.join(str(tmp_path), "out", "remove_recomb.scn")).read() == fx["remove_recomb_scn"]
    assert {"recombination", "potential_lines", "flank_align"} <= set(seconds)
    # the left terminals: chr-start-end, a repeated name with -repN, the sequence of the line
    kept = fx["filter_terminal_align_scn"].splitlines()
    assert len(terminals) == len(kept)
    for name, line in zip(terminals, kept):
        p = line.split(" ")
        assert name.startswith("%s-%s-%s" % (p[11], p[3], p[4])) and terminals[name] == fx["contigs"][p[11]][int(p[3]) - 1:int(p[4])]
    assert len(set(terminals)) == len(terminals)


def test_refused_pairs_are_treated_as_a_failed_search(tmp_path):
    """a pair the search refuses: not recombinant, its line gives no line in step 1b and is not kept in step 2; the count is logged"""
    fx = load_fixture()
    scn_path, ref_path = write_inputs(tmp_path, fx["contigs"], fx["scn"])
    _names, ref_contigs = util.read_fasta(ref_path)
    cand, lines = util.read_scn(scn_path, None, remove_dup=True)
    none = lambda seqs, pairs, diag_min=None: [None] * len(pairs)  # noqa: E731
    log = Log()
    assert util.get_recombination_ltr(cand, ref_contigs, 1, str(tmp_path), log, hsps=none) == []
    assert util.get_all_potential_ltr_lines(list(lines.values()), ref_contigs, 1, os.path.join(str(tmp_path), "p.json"), str(tmp_path), log, hsps=none) == []
    assert util.filter_ltr_by_flank_seq_v2(scn_path, os.path.join(str(tmp_path), "f.scn"), ref_contigs, 1, str(tmp_path), log, hsps=none) == []
    assert open(os.path.join(str(tmp_path), "f.scn")).read() == ""
    assert sum("beyond the limits of the search" in x for x in log.lines) == 3 and any(x.startswith("get_recombination_ltr: %d pairs" % len(cand)) for x in log.lines)


def test_rules_on_made_up_tables():
    """the two boundary tests, the coverage and the offsets of step 2 and the line arithmetic of step 1b at their edges"""
    # a terminal of 200 bases, window +- 50: the alignment may begin at 40 .. 60 and end at 240 .. 260
    j = lambda hs: util.judge_flank_hsps(hs, 200, 200, 1000, 1199, 5000, 5199)  # noqa: E731
    assert j([(50, 249, 50, 249, 400, 200, 200)]) == (1, None)
    assert j([(45, 253, 46, 252, 400, 200, 200)]) == (1, (995, 1203, 4996, 5202))
    assert j([(39, 249, 50, 249, 400, 200, 200)]) == (0, None) and j([(40, 229, 60, 249, 1, 1, 1)]) == (1, (990, 1199, 5010, 5199))
    assert j([(40, 219, 60, 239, 1, 1, 1)]) == (0, None)          # 179 of 200 covered
    assert j([(50, 150, 50, 150, 1, 1, 1), (160, 249, 160, 249, 1, 1, 1)]) == (1, None)      # two pieces: 100 + 89 >= 180
    assert j([(1, 300, 1, 300, 600, 300, 300)]) == (0, None) and j([]) == (0, None)
    line = "1001 9000 8000 1001 1500 500 8501 9000 500 95.00 7 chrX"
    rep = (101, 500, 2101, 2500, 780, 395, 400)       # 98.75 %, 399 long, 1 601 apart
    assert util.ltr_lines_from_hsps(line, 1500, "chrX", "7", [rep]) == [line, "1601 4000 2400 1601 2000 400 3601 4000 400 98.75 7 chrX"]
    assert util.ltr_lines_from_hsps(line, 1500, "chrX", "7", [(101, 401, 2101, 2401, 1, 286, 301)]) == [line]      # 95.017 passes ...
    assert util.ltr_lines_from_hsps(line, 1500, "chrX", "7", [(101, 402, 2101, 2402, 1, 287, 302)])[1:] != []
    assert util.ltr_lines_from_hsps(line, 1500, "chrX", "7", [(101, 402, 2101, 2402, 1, 286, 302)]) == [line]      # ... 94.702 does not
    assert util.ltr_lines_from_hsps(line, 1500, "chrX", "7", [(101, 500, 1000, 1399, 780, 395, 400)]) == [line]    # more than 500 apart is needed
    assert util.blast6_identity(286, 301) == 95.017 and util.blast6_identity(1, 3) == 33.333
    assert util.merge_intervals([(5, 9), (1, 5), (20, 30)]) == [(1, 9), (20, 30)]


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    g = synth.make_ltr_element_genome(PLAN, seed=SEED)
    d = tmp_path_factory.mktemp("planted")
    scn_path, ref_path = write_inputs(d, g["contigs"], g["scn"])
    return g, scn_path, ref_path, str(d)


def test_planted_elements_through_the_twin(planted):
    g, scn_path, ref_path, d = planted
    seconds = {}
    final, dirty, terminals = util.ltr_scn_filter(scn_path, ref_path, os.path.join(d, "twin"), hsps=T.pair_hsps, seconds=seconds)
    recomb_lines = open(os.path.join(d, "twin", "remove_recomb.scn")).read().splitlines()
    final_lines = open(final).read().splitlines()
    table, wrong = synth.ltr_element_decisions(g["truth"], recomb_lines, final_lines, dirty)
    assert not wrong, (table, [g["truth"][w] for w in wrong])
    assert {k: v[1] for k, v in table.items()} == dict(PLAN, inner=3)
    assert len(terminals) == len(final_lines) and set(seconds) >= {"recombination", "potential_lines", "flank_align"}
