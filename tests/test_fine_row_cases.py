"""The cases of tests/fine_row_cases.py on the CPU: every check_* with the twin (tests/oracle_pipeline.py: pass_rows, O.clip_probe) in
the device's place, the self-checks that show, by the twin alone, that each case reaches the limit it is named for, and the twin's
choice of 100 rows among equal lengths against the machine's own `sort -nk 2 -r` under LC_ALL=C (what tools/ready_for_MSA.sh of the
reference runs on the .fai).  tests/test_gpu_fine_rows.py holds the device to the same checks."""
import os
import shutil
import subprocess

import pytest

import fine_row_cases as FR
import oracle_pipeline as OP


@pytest.fixture(scope="module")
def twin():
    return FR.Twin()


def test_select_reaches_its_limits():
    FR.selfcheck_select()


def test_ties_reach_their_limits():
    FR.selfcheck_ties()


def test_slots_reach_their_limits():
    FR.selfcheck_slots()


def test_gather_reaches_its_limits():
    FR.selfcheck_gather()


def test_pads_reach_their_limits():
    FR.selfcheck_pads()


def test_probe_reaches_its_limits():
    FR.selfcheck_probe()


def test_checks_with_the_twin(twin):
    FR.check_select(twin)
    FR.check_ties(twin)
    FR.check_slots(twin)
    for name in FR.gather_names():
        FR.check_gather(twin, name)
    for name in FR.pad_names():
        FR.check_pads(twin, name)
    FR.check_probe(twin)


def test_independence_with_the_twin(twin):
    for part in range(3):
        FR.check_independence(twin, part, 3)


def test_stage_with_the_twin(twin):
    FR.check_stage_stats(twin)
    FR.check_stage_stats_passing(twin)
    for te in ("tir", "helitron", "non_ltr"):
        assert 6 <= FR.check_end_to_end(twin, te) <= 12


@pytest.mark.skipif(shutil.which("sort") is None, reason="no sort on this machine")
def test_ties_against_a_real_sort(tmp_path):
    """name <tab> length lines through `sort -nk 2 -r` in the POSIX locale: its first 100 lines are the windows the twin keeps (as a
    multiset of names: the two lines of a record given twice are the same line)"""
    env = dict(os.environ, LC_ALL="C")
    n = 0
    cases = [c for c, _numeric in FR.tie_cases()] + [{"name": "modes_%d" % k, "cands": [FR.case_modes()["cands"][k]], "copies": [FR.case_modes()["copies"][k]]}
                                                     for k in (2, 3)]
    for c in cases:
        for names in (FR.NAMES, None):
            for cut in (True, False):
                recs = OP.pass_records(c["cands"][0], c["copies"][0], FR.genome()["contigs"], c.get("flank", FR.FLANK), names)
                recs = [r for r in recs if r[5]] if cut else recs
                if len(recs) <= FR.MAXROWS:
                    continue
                nm, ln = [r[2] for r in recs], [1000 if cut else len(r[1]) for r in recs]
                f = tmp_path / "fai"
                f.write_text("".join("%s\t%d\n" % (a, b) for a, b in zip(nm, ln)))
                out = subprocess.run(["sort", "-nk", "2", "-r", str(f)], env=env, check=True, capture_output=True, text=True).stdout
                want = sorted(line.split("\t")[0] for line in out.splitlines()[:FR.MAXROWS])
                assert sorted(nm[i] for i in OP.select_rows(ln, nm)) == want, (c["name"], names is None, cut)
                n += 1
    assert n >= 12


def test_consensus_pool_table_has_every_kind():
    t = FR.cons_pool_table()
    assert 8 <= len(t["cands"]) <= 12 and sum(1 for r in t["expect"] if r[0]) >= 3
