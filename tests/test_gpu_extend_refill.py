"""chain_extend_kernel with windows refilled 16 bases at a time (hite_ext.h) == the twin, on the cases of extend_refill_cases: ends of
0 .. 2048 bases to the left and to the right on both strands, candidates at every offset mod 16 of the candidate buffer, a batch
of over 1000 (chain, end) tasks of mixed lengths, and a genome of 120 contigs whose ends the walks meet.  Every case runs in this process and in two fresh ones (tests/_copy_limits_child.py
with the 12-byte hits, which take the same extension kernel): one as it is, one with HITE_EXT_BLOCKS=1 -- a single block of four
wavefronts, whose lanes take task after task at whatever column the last one ended, where the uncapped grid has a lane per task.  The
copy tables with their clip words must be the twin's row for row, and copy_stats_ext() (the DP columns among them) the same with and
without the cap."""
import json
import os
import pickle
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import extend_refill_cases as EC  # noqa: E402
import oracle_lib as O  # noqa: E402
from _copy_limits_child import run  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ("end_lengths", "cand_offsets", "mixed_batch", "many_contigs")
PATHS = ("default", "wide hits", "wide hits, one block")


def _child(tmp, tag, env):
    out = tmp / (tag + ".json")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_copy_limits_child.py"), str(out), str(tmp / "cases.pickle")],
                       env={**{k: v for k, v in os.environ.items() if k != "HITE_EXT_BLOCKS"}, **env}, capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    with open(out) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def cases():
    return EC.all_cases()


@pytest.fixture(scope="module")
def twin(cases):
    """the twin's tables: computed once, shared, never changed"""
    return {name: [[list(r) for r in rows] for rows in O.find_copies(c["contigs"], c["cands"], clips=True)] for name, c in cases}


@pytest.fixture(scope="module")
def paths(cases, tmp_path_factory):
    import hite_amd

    tmp = tmp_path_factory.mktemp("extend_refill")
    with open(tmp / "cases.pickle", "wb") as f:
        pickle.dump(cases, f)
    res = {}
    ctx = hite_amd.Context(0)
    try:
        res["default"] = run(ctx, cases)
    finally:
        ctx.close()
    res["wide hits"] = _child(tmp, "wide", {"HITE_HITS_WIDE": "1"})
    res["wide hits, one block"] = _child(tmp, "capped", {"HITE_HITS_WIDE": "1", "HITE_EXT_BLOCKS": "1"})
    return res


@pytest.mark.parametrize("name", NAMES)
def test_case_capped_and_uncapped(name, paths, twin):
    for p in PATHS:
        print(name, p, "stats", paths[p][name]["stats"])
    assert sum(len(r) for r in twin[name]) > 0
    for p in PATHS:
        assert paths[p][name]["table"] == twin[name], (name, p)
    st = paths["wide hits"][name]["stats"]
    assert paths["wide hits, one block"][name]["stats"] == st, (name, paths["wide hits, one block"][name]["stats"], st)
    assert paths["default"][name]["stats"] == st, (name, paths["default"][name]["stats"], st)
    if name == "end_lengths":
        assert st[4] > 0 and st[5] > 0, st                      # chains with an end of >= 384 bases and the others
    if name == "mixed_batch":
        assert 2 * (st[4] + st[5]) >= 1000, st                  # tasks, for the 256 lanes of the capped run
