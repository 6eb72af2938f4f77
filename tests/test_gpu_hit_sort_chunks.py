"""The per-candidate sort of the hits (hit_segsort_kernel of hite_amd/csrc/hite_copies.hip) at the cases of
tests/hit_sort_chunk_cases.py: chunks of 1, 3, 9, 15, 17, 31, 33 and 41 keys per thread on both sides of every place where a pass changes
shape, and genomes on both sides of the capacity of the contig table in LDS.  Per case: the device's table with its clip words == the
twin's on the default path and on HITE_HIT_SEGSORT=0 (global sort and cluster kernels; ONE fresh process for all the cases, through
tests/_copy_limits_child.py), the eight counts of copy_stats_ext() equal between the two paths, hits == the model's, clusters /
copies before the cap / chains == the closed forms, and every candidate searched ALONE gives the rows it has in its batch (state a
workgroup carries from one candidate to the next, the staged contig table among it, shows up there)."""
import json
import os
import pickle
import subprocess
import sys

import pytest

import hit_sort_chunk_cases as HC
import oracle_lib as O
from _copy_limits_child import run

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATHS = ("default", "global sort")


@pytest.fixture(scope="module")
def cases():
    return HC.all_cases()


@pytest.fixture(scope="module")
def twin(cases):
    """the twin's tables: computed once, shared, never changed"""
    out = {}
    try:
        for name, c in cases:
            O.find_copies_config(c["aligned"])
            out[name] = [[list(r) for r in rows] for rows in O.find_copies(c["contigs"], c["cands"], clips=True)]
    finally:
        O.find_copies_config(None)
    return out


@pytest.fixture(scope="module")
def paths(cases, tmp_path_factory):
    """the case list on the two paths: the default one in this process, the unfused one in one fresh child"""
    import hite_amd

    tmp = tmp_path_factory.mktemp("hit_sort_chunks")
    with open(tmp / "cases.pickle", "wb") as f:
        pickle.dump(cases, f)
    res = {}
    ctx = hite_amd.Context(0)
    try:
        res["default"] = run(ctx, cases)
    finally:
        ctx.close()
    out = tmp / "unfused.json"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_copy_limits_child.py"), str(out), str(tmp / "cases.pickle")],
                       env={**os.environ, "HITE_HIT_SEGSORT": "0"}, capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    with open(out) as f:
        res["global sort"] = json.load(f)
    return res


@pytest.mark.parametrize("name", HC.names())
def test_case_on_both_paths(name, paths, twin):
    c = HC.get(name)
    for p in PATHS:
        print(name, p, "stats", paths[p][name]["stats"])
    for p in PATHS:
        assert paths[p][name]["table"] == twin[name], (name, p)
    st = paths["default"][name]["stats"]
    assert len(st) == 8 and paths["global sort"][name]["stats"] == st, (name, paths["global sort"][name]["stats"], st)
    HC.check_stats(name, st)
    HC.check_closed_forms(name, twin[name])
    for k in c["alone"]:
        for p in PATHS:
            one = paths[p][name]["alone"][str(k)]
            assert one["rows"] == twin[name][k], (name, p, k)
            assert one["stats"] == paths["default"][name]["alone"][str(k)]["stats"], (name, p, k)
        HC.check_alone(name, k, paths["default"][name]["alone"][str(k)]["stats"])
