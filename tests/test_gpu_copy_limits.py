"""The copy finder (hite_amd/csrc/hite_copies.hip: candidate minimizers, occurrences, hits, per-candidate sort, chains, end extension,
filters, cap and order) at the limits tests/copy_limit_cases.py builds, on four paths: (a) the default one, (b) HITE_HIT_SEGSORT=0
(global sort and cluster kernels) and (c) HITE_HITS_WIDE=1 (12-byte hits), each in ONE fresh process, and (d) the restricted index.
Per case: the table with its clip words == the twin's on all four paths, all eight counts equal on (a), (b) and (c), candidate
minimizers and hits == the model's, clusters / copies before the cap / chains == the closed forms of the construction, and every
candidate of the minimizer and chain cases searched ALONE gives the rows it has in its batch (state a workgroup carries from one
candidate to the next shows up there).  tests/test_copy_limit_cases.py holds the twin to the same cases without a GPU."""
import json
import os
import pickle
import re
import subprocess
import sys

import pytest

import copy_limit_cases as CL
import oracle_lib as O
from _copy_limits_child import run

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATHS = ("default", "global sort", "wide hits", "restricted")


def _child(tmp, tag, env):
    out = tmp / (tag + ".json")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_copy_limits_child.py"), str(out), str(tmp / "cases.pickle")], env={**os.environ, **env},
                       capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    with open(out) as f:
        return json.load(f), p.stderr


@pytest.fixture(scope="module")
def cases():
    return CL.all_cases()


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
    """the case list on the four paths, in this order; -> ({path: results}, the HITE_HIT_HIST line of the global-sort process)"""
    import hite_amd

    tmp = tmp_path_factory.mktemp("copy_limits")
    with open(tmp / "cases.pickle", "wb") as f:
        pickle.dump(cases, f)
    res = {}
    ctx = hite_amd.Context(0)
    try:
        res["default"] = run(ctx, cases)
        res["global sort"], err = _child(tmp, "unfused", {"HITE_HIT_SEGSORT": "0", "HITE_HIT_HIST": "1"})
        res["wide hits"], _err = _child(tmp, "wide", {"HITE_HITS_WIDE": "1"})
        res["restricted"] = run(ctx, cases, restricted=True)
    finally:
        ctx.close()
    hist = [ln for ln in err.splitlines() if ln.startswith("hit_hist:")]
    assert len(hist) == 1, err[-2000:]
    return res, hist[0]


@pytest.mark.parametrize("name", CL.names())
def test_case_on_every_path(name, paths, twin):
    res = paths[0]
    c = CL.get(name)
    for p in PATHS:
        print(name, p, "stats", res[p][name]["stats"])
    for p in PATHS:
        assert res[p][name]["table"] == twin[name], (name, p)
    st = res["default"][name]["stats"]
    for p in PATHS[1:3]:
        assert res[p][name]["stats"] == st, (name, p, res[p][name]["stats"], st)
    CL.check_stats(name, st)
    CL.check_closed_forms(name, twin[name])
    for k in c["alone"]:
        for p in PATHS:
            one = res[p][name]["alone"][str(k)]
            assert one["rows"] == twin[name][k], (name, p, k)
            if p != "restricted":
                assert one["stats"] == res["default"][name]["alone"][str(k)]["stats"], (name, p, k)
        CL.check_alone(name, k, res["default"][name]["alone"][str(k)]["stats"])


def test_hit_classes_of_the_first_call(paths):
    """the six candidates of hit_classes (2048, 2049, 4096, 4097, 8192 and 8193 hits) in the classes of the per-candidate sort, as the
    device counts them"""
    line = paths[1]
    print(line)
    m = re.search(r"candidates (\d+) hits (\d+) max (\d+) .*above: candidates (\d+) (\d+) (\d+) (\d+) (\d+) hits (\d+) (\d+) (\d+) (\d+) (\d+)", line)
    g = [int(x) for x in m.groups()]
    assert g[0] == 6 and g[1] == 2 * (2048 + 4096 + 8192) + 3 and g[2] == 8193
    assert g[3:8] == [0, 1, 2, 2, 1] and g[8:13] == [0, 2048, 2049 + 4096, 4097 + 8192, 8193]
