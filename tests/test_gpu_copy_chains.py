"""The copy finder's chains straight from the per-candidate sort (hit_segsort_kernel's epilogue: cluster rule, runs, extreme anchors,
chain filters, chain table) against the CPU twin, record for record with the clip words, and against the path that keeps the cluster
kernels (HITE_HIT_SEGSORT=0: global sort, flags, scan, cluster arrays, chain_list_kernel), count for count: minimizers, hits,
clusters, copies, long-end chains, other chains and extension columns.  Cases: tests/copy_chain_cases.py."""
import os
import re
import subprocess
import sys

import pytest

import copy_chain_cases as CC
import oracle_lib as O
from _copy_chains_child import run

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return CC.all_cases()


@pytest.fixture(scope="module")
def twin(cases):
    """the twin's tables: computed once, shared, never changed"""
    return {label: [[list(r) for r in rows] for rows in O.find_copies(c["contigs"], c["cands"], clips=True)] for label, c in cases}


@pytest.fixture(scope="module")
def fused(cases):
    """default path, in this process"""
    import hite_amd

    ctx = hite_amd.Context(0)
    try:
        return run(ctx, cases)
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def unfused(tmp_path_factory):
    """HITE_HIT_SEGSORT=0 in ONE fresh process for all the cases; -> (results, the HITE_HIT_HIST line of its first call, the case "classes")"""
    out = tmp_path_factory.mktemp("copy_chains") / "unfused.json"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_copy_chains_child.py"), str(out)],
                       env={**os.environ, "HITE_HIT_SEGSORT": "0", "HITE_HIT_HIST": "1"}, capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    import json

    hist = [ln for ln in p.stderr.splitlines() if ln.startswith("hit_hist:")]
    assert len(hist) == 1, p.stderr[-2000:]
    return json.load(open(out)), hist[0]


def _same(label, fused, unfused, twin):
    """the table of the default path == the twin's == the other path's; all eight counts equal on both paths"""
    a, b = fused[label], unfused[0][label]
    print(label, "stats", a["stats"], "| global sort", b["stats"])
    assert a["table"] == twin[label]
    assert b["table"] == twin[label]
    assert a["stats"] == b["stats"]
    return a["stats"]


def test_every_sort_class_in_one_call(cases, fused, unfused, twin):
    """one candidate in each class of the per-candidate sort (<= 2048, <= 4096, <= 8192 hits, and the global ping-pong class above),
    beside candidates with no valid k-mer, with one hit (sorted by nobody, counted by the classify kernel) and with runs of exactly
    two and exactly three hits"""
    case = dict(cases)["classes"]
    st = _same("classes", fused, unfused, twin)
    print(unfused[1])
    m = re.search(r"above: candidates (\d+) (\d+) (\d+) (\d+) (\d+) hits (\d+) (\d+) (\d+) (\d+) (\d+)", unfused[1])
    ncand = [int(x) for x in m.groups()[:5]]
    assert sum(ncand) == len(case["cands"])
    assert ncand[1] >= 1 and ncand[2] >= 1 and ncand[3] >= 1 and ncand[4] >= 1, ncand       # 1025 .. 2048, .. 4096, .. 8192, above
    assert st[1] > 0 and st[2] > 0 and st[3] > 0
    assert st[4] + st[5] >= st[3] >= sum(len(t) for t in twin["classes"])                          # every copy was a chain
    for k in range(case["n_fam"]):
        assert len(twin["classes"][k]) >= 5
    for k in range(case["n_fam"], case["first_snippet"]):                                   # no valid k-mer
        assert twin["classes"][k] == []
    # the snippets, each searched alone: same counts on both paths; among them one hit, a run of exactly two, a run of exactly three
    singles = fused["classes"]["singles"]
    assert singles == unfused[0]["classes"]["singles"]
    print("snippets alone (minimizers, hits, clusters, copies):", singles)
    runs = {s[1] for s in singles if s[2] == 1}
    assert {1, 2, 3} <= runs, runs


def test_cluster_rule_at_its_edges(fused, unfused, twin):
    """two anchor blocks of one strand whose diagonals differ by TD - 1, TD (one cluster) and TD + 1 (two), through a deletion and
    through an insertion, on both strands; and a copy cut by a contig end, whose halves share a diagonal"""
    st = _same("edges", fused, unfused, twin)
    # per candidate (the element and its reverse complement): the intact copy is 1 cluster, the copy cut by the contig end 2, the 8
    # copies with an indel of TD - 1 or TD bases 1 each, the 4 with TD + 1 bases 2 each; only the 9 single-cluster copies cover the
    # candidate
    assert st[2] == 2 * (1 + 2 + 8 + 4 * 2)
    assert st[4] + st[5] <= st[2]
    assert [len(t) for t in twin["edges"]] == [9, 9] and st[3] == 18


def test_one_cluster_and_all_singletons(cases, fused, unfused, twin):
    """a candidate whose whole range is one cluster, one whose range is all singletons (no chain), and low-complexity candidates"""
    _same("one-and-singletons", fused, unfused, twin)
    case = dict(cases)["one-and-singletons"]
    import hite_amd

    ctx = hite_amd.Context(0)
    try:
        ctx.genome_pack(case["contigs"])
        ctx.find_copies(case["cands"][:1])
        one = ctx.copy_stats_ext()
        ctx.find_copies(case["cands"][1:])
        sing = ctx.copy_stats_ext()
    finally:
        ctx.close()
    print("one cluster:", one, "singletons:", sing)
    assert one[1] >= 100 and one[2] == 1 and one[4] + one[5] == 1 and one[3] == 1
    assert sing[1] >= 10 and sing[2] == sing[1] and sing[4] + sing[5] == 0 and sing[3] == 0
    assert len(twin["one-and-singletons"][0]) == 1 and twin["one-and-singletons"][1] == []
    _same("low-complexity", fused, unfused, twin)


def test_long_end_chains_are_listed_first(fused, unfused, twin):
    """a candidate with >= EXT_LONG bases beyond its outermost anchor (its first 400 bases hold no intact 15-mer): its chains go to the
    front of the chain table, the intact candidate's to the back; found, with the twin's clip words"""
    st = _same("long-end", fused, unfused, twin)
    assert st[4] >= 2 and st[5] >= 1                 # long-end chains (worn candidate, both strands) and others (intact candidate)
    for k in range(3):
        assert len(twin["long-end"][k]) >= 1, k
