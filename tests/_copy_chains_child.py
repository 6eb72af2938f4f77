"""helper of tests/test_gpu_copy_chains.py: runs the cases of copy_chain_cases through Context.find_copies and collects the copy
tables and the copy finder's own counts.  The test calls run() in its own process (the default path: chains straight from the
per-candidate sort) and starts this file once as a fresh process with HITE_HIT_SEGSORT=0 (global sort + cluster kernels; the
switch is read once per process) and HITE_HIT_HIST=1 (hits per candidate of the FIRST call, printed to stderr); the result goes
to argv[1] as JSON."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import copy_chain_cases as CC  # noqa: E402


def run(ctx, cases):
    """{label: {"table": per candidate list of records with clip words, "stats": copy_stats_ext(), "singles": copy_stats() of every
    snippet candidate searched alone (the case that has them)}}, as JSON would hand it back"""
    out = {}
    for label, case in cases:
        ctx.genome_pack(case["contigs"])
        ctx.release_copy_index()
        rec = {"table": ctx.find_copies(case["cands"], clips=True), "stats": ctx.copy_stats_ext()}
        if "first_snippet" in case:
            rec["singles"] = []
            for s in case["cands"][case["first_snippet"]:]:
                ctx.find_copies([s])
                rec["singles"].append(ctx.copy_stats())
        out[label] = rec
    return json.loads(json.dumps(out))


if __name__ == "__main__":
    assert os.environ.get("HITE_HIT_SEGSORT") == "0"
    import hite_amd

    ctx = hite_amd.Context(0)
    try:
        res = run(ctx, CC.all_cases())
        with open(sys.argv[1], "w") as f:
            json.dump(res, f)
    finally:
        ctx.close()
