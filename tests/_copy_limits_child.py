"""helper of tests/test_gpu_copy_limits.py: runs the cases of copy_limit_cases through Context.find_copies and collects the copy
tables with their clip words, the copy finder's own counts, and the same for every candidate a case wants searched alone.  The test
calls run() in its own process (the default path, and restricted=True) and starts this file as a fresh process, once with
HITE_HIT_SEGSORT=0 HITE_HIT_HIST=1 (global sort + cluster kernels; the hits per candidate of the FIRST call go to stderr) and once
with HITE_HITS_WIDE=1 (the 12-byte hit form): both switches are read once per process.  The result goes to argv[1] as JSON; argv[2],
if given, is the pickled case list of the test (the child then does not build the cases a second time)."""
import json
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import copy_limit_cases as CL  # noqa: E402


def run(ctx, cases, restricted=False):
    """{name: {"table": per candidate list of records with clip words, "stats": copy_stats_ext(), "alone": {candidate: {"rows", "stats"}}}},
    as JSON would hand it back"""
    out = {}
    try:
        for name, case in cases:
            ctx.copy_config(case["aligned"])
            ctx.genome_pack(case["contigs"])
            ctx.release_copy_index()
            rec = {"table": ctx.find_copies(case["cands"], restricted=restricted, clips=True), "stats": ctx.copy_stats_ext(), "alone": {}}
            for k in case["alone"]:
                rows = ctx.find_copies([case["cands"][k]], restricted=restricted, clips=True)[0]
                rec["alone"][str(k)] = {"rows": rows, "stats": ctx.copy_stats_ext()}
            out[name] = rec
    finally:
        ctx.copy_config(None)
    return json.loads(json.dumps(out))


if __name__ == "__main__":
    assert os.environ.get("HITE_HIT_SEGSORT") == "0" or os.environ.get("HITE_HITS_WIDE") == "1"
    import hite_amd

    ctx = hite_amd.Context(0)
    try:
        if len(sys.argv) > 2:
            with open(sys.argv[2], "rb") as f:
                cases = pickle.load(f)
        else:
            cases = CL.all_cases()
        res = run(ctx, cases)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f)
    finally:
        ctx.close()
