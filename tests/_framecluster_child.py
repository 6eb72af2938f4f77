"""helper of tests/test_gpu_framecluster.py::test_small_batches_in_a_fresh_process: started once, as a fresh process, with
HITE_FRAMECLUSTER_BATCH_BYTES=4096 (read when a context is created), so that the groups go up in many batches (a unit larger than a
batch runs alone).  Writes {"many": result, label: result ...} as JSON to argv[1]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hite_amd  # noqa: E402
import framecluster_cases as FC  # noqa: E402

if __name__ == "__main__":
    assert os.environ.get("HITE_FRAMECLUSTER_BATCH_BYTES") == "4096"
    ctx = hite_amd.Context(0)
    try:
        out = {"many": ctx.frame_cluster(FC.many_small(), **FC.SORT)}
        for label, groups, kw in FC.row_edges() + FC.length_edges():
            out[label] = ctx.frame_cluster(groups, **kw)
    finally:
        ctx.close()
    with open(sys.argv[1], "w") as f:
        json.dump(out, f)
