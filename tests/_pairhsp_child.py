"""helper of tests/test_gpu_pairhsp.py::test_small_batches_in_a_fresh_process: started once, as a fresh process, with
HITE_PAIRHSP_BATCH_PAIRS=257 (read when a context is created), so that the pairs go up in many batches.  Writes {"mixed": result} as
JSON to argv[1]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hite_amd  # noqa: E402
import pairhsp_cases as PC  # noqa: E402

if __name__ == "__main__":
    assert os.environ.get("HITE_PAIRHSP_BATCH_PAIRS") == "257"
    ctx = hite_amd.Context(0)
    try:
        seqs, pairs = PC.mixed()
        out = {"mixed": ctx.pair_hsps(seqs, pairs)}
    finally:
        ctx.close()
    with open(sys.argv[1], "w") as f:
        json.dump(out, f)
