"""helper of tests/test_gpu_ltrscan.py::test_volume_in_small_batches_in_a_fresh_process: started once, as a fresh process, with
HITE_LTRSCAN_BATCH_BYTES set (read when a context is created), so that the pieces of the volume genome go up in several batches.
argv: output path, number of pieces.  Writes {"records": ..., "stats": ...} as JSON"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hite_amd  # noqa: E402
import ltrscan_cases as LC  # noqa: E402

if __name__ == "__main__":
    assert int(os.environ["HITE_LTRSCAN_BATCH_BYTES"]) >= 1
    seq, cuts = LC.volume()
    pieces = LC.split(seq, cuts, int(sys.argv[2]))
    ctx = hite_amd.Context(0)
    try:
        st = {}
        out = {"records": ctx.ltr_scan(pieces, stats=st).tolist(), "stats": st}
    finally:
        ctx.close()
    with open(sys.argv[1], "w") as f:
        json.dump(out, f)
