"""helper of tests/test_gpu_subcluster.py::test_small_chunks_in_a_fresh_process: started once, as a fresh process, with
HITE_SUBCLUSTER_CHUNK_ROWS=8 (read when a context is created): every alignment of more than 8 rows then takes the chunked path
(phase A, phase B, the ordered pass, several chunks) that only alignments of more than HITE_SUBCLUSTER_CHUNK rows take by default.
A second context, created with HITE_SUBCLUSTER_BATCH_BYTES=4096 on top, sends the same alignments up in many batches (some
alignments are larger than a batch).  Writes {"chunk": {label: result}, "batches": {label: result}} as JSON to argv[1]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hite_amd  # noqa: E402
import subcluster_cases as SC  # noqa: E402


def cases():
    """[(label, alignments, cutoff)]: the parent compares the same list"""
    return [("families", SC.family_batch(), 0.2)] + SC.order() + SC.leader_counts()


def run(ctx):
    return {label: ctx.msa_subcluster(als, cutoff) for label, als, cutoff in cases()}


if __name__ == "__main__":
    assert os.environ.get("HITE_SUBCLUSTER_CHUNK_ROWS") == "8" and "HITE_SUBCLUSTER_BATCH_BYTES" not in os.environ
    out = {}
    ctx = hite_amd.Context(0)
    try:
        out["chunk"] = run(ctx)
    finally:
        ctx.close()
    os.environ["HITE_SUBCLUSTER_BATCH_BYTES"] = "4096"
    ctx = hite_amd.Context(0)
    try:
        out["batches"] = run(ctx)
    finally:
        ctx.close()
    with open(sys.argv[1], "w") as f:
        json.dump(out, f)
