"""helper of tests/test_gpu_ltrdeep.py::test_same_bits_at_every_batch_size_and_place: started as a fresh process with
HITE_LTRDEEP_BATCH set or unset (it is read when a context is created).  Scores the first 9 matrices of the fixture with the fixture's
model in three orders -- as they are, rotated by 4 and rotated by 8, so that every matrix is once the first, once in the middle and
once the last of the call -- and writes logits [3, 9, 2] and pooled [3, 9, 64], each brought back to the fixture's order, to argv[1] (.npz)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hite_amd  # noqa: E402
from conftest import load_golden  # noqa: E402

N, ROTATIONS = 9, (0, 4, 8)

if __name__ == "__main__":
    mats = [c["matrix"] for c in load_golden("ltr_deep")["cases"][:N]]
    params = np.load(os.path.join(ROOT, "tests", "golden", "ltr_deep_model.npy"))
    ctx = hite_amd.Context(0)
    try:
        model = ctx.ltr_model(params)
        logits, pooled = np.zeros((len(ROTATIONS), N, 2), dtype=np.float32), np.zeros((len(ROTATIONS), N, 64), dtype=np.float32)
        for k, rot in enumerate(ROTATIONS):
            order = [(i + rot) % N for i in range(N)]
            lg, pl, status = ctx.ltr_deep(model, [mats[i] for i in order], pooled=True)
            assert not status.any()
            logits[k, order], pooled[k, order] = lg, pl
    finally:
        ctx.close()
    np.savez(sys.argv[1], logits=logits, pooled=pooled)
