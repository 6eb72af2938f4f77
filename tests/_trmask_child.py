"""helper of tests/test_gpu_trmask.py::test_on_the_spot_extension_path: started once, as a fresh process, with HITE_TR_DEFER=0 (the
switch is read once per process): hite_tr_mask then keeps no seed list and every seed is extended by the thread that found it, the
path a full list falls back to.  Opens its own context on GPU 0, masks the listed cases and writes {label: [bases, hex of the mask
packed with np.packbits]} as JSON to argv[1]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hite_amd  # noqa: E402
import trmask_cases as TC  # noqa: E402


def cases():
    """[(label, contigs, max_period)]: the parent compares the same list"""
    out = [(lab, contigs, P) for lab, contigs, P, _n in TC.border_cases() if P == 500]
    out += [("period-P%d" % P, TC.period_genome(), P) for P in (63, 64, 500)]
    return out


if __name__ == "__main__":
    assert os.environ.get("HITE_TR_DEFER") == "0"
    ctx = hite_amd.Context(0)
    try:
        out = {}
        for label, contigs, P in cases():
            ctx.genome_pack(contigs)
            m = ctx.tr_mask(P)
            out[label] = [int(m.size), np.packbits(m).tobytes().hex()]
        with open(sys.argv[1], "w") as f:
            json.dump(out, f)
    finally:
        ctx.close()
