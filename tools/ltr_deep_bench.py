#!/usr/bin/env python
"""The high-copy LTR vote of FiLTR's hybrid CNN (hite_ltr_deep, Context.ltr_deep) on one GPU: `--candidates` seeded matrices of 100
rows (two in three with unrelated flanks, the others with flanks from one ancestor), the parameters of tests/golden/ltr_deep_model.npy.
  - host-to-host seconds of one call (packing, copies and the batches included), best of `--repeat`, and candidates per second;
  - the device time of the features, the convolutions and the head from HIP events (hite_profile_*);
  - the achieved share of the fp32 peak of the convolution kernels: the multiply-adds the definition needs (the 3 x 3 and the 1 x 1
    convolutions of both branches, counted from the shapes) x 2 over the convolutions' device time, against 157.3 TFLOP/s;
  - for comparison on the same machine: the twin's integer features (numpy, one process) on `--cpu-candidates` matrices plus a
    torch-CPU float32 restatement of the model on `--threads` threads; results held against the device's.
The reference's own programs do not exist on the GPU machine: their time is taken once where the reference tree is and quoted in the
record as such.
    python tools/ltr_deep_bench.py [--out profiles/r16_ltr_deep.txt]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ACGT = np.frombuffer(b"ACGT-", np.uint8)
PEAK_FP32 = 157.3e12


def make_matrices(rng, n, rows=100):
    out = []
    for k in range(n):
        if k % 3 == 2:
            anc = rng.integers(0, 4, size=200)
            m = np.where(rng.random((rows, 200)) < 0.06, rng.integers(0, 4, size=(rows, 200)), anc)
        else:
            m = rng.integers(0, 4, size=(rows, 200))
        m = np.where(rng.random((rows, 200)) < 0.03, 4, m)
        out.append([r.tobytes().decode() for r in ACGT[m]])
    return out


def model_macs():
    """multiply-adds per candidate of the convolutions (3 x 3 twice and the 1 x 1 shortcut per block, both branches)"""
    macs = 0
    for c0, pixels in ((3, 100 * 200), (2, 3872)):
        for cin, cout in ((c0, 8), (8, 16), (16, 32)):
            macs += pixels * (cin * cout * 9 + cout * cout * 9 + cin * cout)
    return macs


def torch_model(params, threads):
    """class CNNCAT restated with torch.nn.functional in float32 on the CPU: (img [n,3,100,200], kmer [n,2,1,3872]) -> logits"""
    import torch
    import ltrdeep_twin as T

    torch.set_num_threads(threads)
    F = torch.nn.functional
    P = {k: torch.from_numpy(v.astype(np.float32)) for k, v in T.unpack(params).items()}
    bn = lambda x, key: F.batch_norm(x, P[key + ".running_mean"], P[key + ".running_var"], P[key + ".weight"], P[key + ".bias"], False, 0.0, 1e-5)  # noqa: E731

    def run(img, kmer):
        with torch.no_grad():
            pooled = []
            for branch, x in (("model", F.normalize(torch.from_numpy(img).float(), p=2.0, dim=1)), ("model_kmer", F.normalize(torch.from_numpy(kmer).float(), p=2.0, dim=1))):
                for b in range(3):
                    key = "%s.%d" % (branch, b)
                    t = F.relu(bn(F.conv2d(x, P[key + ".conv1.weight"], padding=1), key + ".bn1"))
                    x = F.relu(bn(F.conv2d(t, P[key + ".conv2.weight"], padding=1), key + ".bn2") + bn(F.conv2d(x, P[key + ".shortcut.0.weight"]), key + ".shortcut.1"))
                pooled.append(x.mean(dim=(2, 3)))
            h = F.relu(bn(F.linear(torch.cat(pooled, 1), P["fc_layers.0.weight"], P["fc_layers.0.bias"]), "fc_layers.1"))
            h = F.relu(bn(F.linear(h, P["fc_layers.4.weight"], P["fc_layers.4.bias"]), "fc_layers.5"))
            return F.linear(h, P["fc_layers.8.weight"], P["fc_layers.8.bias"]).numpy()
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=1024)
    ap.add_argument("--cpu-candidates", type=int, default=64)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import hite_amd
    import ltrdeep_twin as T

    lines = []
    say = lambda s: (lines.append(s), print(s, flush=True))  # noqa: E731
    params = np.load(os.path.join(ROOT, "tests", "golden", "ltr_deep_model.npy"))
    mats = make_matrices(np.random.default_rng(16), a.candidates)
    ctx = hite_amd.Context(0)
    model = ctx.ltr_model(params)
    ctx.ltr_deep(model, mats[:80])          # warm-up: code objects, the scratch of a full batch
    best, logits = None, None
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        logits, status = ctx.ltr_deep(model, mats)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    assert not status.any()
    say("hite_ltr_deep, %d matrices of 100 rows, batches of the default size: %.4f s host to host (best of %d) = %.0f candidates / s" %
        (a.candidates, best, a.repeat, a.candidates / best))
    ctx.profile(on=True, reset=True)
    ctx.ltr_deep(model, mats)
    prof = ctx.profile(on=False)
    stages = {k: v for k, v in prof.items() if k.startswith("ltrdeep")}
    say("device time (HIP events): " + ", ".join("%s %.3f ms / %d" % (k, v[0], v[1]) for k, v in sorted(stages.items())))
    conv_s = stages["ltrdeep_conv"][0] / 1e3
    flops = 2.0 * model_macs() * a.candidates
    say("convolutions: %.3f GFLOP per candidate needed (%.3f G multiply-adds), %.2f TFLOP/s achieved = %.1f %% of the fp32 peak of %.1f TFLOP/s "
        "(compute bound by the count: the planes of a batch, %.1f MB per candidate read and written once per layer, would take %.2f ms at 6.3 TB/s)" %
        (2e-9 * model_macs(), 1e-9 * model_macs(), flops / conv_s / 1e12, 100.0 * flops / conv_s / PEAK_FP32, PEAK_FP32 / 1e12,
         plane_bytes() / 1e6, 1e3 * plane_bytes() * a.candidates / 6.3e12))
    say("decisions at 0.5: %d LTR, %d not" % (int((logits[:, 1] > logits[:, 0]).sum()), int((logits[:, 1] <= logits[:, 0]).sum())))
    # the CPU side on the same machine
    sub = mats[:a.cpu_candidates]
    t0 = time.perf_counter()
    img, kmer, _s = T.ltr_deep_features(sub)
    t_feat = time.perf_counter() - t0
    run = torch_model(params, a.threads)
    kmer4 = kmer[:, :, None, :].astype(np.int64)
    run(img[:4].astype(np.int64), kmer4[:4])
    t0 = time.perf_counter()
    cpu_logits = run(img.astype(np.int64), kmer4)
    t_model = time.perf_counter() - t0
    say("CPU on the same machine, %d matrices: the twin's features (numpy, one process) %.3f s = %.1f / s; torch float32 on %d threads %.3f s = %.1f / s; "
        "largest |device - torch CPU| logit %.3g" % (len(sub), t_feat, len(sub) / t_feat, a.threads, t_model, len(sub) / t_model,
                                                    float(np.abs(cpu_logits - logits[:len(sub)]).max())))
    model.release()
    ctx.close()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


def plane_bytes():
    """bytes of fp32 planes a candidate's layers read and write (inputs, shortcut inputs and outputs of the six convolutions per branch)"""
    total = 0
    for c0, pixels in ((3, 100 * 200), (2, 3872)):
        for cin, cout in ((c0, 8), (8, 16), (16, 32)):
            total += 4 * pixels * ((cin + cout) + (cout + cin + cout))
    return total - 4 * (100 * 200 + 3872) * 32          # the last block's output is pooled, not stored


if __name__ == "__main__":
    main()
