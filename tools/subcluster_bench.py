#!/usr/bin/env python
"""Both routes of the sub-clustering step of generate_cons_v1 (where the reference runs `Ninja --cluster_cutoff 0.2`): the host loop
util.ninja_stand_in and the device stage hite_msa_subcluster (Context.msa_subcluster), on
  (a) the first alignments of the clusters of a synthetic C5-style library: `--families` consensus sequences of hite_amd/synth.py
      (TIR families, 150 - 3 000 bases), `--copies` copies of each, 0 - 15 % from their consensus, shuffled, through
      util.deredundant_for_LTR_v5;
  (b) one 1 500 x 4 000 alignment of unrelated rows (every row a leader: rows x leaders x columns at its worst);
  (c) one 10 000 x 4 000 alignment of unrelated rows, the largest cluster the merge forms -- the device only; the host time is an
      EXTRAPOLATION from (b) by (rows / 1 500)^2 and labelled as one.
    python tools/subcluster_bench.py [--families 6000] [--copies 8] [--out profiles/r09_msa_subcluster.txt]
The results of the two routes are compared on (a) and (b); the record gives both times and their ratio, the kernels' own time (HIP
events), and stages["seconds"] of one deredundant_for_LTR_v5 run with the switch off and one with it on."""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ("hits", "stretch", "chain", "cluster", "align_first", "subcluster", "align_second", "consensus", "redundancy")


def make(rng, n_fam, n_copy):
    from hite_amd import synth

    recs = []
    for f, fam in enumerate(synth.make_families(rng, n_fam, 0)):
        for k in range(n_copy):
            div = float(rng.uniform(0.0, 0.15))
            s = synth._mutate_copy(rng, fam["cons"], div, div / 10)
            recs.append(("fam%d_c%d" % (f, k), np.frombuffer(b"ACGT", np.uint8)[s].tobytes().decode()))
    return [recs[i] for i in rng.permutation(len(recs))]


class Recorder:
    """the context, remembering the alignments the sub-clustering step is given"""

    def __init__(self, ctx):
        self._ctx = ctx
        self.sent = None

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    def msa_subcluster(self, alignments, cutoff=0.2):
        self.sent = list(alignments)
        return self._ctx.msa_subcluster(alignments, cutoff)


def best_of(k, fn):
    out, best = None, None
    for _ in range(k):
        t0 = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, out


def kernel_ms(ctx, als):
    ctx.profile(on=True, reset=True)
    ctx.msa_subcluster(als)
    prof = ctx.profile(on=False)
    return ", ".join("%s %.3f ms / %d" % (k, v[0], v[1]) for k, v in sorted(prof.items()) if k.startswith("subcluster")) or "none"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--families", type=int, default=6000)
    ap.add_argument("--copies", type=int, default=8)
    ap.add_argument("--big-rows", type=int, default=10000)
    ap.add_argument("--commit", default=None, help="the commit the numbers are taken on (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_msa_subcluster.txt"))
    a = ap.parse_args()

    import hite_amd
    from hite_amd import util

    rng = np.random.default_rng(909)
    recs = make(rng, a.families, a.copies)
    d = tempfile.mkdtemp(prefix="subcluster_bench_")
    ctx = hite_amd.Context(0)
    rec = Recorder(ctx)
    devnull = open(os.devnull, "w")
    stderr, sys.stderr = sys.stderr, devnull
    secs = {}
    try:
        for k, mode in enumerate(("warm", "off", "gpu")):           # the first run warms code objects, scratch and the index
            lib = os.path.join(d, "lib_%s.fa" % mode)
            with open(lib, "w") as f:
                f.write("".join(">%s\n%s\n" % r for r in recs))
            st = {}
            util.deredundant_for_LTR_v5(lib, d, 1, "terminal", 0.95, 0, ctx=rec, stages=st, subcluster="gpu" if mode != "off" else "off")
            secs[mode] = (st["seconds"], util.read_fasta(lib + ".tmp.cons")[1], len(st["clusters"]))
    finally:
        sys.stderr = stderr
    als = rec.sent
    rows = [m.shape[0] for m in als]
    t_host_a, host_a = best_of(3, lambda: [util.ninja_stand_in(m) for m in als])
    t_gpu_a, gpu_a = best_of(3, lambda: ctx.msa_subcluster(als))
    k_a = kernel_ms(ctx, als)

    rb = np.random.default_rng(910)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    mb = acgt[rb.integers(0, 4, size=(1500, 4000))]
    t_host_b, host_b = best_of(1, lambda: util.ninja_stand_in(mb))
    t_gpu_b, gpu_b = best_of(3, lambda: ctx.msa_subcluster([mb]))
    k_b = kernel_ms(ctx, [mb])

    mc = acgt[rb.integers(0, 4, size=(a.big_rows, 4000))]
    t_gpu_c, gpu_c = best_of(2, lambda: ctx.msa_subcluster([mc]))
    k_c = kernel_ms(ctx, [mc])
    t_host_c = t_host_b * (a.big_rows / 1500.0) ** 2

    try:
        commit = a.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    lens = [len(s) for _n, s in recs]
    off, on = secs["off"], secs["gpu"]
    lines = [
        "sub-clustering of aligned clusters, host route (util.ninja_stand_in) and device route (hite_msa_subcluster) -- tools/subcluster_bench.py; "
        "taken on the tree above commit %s" % commit,
        "the host route is the code of the parent commit, on the same machine; the switch stays off by default",
        "(a) library: %d families x %d copies = %d sequences of %d - %d bases; %d clusters -> %d first alignments, %d rows in all, "
        "the largest %d x %d, %d bytes" % (a.families, a.copies, len(recs), min(lens), max(lens), on[2], len(als), sum(rows), max(rows),
                                            max(m.shape[1] for m in als), sum(m.size for m in als)),
        "    host %.4f s (best of 3), device %.4f s (best of 3, ONE call, copies included): host / device = %.2f; results equal: %s" %
        (t_host_a, t_gpu_a, t_host_a / t_gpu_a, host_a == gpu_a),
        "    kernels (HIP events, ms / launches): %s" % k_a,
        "(b) 1 500 x 4 000, unrelated rows (%d sub-clusters): host %.3f s (one run), device %.4f s (best of 3): host / device = %.1f; results equal: %s" %
        (len(gpu_b[0]), t_host_b, t_gpu_b, t_host_b / t_gpu_b, [host_b] == gpu_b),
        "    kernels: %s" % k_b,
        "(c) %d x 4 000, unrelated rows (%d sub-clusters): device %.3f s (best of 2); host NOT RUN: %.0f s EXTRAPOLATED from (b) by (rows / 1 500)^2: "
        "host (extrapolated) / device = %.0f" % (a.big_rows, len(gpu_c[0]), t_gpu_c, t_host_c, t_host_c / t_gpu_c),
        "    kernels: %s" % k_c,
        "deredundant_for_LTR_v5 on the library of (a), stages[\"seconds\"] (wall seconds), switch off | switch on:",
    ]
    lines += ["    %-13s %9.4f | %9.4f" % (k, off[0][k], on[0][k]) for k in STAGES]
    lines += ["    %-13s %9.4f | %9.4f" % ("total", sum(off[0].values()), sum(on[0].values())),
              "    the sub-clustering step is %.2f %% of the merge with the switch off, %.2f %% with it on; consensus libraries equal: %s" %
              (100.0 * off[0]["subcluster"] / sum(off[0].values()), 100.0 * on[0]["subcluster"] / sum(on[0].values()), off[1] == on[1]),
              "(parity with Ninja itself is unpinned: both routes are the project's leader clustering)"]
    txt = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(txt)
    sys.stdout.write(txt)
    ctx.close()


if __name__ == "__main__":
    main()
