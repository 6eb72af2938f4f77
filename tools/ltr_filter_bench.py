#!/usr/bin/env python
"""The LTR flank filter (util.ltr_flank_filter, FiLTR's step 3) and the clustering of frames under it (hite_frame_cluster,
Context.frame_cluster) on one GPU:
  (a) the three clustering calls of the step (left frames, right frames, joined frames) on a synthetic batch of `--candidates`
      candidates whose copy counts follow the C3 generator of hite_amd/synth.py (2 + Geom(0.05), capped at 100) and on a worst-case
      batch of `--worst` candidates x 100 rows of unrelated flanks: wall time of the call (packing and copies included) and the
      kernel's own time (HIP events).  The baseline is the CPU twin in its C form (tests/framecluster_twin.c) on the same host, on
      the first `--twin-candidates` / `--twin-worst` candidates of each batch, beside the device on the same subset.  cd-hit-est is
      on no machine of the project: it is not run and nothing is extrapolated to it;
  (b) the whole stage on a planted genome (hite_amd/synth.py::make_ltr_flank_genome, `--genome-mbp`): the wall seconds of every step
      and the quality -- the share of true LTR terminals kept, of terminals with homologous flanks dropped;
  (c) the share of pairs of RANDOM 100-base frames that the first rule (-c 0.8 -aS 0.3 -A 20) calls similar: the noise floor under
      FiLTR's 0.8 / 0.9 row thresholds.
    python tools/ltr_filter_bench.py [--out profiles/r11_ltr_flank_filter.txt]"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
FLANK = 100
ACGT = np.frombuffer(b"ACGT", np.uint8)


def rand_frames(rng, n):
    return [r.tobytes().decode() for r in ACGT[rng.integers(0, 4, size=(n, FLANK))]]


def related_frames(rng, n, div=0.05):
    anc = rng.integers(0, 4, size=FLANK)
    rows = np.where(rng.random((n, FLANK)) < div, rng.integers(0, 4, size=(n, FLANK)), anc)
    return [r.tobytes().decode() for r in ACGT[rows]]


def make_batch(rng, n_cand, copies=None):
    """-> [(left frames, right frames)]: two candidates in three have unrelated flanks, the others a homologous flank on one side or both"""
    out = []
    for _ in range(n_cand):
        n = copies or int(min(100, 2 + rng.geometric(0.05)))
        kind = int(rng.integers(0, 6)) if copies is None else 0
        out.append((related_frames(rng, n) if kind in (4, 5) else rand_frames(rng, n), related_frames(rng, n) if kind in (3, 5) else rand_frames(rng, n)))
    return out


def three_calls(cluster, batch, sort_kw, joined_kw):
    t = [time.perf_counter()]
    res = []
    for groups, kw in (([l for l, _r in batch], sort_kw), ([r for _l, r in batch], sort_kw), ([[a + b for a, b in zip(l, r)] for l, r in batch], joined_kw)):
        res.append(cluster(groups, **kw))
        t.append(time.perf_counter())
    return [t[k + 1] - t[k] for k in range(3)], res


def best_three(k, cluster, batch, sort_kw, joined_kw):
    best, res = None, None
    for _ in range(k):
        secs, res = three_calls(cluster, batch, sort_kw, joined_kw)
        best = secs if best is None else [min(a, b) for a, b in zip(best, secs)]
    return best, res


def kernel_ms(ctx, batch, sort_kw, joined_kw):
    ctx.profile(on=True, reset=True)
    three_calls(ctx.frame_cluster, batch, sort_kw, joined_kw)
    prof = ctx.profile(on=False)
    return ", ".join("%s %.3f ms / %d" % (k, v[0], v[1]) for k, v in sorted(prof.items()) if k.startswith("framecluster")) or "none"


def fmt(secs):
    return "left %.4f + right %.4f + joined %.4f = %.4f s" % (secs[0], secs[1], secs[2], sum(secs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=5000)
    ap.add_argument("--twin-candidates", type=int, default=300)
    ap.add_argument("--worst", type=int, default=1000)
    ap.add_argument("--twin-worst", type=int, default=10)
    ap.add_argument("--genome-mbp", type=float, default=100.0)
    ap.add_argument("--families", type=int, default=400, help="planted families of each of the four kinds")
    ap.add_argument("--noise-pairs", type=int, default=200000)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_ltr_flank_filter.txt"))
    a = ap.parse_args()

    import framecluster_twin as T
    from hite_amd import synth, util

    sort_kw, joined_kw = util.LTR_SORT_OPTIONS, util.LTR_JOINED_OPTIONS
    rng = np.random.default_rng(1111)
    ctx = util.get_ctx()
    lines = []
    try:
        commit = a.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    lines.append("LTR flank filter (util.ltr_flank_filter, FiLTR step 3) and the clustering of frames under it (hite_frame_cluster) -- "
                 "tools/ltr_filter_bench.py; taken on the tree above commit %s, one MI355X" % commit)
    lines.append("baseline: the CPU twin in its C form (tests/framecluster_twin.c, gcc -O2, one thread) on the same host.  cd-hit-est is on no "
                 "machine of the project: NOT RUN, nothing extrapolated to it")
    # ---- (a) the three clustering calls ------------------------------------------------------------------------------------------
    three_calls(ctx.frame_cluster, make_batch(rng, 50), sort_kw, joined_kw)      # code objects, scratch
    for label, batch, n_twin in (("C3-style copy counts", make_batch(rng, a.candidates), a.twin_candidates),
                                 ("worst case, 100 rows of unrelated flanks", make_batch(rng, a.worst, copies=100), a.twin_worst)):
        rows = [len(l) for l, _r in batch]
        t_gpu, res = best_three(3, ctx.frame_cluster, batch, sort_kw, joined_kw)
        sub = batch[:n_twin]
        t_twin, res_twin = three_calls(T.frame_cluster, sub, sort_kw, joined_kw)
        t_sub, res_sub = best_three(3, ctx.frame_cluster, sub, sort_kw, joined_kw)
        lines += ["(a) %s: %d candidates, %d rows in all (%d - %d per candidate), %d pairs per call" %
                  (label, len(batch), sum(rows), min(rows), max(rows), sum(n * (n - 1) // 2 for n in rows)),
                  "    device, whole batch, three calls (best of 3 each, packing and copies included): %s" % fmt(t_gpu),
                  "    kernel alone (HIP events, ms / launches, the three calls together): %s" % kernel_ms(ctx, batch, sort_kw, joined_kw),
                  "    first %d candidates (%d rows): twin %s (one run); device %s; twin / device = %.1f; results equal: %s" %
                  (len(sub), sum(rows[:n_twin]), fmt(t_twin), fmt(t_sub), sum(t_twin) / sum(t_sub), res_twin == res_sub),
                  "    (the twin compares a row with the representatives only and stops at the first match; the device fills the whole pair "
                  "matrix of a group: %d pairs against the twin's share of them)" % sum(n * (n - 1) // 2 for n in rows[:n_twin])]
    # ---- (c) the noise floor -----------------------------------------------------------------------------------------------------
    pairs = [rand_frames(rng, 2) for _ in range(a.noise_pairs)]
    t0 = time.perf_counter()
    res = ctx.frame_cluster(pairs, **sort_kw)
    dt = time.perf_counter() - t0
    hit = sum(1 for cl in res if len(cl) == 1)
    lines.append("(c) noise floor: %d of %d pairs of random %d-base frames (%.4f %%) are similar under -c 0.8 -aS 0.3 -A 20, both strands "
                 "(%.3f s on the device)" % (hit, len(pairs), FLANK, 100.0 * hit / len(pairs), dt))
    # ---- (b) the whole stage on a planted genome ----------------------------------------------------------------------------------
    plan = []
    for _ in range(a.families):
        plan += [("ltr", int(min(100, 2 + rng.geometric(0.05)))), ("inner", int(min(100, 2 + rng.geometric(0.05)))),
                 ("left" if rng.integers(0, 2) else "right", int(min(100, 2 + rng.geometric(0.05)))), ("ltr", 1)]
    t0 = time.perf_counter()
    g = synth.make_ltr_flank_genome(plan, genome_bp=int(a.genome_mbp * 1e6), chrom_bp=min(50_000_000, int(a.genome_mbp * 1e6)), seed=1112)
    d = tempfile.mkdtemp(prefix="ltr_filter_bench_")
    ref = os.path.join(d, "genome.fa")
    util.store_fasta({"chr_%d" % k: c for k, c in enumerate(g["contigs"])}, ref)
    t_make = time.perf_counter() - t0
    t0 = time.perf_counter()
    util.set_reference(ref)
    t_pack = time.perf_counter() - t0
    util.ltr_flank_filter(dict(list(g["terminals"].items())[:40]), ref, FLANK, ctx=ctx)          # warm: the index, code objects
    seconds = {}
    t0 = time.perf_counter()
    table, high = util.ltr_flank_filter(g["terminals"], ref, FLANK, ctx=ctx, seconds=seconds)
    t_stage = time.perf_counter() - t0
    kinds = {}
    for n in g["names"]:
        k = "single" if g["copies"][n] == 1 else ("one flank" if g["kind"][n] in ("left", "right") else g["kind"][n])
        kinds.setdefault(k, []).append(table[n])
    lines += ["(b) whole stage: %d terminal sequences (%d planted copies) on a %.0f Mbp genome (built in %.1f s, read and packed in %.1f s; "
              "neither is part of the stage)" % (len(g["names"]), sum(g["copies"].values()), a.genome_mbp, t_make, t_pack),
              "    ltr_flank_filter: %.3f s wall; steps (wall seconds): %s" % (t_stage, ", ".join("%s %.3f" % kv for kv in seconds.items())),
              "    (the alignments come down after star_msa and go up again for ltr_both_ends, the frames come down and go up again for the "
              "clustering and the vote: their cost is inside msa, both_ends, cluster_* and frame_vote)"]
    for k in ("ltr", "inner", "one flank", "single"):
        v = kinds.get(k, [])
        kept = sum(1 for r in v if r[0])
        by = {}
        for r in v:
            by[r[2]] = by.get(r[2], 0) + 1
        lines.append("    %-9s %5d families: kept %5d (%.2f %%), by step %s" % (k, len(v), kept, 100.0 * kept / max(1, len(v)),
                                                                              ", ".join("%s %d" % (s, c) for s, c in sorted(by.items(), key=str))))
    lines.append("    high-copy matrices handed on: %d" % len(high))
    txt = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(txt)
    sys.stdout.write(txt)
    ctx.close()


if __name__ == "__main__":
    main()
