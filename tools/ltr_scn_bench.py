#!/usr/bin/env python
"""FiLTR's steps 1 and 2 on the lines of a `.scn` candidate table (util.ltr_scn_filter) and the pairwise search under them
(hite_pair_hsps, Context.pair_hsps) on one GPU, on a planted genome (hite_amd/synth.py::make_ltr_element_genome, `--elements` of
every kind):
  (a) the decisions against the planted truth, per kind;
  (b) the wall seconds of the three steps (recombination, potential_lines, flank_align), the searches through the device;
  (c) the pairs per second of the primitive on the pairs of each step (wall time of Context.pair_hsps, packing and copies included, best
      of 3, and the kernel's own time from HIP events) next to the CPU twin in its C form (tests/pairhsp_twin.c, one thread) on the
      same host on the first `--twin-pairs` pairs of the step, with the device on the same subset.  blastn is on no machine of the
      project: it is not run and nothing is extrapolated to it.
    python tools/ltr_scn_bench.py [--out profiles/r12_ltr_scn_filter.txt]"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def best_of(k, fn, *args, **kw):
    best, res = None, None
    for _ in range(k):
        t0 = time.perf_counter()
        res = fn(*args, **kw)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elements", type=int, default=400, help="planted elements of each of the seven kinds")
    ap.add_argument("--twin-pairs", type=int, default=300)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_ltr_scn_filter.txt"))
    a = ap.parse_args()

    import pairhsp_twin as T
    from hite_amd import synth, util

    ctx = util.get_ctx()
    try:
        commit = a.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    lines = ["FiLTR steps 1 and 2 on the `.scn` candidate table (util.ltr_scn_filter) and the pairwise search under them (hite_pair_hsps) -- "
             "tools/ltr_scn_bench.py; taken on the tree above commit %s, one MI355X" % commit,
             "baseline: the CPU twin in its C form (tests/pairhsp_twin.c, gcc -O2, one thread) on the same host.  blastn is on no machine of "
             "the project: NOT RUN, nothing extrapolated to it"]
    t0 = time.perf_counter()
    g = synth.make_ltr_element_genome([(k, a.elements) for k in synth.LTR_ELEMENT_KINDS], seed=1201)
    d = tempfile.mkdtemp(prefix="ltr_scn_bench_")
    scn, ref = os.path.join(d, "in.scn"), os.path.join(d, "genome.fa")
    with open(scn, "w") as f:
        f.write(g["scn"])
    util.store_fasta(g["contigs"], ref)
    t_make = time.perf_counter() - t0
    n_bp = sum(len(s) for s in g["contigs"].values())

    # the pairs of every step, as the functions send them, recorded on a first (warming) run
    calls = []

    def recording(seqs, pairs, diag_min=None):
        calls.append((seqs, pairs, diag_min))
        return ctx.pair_hsps(seqs, pairs, diag_min)

    util.ltr_scn_filter(scn, ref, os.path.join(d, "warm"), hsps=recording)
    seconds = {}
    t0 = time.perf_counter()
    final, dirty, terminals = util.ltr_scn_filter(scn, ref, os.path.join(d, "out"), ctx=ctx, seconds=seconds)
    t_all = time.perf_counter() - t0
    recomb_lines = open(os.path.join(d, "out", "remove_recomb.scn")).read().splitlines()
    final_lines = open(final).read().splitlines()
    table, wrong = synth.ltr_element_decisions(g["truth"], recomb_lines, final_lines, dirty)
    lines += ["planted genome: %d elements of each of %d kinds (%d lines, %d of them repeated) on %.1f Mbp in %d chromosomes (built in %.1f s; "
              "not part of the stage)" % (a.elements, len(synth.LTR_ELEMENT_KINDS), g["scn"].count("\n") - 1, a.elements, n_bp / 1e6,
                                          len(g["contigs"]), t_make),
              "(a) decisions as planted, per kind (as planted / elements): " +
              ", ".join("%s %d / %d" % (k, v[0], v[1]) for k, v in sorted(table.items())) + "; %d of %d elements not as planted" % (len(wrong), len(g["truth"])),
              "    lines: %d read, %d after step 1 (remove_recomb.scn), %d after step 2 (filter_terminal_align.scn), %d in dirty_dicts, %d left terminals" %
              (len(util.read_scn(scn, None, remove_dup=True)[1]), len(recomb_lines), len(final_lines), len(dirty), len(terminals)),
              "(b) ltr_scn_filter: %.3f s wall; steps (wall seconds, reading the genome and the table is `read`): %s" %
              (t_all, ", ".join("%s %.3f" % kv for kv in seconds.items()))]
    for label, (seqs, pairs, diag_min) in zip(("recombination (left terminal x internal)", "potential_lines (internal x itself, diag_min 500)",
                                               "flank_align (left terminal +- 50 x right terminal +- 50)"), calls):
        cells = sum((p[2] - p[1]) for p in pairs)
        t_gpu, res = best_of(3, ctx.pair_hsps, seqs, pairs, diag_min)
        ctx.profile(on=True, reset=True)
        ctx.pair_hsps(seqs, pairs, diag_min)
        prof = ctx.profile(on=False)
        kern = ", ".join("%s %.3f ms / %d" % (k, v[0], v[1]) for k, v in sorted(prof.items()) if k.startswith("pairhsp")) or "none"
        sub = pairs[:a.twin_pairs]
        t_twin, res_twin = best_of(1, T.pair_hsps, seqs, sub, diag_min)
        t_sub, res_sub = best_of(3, ctx.pair_hsps, seqs, sub, diag_min)
        lines += ["(c) %s: %d pairs, %d HSPs, %d refused, %.0f rows of Q on average" %
                  (label, len(pairs), sum(len(r) for r in res if r is not None), sum(r is None for r in res), cells / max(1, len(pairs))),
                  "    device, all pairs (best of 3, packing and copies included): %.4f s -> %.0f pairs/s; kernel alone (HIP events, ms / launches): %s" %
                  (t_gpu, len(pairs) / t_gpu, kern),
                  "    first %d pairs: twin %.4f s -> %.0f pairs/s (one run); device %.4f s -> %.0f pairs/s; twin / device = %.1f; results equal: %s" %
                  (len(sub), t_twin, len(sub) / t_twin, t_sub, len(sub) / t_sub, t_twin / t_sub, res_twin == res_sub)]
    text = "\n".join(lines) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
