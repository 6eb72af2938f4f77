#!/usr/bin/env python
"""The genome annotation (hite_annotate, Context.annotate) on one GPU, on a synthetic genome of random sequence with planted copies of
a random library (entries of 300 .. 6 000 bases; per entry two copies at each of 0 / 5 / 10 / 15 / 20 / 25 % substitutions with a
tenth as many indels, hite_amd.synth._mutate_copy, on either strand; chromosomes of 25 Mbp):
  (a) the wall time of the call host to host (the texts, the pieces, copies and the resolve included, best of 2) and ms per Gbp, the
      counters of the call;
  (b) recall (planted copies covered for >= 90 % of their length by records of their own entry and strand) and base-level precision
      (bases under records of an entry that lie inside a planted copy of that entry) by divergence, recall by copy length;
  (c) the time of every step from HIP events (hite_profile_*) and which one dominates;
  (d) the CPU twin in its C form (tests/annotate_twin.c, one thread) on the first `--twin-mbp` of the same genome on the same host,
      with the device on the same piece.  RepeatMasker is on no machine of the project: it is not run and nothing is extrapolated.
    python tools/annotate_bench.py [--mbp 100] [--entries 1000] [--twin-mbp 4] [--out profiles/r15_annotate.txt]"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
CHROM = 25_000_000
DIVS = (0.0, 0.05, 0.10, 0.15, 0.20, 0.25)
LENGTHS = ((300, 600), (600, 1200), (1200, 2500), (2500, 6001))


def make_genome(mbp, n_entries, seed=15):
    """-> ([chromosome bytes], [entry bytes], truth rows (chromosome, begin, end, entry, strand, divergence)); a copy per slot, the
    slots of a chromosome filled in a random order of (entry, divergence, strand)"""
    from hite_amd import synth

    rng = np.random.default_rng(seed)
    lib = [rng.integers(0, 4, size=int(rng.integers(300, 6001)), dtype=np.uint8) for _ in range(n_entries)]
    plan = [(e, d, k) for e in range(n_entries) for d in DIVS for k in range(2)]
    plan = [plan[i] for i in rng.permutation(len(plan))]
    total = int(mbp * 1e6)
    slot = max(total // len(plan), 8000)
    chroms, truth, at = [], [], 0
    for c0 in range(0, total, CHROM):
        n = min(CHROM, total - c0)
        g = ACGT[rng.integers(0, 4, size=n, dtype=np.uint8)]
        for s0 in range(0, n - slot + 1, slot):
            if at == len(plan):
                break
            e, d, k = plan[at]
            at += 1
            c = synth._mutate_copy(rng, lib[e], d, d / 10)
            strand = int(rng.integers(0, 2))
            if strand:
                c = (3 - c[::-1]).astype(np.uint8)
            pos = s0 + int(rng.integers(500, slot - len(c) - 500))
            g[pos:pos + len(c)] = ACGT[c]
            truth.append((len(chroms), pos, pos + len(c), e, strand, d))
        chroms.append(g.tobytes())
    return chroms, [ACGT[e].tobytes() for e in lib], truth


def best_of(k, fn, *args, **kw):
    best, res = None, None
    for _ in range(k):
        t0 = time.perf_counter()
        res = fn(*args, **kw)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, res


def accuracy(recs, truth, lib, chrom_lens):
    """-> lines of the recall / precision tables"""
    by_key = {}
    for r in recs:
        by_key.setdefault((r[0], r[3], r[4]), []).append((r[1], r[2]))
    found = {}
    for c, b, e, ent, strand, d in truth:
        m = np.zeros(e - b, dtype=bool)
        for gs, ge in by_key.get((c, ent, strand), ()):
            if ge > b and gs < e:
                m[max(gs, b) - b:min(ge, e) - b] = True
        found[(c, b)] = 10 * int(m.sum()) >= 9 * (e - b)
    # base-level precision per divergence: the bases of a record that lie inside a planted copy of its entry and strand, the record
    # counted under the divergence of the copy it overlaps most (a record that overlaps none counts under "none")
    spans = {}
    for c, b, e, ent, strand, d in truth:
        spans.setdefault((c, ent, strand), []).append((b, e, d))
    prec = {d: [0, 0] for d in DIVS + ("none",)}
    for r in recs:
        best, inside = "none", 0
        for b, e, d in spans.get((r[0], r[3], r[4]), ()):
            ov = min(r[2], e) - max(r[1], b)
            if ov > 0:
                if ov > inside:
                    best = d
                inside += ov
        prec[best][0] += min(inside, r[2] - r[1])
        prec[best][1] += r[2] - r[1]
    n_none = sum(1 for r in recs if not any(min(r[2], e) > max(r[1], b) for b, e, _d in spans.get((r[0], r[3], r[4]), ())))
    lines = ["(b) recall = planted copies covered >= 90 %% by records of their entry and strand; precision = record bases inside a planted copy of "
             "the record's entry and strand (records: %d, of these %d under no planted copy of their entry and strand)" % (len(recs), n_none),
             "    divergence   copies   found   recall   record bases   precision"]
    for d in DIVS:
        rows = [t for t in truth if t[5] == d]
        n = sum(found[(t[0], t[1])] for t in rows)
        lines.append("    %8.0f %% %8d %7d %7.1f %% %14d %9.2f %%" % (100 * d, len(rows), n, 100.0 * n / max(len(rows), 1), prec[d][1],
                                                                     100.0 * prec[d][0] / max(prec[d][1], 1)))
    lines.append("    recall by entry length (rows) and divergence (columns " + " ".join("%.0f %%" % (100 * d) for d in DIVS) + "):")
    for lo, hi in LENGTHS:
        cells = []
        for d in DIVS:
            rows = [t for t in truth if t[5] == d and lo <= len(lib[t[3]]) < hi]
            cells.append("%5.1f" % (100.0 * sum(found[(t[0], t[1])] for t in rows) / max(len(rows), 1)))
        lines.append("    %5d .. %5d  " % (lo, hi - 1) + "  ".join(cells))
    return lines


def bench(a):
    import annotate_twin as AT
    import hite_amd

    try:
        commit = a.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    t0 = time.perf_counter()
    chroms, lib, truth = make_genome(a.mbp, a.entries)
    t_make = time.perf_counter() - t0
    n_bp = sum(len(c) for c in chroms)
    ctx = hite_amd.Context(0)
    lines = ["genome annotation (hite_annotate, Context.annotate) -- tools/annotate_bench.py; taken on the tree above commit %s, one MI355X" % commit,
             "constants: word 13, MAX_OCC %d, GAP %d, MIN_HITS %d, MAX_SPAN %d, EDGE %d, MAX_REDO %d, PIECE 2^24, OVERLAP 2^16, MAX_LIB_LEN %d" %
             (AT.MAX_OCC, AT.GAP, AT.MIN_HITS, AT.MAX_SPAN, AT.EDGE, AT.MAX_REDO, AT.MAX_LIB_LEN),
             "baseline: the CPU twin in its C form (tests/annotate_twin.c, gcc -O2, one thread) on the same host.  RepeatMasker is on no machine of "
             "the project: NOT RUN, nothing extrapolated to it; there is no earlier time of this stage to compare with",
             "genome: %.1f Mbp of random sequence in %d chromosomes, %d planted copies of %d entries (%.2f Mbp of library; built in %.1f s, not part "
             "of the stage)" % (n_bp / 1e6, len(chroms), len(truth), len(lib), sum(map(len, lib)) / 1e6, t_make)]
    ctx.annotate([chroms[0][:200000]], lib[:10])          # warm: code objects, the first allocations
    st = {}
    t_gpu, (recs, _status) = best_of(2, ctx.annotate, chroms, lib, stats=st)
    lines += ["(a) device, whole genome (best of 2, host to host): %.3f s wall -> %.0f ms per Gbp" % (t_gpu, t_gpu * 1e3 / (n_bp / 1e9)),
              "    counters: " + ", ".join("%s %d" % kv for kv in st.items())]
    lines += accuracy(recs.tolist(), truth, lib, [len(c) for c in chroms])
    ctx.profile(on=True, reset=True)
    ctx.annotate(chroms, lib)
    prof = ctx.profile(on=False)
    steps = [(k, v) for k, v in prof.items() if k.startswith("annot")]
    t_steps = sum(v[0] for _k, v in steps)
    top = max(steps, key=lambda kv: kv[1][0])
    lines += ["(c) steps of one call from HIP events (ms / launches; annot_table holds its sort, annot_runs the sorts of the hits): " +
              ", ".join("%s %.3f / %d" % (k, v[0], v[1]) for k, v in steps),
              "    all steps %.3f ms -> %.1f ms per Gbp on the device; %s dominates (%.0f %% of the device time); the rest of the wall time is the "
              "host (the texts, joining the pieces, copies, allocations, the resolve)" % (t_steps, t_steps / (n_bp / 1e9), top[0],
                                                                                        100.0 * top[1][0] / max(t_steps, 1e-9))]
    piece = [chroms[0][:int(a.twin_mbp * 1e6)]]
    st_t, st_g = {}, {}
    t_twin, (r_twin, _s) = best_of(1, AT.annotate, piece, lib, stats=st_t)
    t_sub, (r_sub, _s) = best_of(2, ctx.annotate, piece, lib, stats=st_g)
    lines += ["(d) first %.1f Mbp: twin %.3f s (one run) -> %.0f ms per Gbp; device %.4f s -> %.0f ms per Gbp; twin / device = %.1f; results equal: %s" %
              (len(piece[0]) / 1e6, t_twin, t_twin * 1e3 / (len(piece[0]) / 1e9), t_sub, t_sub * 1e3 / (len(piece[0]) / 1e9), t_twin / t_sub,
               r_twin == [tuple(r) for r in r_sub.tolist()] and st_t == st_g)]
    ctx.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbp", type=float, default=100.0)
    ap.add_argument("--entries", type=int, default=1000)
    ap.add_argument("--twin-mbp", type=float, default=4.0)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    text = "\n".join(bench(a)) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
