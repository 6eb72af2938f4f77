#!/usr/bin/env python
"""The LTR candidate scan (hite_ltr_scan, Context.ltr_scan) on one GPU, on a synthetic genome of planted elements in random sequence
(terminals of 150 .. 1 200 bases, the second copy 1 .. 8 % diverged by substitutions, internal sequences of 1 500 .. 6 000 bases, one
element per 125 kb, chromosomes of 25 Mbp):
  (a) the wall time of the call (packing and copies included, best of 3) and ms per Gbp, the counters of the call, the planted
      elements found at exactly their place;
  (b) the time of every step from HIP events (hite_profile_*);
  (c) the CPU twin in its C form (tests/ltrscan_twin.c, one thread) on the first `--twin-mbp` of the same genome on the same host, with
      the device on the same piece.  LtrDetector, LTR_harvest and LTR_FINDER are on no machine of the project: they are not run and
      nothing is extrapolated to them.
`--recall` needs no GPU: the twin's recall of single planted pairs by identity x terminal length (substitutions only), 30 genomes of
8 kb per cell, a pair counting as found when one record covers 80 % of either terminal.
    python tools/ltr_scan_bench.py [--mbp 100] [--out FILE]        python tools/ltr_scan_bench.py --recall [--out FILE]"""
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
SLOT = 125_000


def make_genome(mbp, seed=13):
    """-> ([chromosome bytes], [(chromosome, ls, le, rs, re)] of the planted elements)"""
    rng = np.random.default_rng(seed)
    total = int(mbp * 1e6)
    chroms, places = [], []
    for c0 in range(0, total, CHROM):
        n = min(CHROM, total - c0)
        g = ACGT[rng.integers(0, 4, size=n, dtype=np.uint8)]
        for s0 in range(0, n - SLOT + 1, SLOT):
            term = rng.integers(0, 4, size=int(rng.integers(150, 1201)), dtype=np.uint8)
            right = term.copy()
            m = rng.random(len(term)) < float(rng.uniform(0.01, 0.08))
            m[:20] = m[-20:] = False
            right[m] = (right[m] + rng.integers(1, 4, size=int(m.sum()), dtype=np.uint8)) & 3
            # the bases next to the two copies come from disjoint alphabets: an alignment ends at the boundary
            ga, gb = rng.integers(0, 2, size=(2, 12), dtype=np.uint8), rng.integers(2, 4, size=(2, 12), dtype=np.uint8)
            internal = rng.integers(0, 4, size=int(rng.integers(1500, 6001)), dtype=np.uint8)
            unit = np.concatenate([ga[0], term, ga[1], internal, gb[0], right, gb[1]])
            pos = s0 + int(rng.integers(1000, SLOT - len(unit) - 1000))
            g[pos:pos + len(unit)] = ACGT[unit]
            ls = pos + 12
            rs = ls + len(term) + 12 + len(internal) + 12
            places.append((len(chroms), ls, ls + len(term), rs, rs + len(right)))
        chroms.append(g.tobytes())
    return chroms, places


def best_of(k, fn, *args, **kw):
    best, res = None, None
    for _ in range(k):
        t0 = time.perf_counter()
        res = fn(*args, **kw)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, res


def recall_table(trials=30):
    import ltrscan_twin as LT

    lengths, idents = (100, 150, 200, 400, 800), (100, 95, 90, 85, 80)
    lines = ["recall of the twin (tests/ltrscan_twin.c) on single planted pairs, substitutions only, default limits (400 / 22 000 / 100 / 6 000 / 85): "
             "pairs found of %d, by identity of the second copy (rows) x terminal length (columns); found = one record covers 80 %% of "
             "either terminal" % trials,
             "identity  " + "".join("%8d" % n for n in lengths)]
    for ident in idents:
        row = []
        for n in lengths:
            found = 0
            for t in range(trials):
                rng = np.random.default_rng(100000 * ident + 100 * n + t)
                term = rng.integers(0, 4, size=n, dtype=np.uint8)
                right = term.copy()
                k = int(round(n * (100 - ident) / 100.0))
                at = rng.choice(n, size=k, replace=False)
                right[at] = (right[at] + rng.integers(1, 4, size=k, dtype=np.uint8)) & 3
                parts = [rng.integers(0, 4, size=3000, dtype=np.uint8), term, rng.integers(0, 4, size=1500, dtype=np.uint8), right,
                         rng.integers(0, 4, size=3000, dtype=np.uint8)]
                ls, rs = 3000, 3000 + n + 1500
                for r in LT.scan([ACGT[np.concatenate(parts)].tobytes()]):
                    left = min(r[2], ls + n) - max(r[1], ls)
                    rght = min(r[4], rs + n) - max(r[3], rs)
                    if left >= 0.8 * n and rght >= 0.8 * n:
                        found += 1
                        break
            row.append(found)
        lines.append("%6d %%  " % ident + "".join("%8d" % v for v in row))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbp", type=float, default=100.0)
    ap.add_argument("--twin-mbp", type=float, default=10.0)
    ap.add_argument("--recall", action="store_true", help="the twin's recall table only (no GPU)")
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.recall:
        lines = recall_table()
    else:
        lines = bench(a)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    sys.stdout.write(text)


def bench(a):
    import hite_amd
    import ltrscan_twin as LT

    try:
        commit = a.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    t0 = time.perf_counter()
    chroms, places = make_genome(a.mbp)
    t_make = time.perf_counter() - t0
    n_bp = sum(len(c) for c in chroms)
    ctx = hite_amd.Context(0)
    lines = ["LTR candidate scan (hite_ltr_scan, Context.ltr_scan) -- tools/ltr_scan_bench.py; taken on the tree above commit %s, one MI355X" % commit,
             "baseline: the CPU twin in its C form (tests/ltrscan_twin.c, gcc -O2, one thread) on the same host.  LtrDetector, LTR_harvest and "
             "LTR_FINDER are on no machine of the project: NOT RUN, nothing extrapolated to them",
             "genome: %.1f Mbp of random sequence in %d chromosomes, %d planted elements (built in %.1f s; not part of the stage)" %
             (n_bp / 1e6, len(chroms), len(places), t_make)]
    ctx.ltr_scan(chroms[:1])          # warm: code objects, the first allocations
    st = {}
    t_gpu, recs = best_of(3, ctx.ltr_scan, chroms, stats=st)
    have = {tuple(r[:5]) for r in recs.tolist()}
    lines += ["(a) device, whole genome (best of 3, packing and copies included): %.3f s wall -> %.0f ms per Gbp" % (t_gpu, t_gpu * 1e3 / (n_bp / 1e9)),
              "    counters: " + ", ".join("%s %d" % kv for kv in st.items()),
              "    planted elements with a record at exactly their place: %d of %d; records: %d" % (sum(p in have for p in places), len(places), len(recs))]
    ctx.profile(on=True, reset=True)
    ctx.ltr_scan(chroms)
    prof = ctx.profile(on=False)
    steps = [(k, v) for k, v in prof.items() if k.startswith("ltrscan")]
    t_steps = sum(v[0] for _k, v in steps)
    lines += ["(b) steps of one call from HIP events (ms / launches of the step; the two runs steps hold the sort of the hits and the scan): " +
              ", ".join("%s %.3f / %d" % (k, v[0], v[1]) for k, v in steps),
              "    all steps %.3f ms -> %.1f ms per Gbp on the device; the rest of the wall time is the host (joining the sequences, copies, "
              "allocations, filters)" % (t_steps, t_steps / (n_bp / 1e9))]
    piece, need = [], int(a.twin_mbp * 1e6)
    for c in chroms:
        if need <= 0:
            break
        piece.append(c[:need])
        need -= len(piece[-1])
    p_bp = sum(len(c) for c in piece)
    st_t, st_g = {}, {}
    t_twin, r_twin = best_of(1, LT.scan, piece, stats=st_t)
    t_sub, r_sub = best_of(3, ctx.ltr_scan, piece, stats=st_g)
    lines += ["(c) first %.1f Mbp: twin %.3f s (one run) -> %.0f ms per Gbp; device %.4f s -> %.0f ms per Gbp; twin / device = %.1f; results equal: %s" %
              (p_bp / 1e6, t_twin, t_twin * 1e3 / (p_bp / 1e9), t_sub, t_sub * 1e3 / (p_bp / 1e9), t_twin / t_sub,
               r_twin == [tuple(r) for r in r_sub.tolist()] and st_t == st_g)]
    ctx.close()
    return lines


if __name__ == "__main__":
    main()
