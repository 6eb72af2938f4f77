#!/usr/bin/env python
"""Throughput of the Helitron candidate scan (hite_helitron_scan, where the reference runs HelitronScanner) and its recall on planted
elements:
    python tools/helitron_bench.py [--mbp 100] [--families 200] [--out profiles/r10_helitron_scan.txt]
Input: the flanked repeats of the C2 configuration (bench.py: 100 Mbp, 500 TIR families, 10 candidates a family, each cut from a
planted copy with its ends moved by up to 30 bases), as the coarse stage hands them to the Helitron stage.  Into the candidates of the
first `--families` families a Helitron is planted: an LCV-matching head over the bases from 50 on and a tail over the bases up to 50
before the end (one head line and one tail line of the tool's lists per family, made concrete per candidate), so the planted element
is the candidate without 50 bases either side and its length follows the family's (100 .. 3 000 bases).
Reports: the wall time of Context.helitron_scan on all candidates (best of 3) and its kernels (hite_profile_*), anchors per second,
the time of the scoring code compiled for the host (tests/helitron_host.py) on the same input in 16 processes, and per length class
of the planted elements the share that has a record with both ends within 3 bases (recall) and, among the records of those
candidates, the share that is such a record (precision).  The tool itself (HelitronScanner.jar) was not run: no time of it is known
beyond the 30 minutes per 50 kb part that the reference grants it."""
import argparse
import multiprocessing
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CLASSES = ((0, 200), (200, 500), (500, 1000), (1000, 2000), (2000, 4000))
_HOST = {}


def _host_part(job):
    import helitron_host as HH
    from hite_amd import util

    workdir, seqs, head, tail = job
    os.environ["HITE_HOST_THREADS"] = "1"
    lib = HH.build(workdir)          # (compiled by the parent: the library is only loaded here)
    return HH.scan(lib, seqs, util.parse_lcvs(head, "head"), util.parse_lcvs(tail, "tail"))


def main():
    import helitron_cases as HC
    import helitron_host as HH
    from hite_amd import synth, util

    ap = argparse.ArgumentParser()
    ap.add_argument("--mbp", type=int, default=100)
    ap.add_argument("--families", type=int, default=200)
    ap.add_argument("--processes", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_helitron_scan.txt"))
    a = ap.parse_args()
    head, tail = HC.lcv_lists()
    hp, tp = util.parse_lcvs(head, "head"), util.parse_lcvs(tail, "tail")
    w = synth.make_workload(genome_bp=a.mbp * 1_000_000, n_tir=5 * a.mbp, n_ltr=0, cands_per_family=10, seed=20250927 + 3)
    off = w["cand_off"]
    seqs = [bytes(w["cands"][off[c]:off[c + 1]]).decode() for c in range(len(off) - 1)]
    rng = np.random.default_rng(10)
    fams = sorted(set(int(f) for f in w["family"]))[:a.families]
    lines = {f: (head[int(rng.integers(0, len(head)))], tail[int(rng.integers(0, len(tail)))]) for f in fams}
    truth = {}                     # candidate -> (start, end)
    for c, f in enumerate(w["family"]):
        if int(f) not in lines:
            continue
        h, t = HC.head_site(rng, lines[int(f)][0]), HC.tail_site(rng, lines[int(f)][1])
        s = seqs[c]
        if len(s) < 100 + len(h) + len(t):
            continue
        seqs[c] = s[:50] + h + s[50 + len(h):len(s) - 50 - len(t)] + t + s[len(s) - 50:]
        truth[c] = (50, len(s) - 50)
    n_bases = sum(len(s) for s in seqs)

    # the host form first: no process may fork once the GPU is open
    workdir = tempfile.mkdtemp(prefix="helitron_bench_")
    HH.build(workdir)
    parts = [(workdir, seqs[k::a.processes], head, tail) for k in range(a.processes)]
    t0 = time.perf_counter()
    with multiprocessing.Pool(a.processes) as pool:
        host_rec = pool.map(_host_part, parts)
    host_s = time.perf_counter() - t0

    import hite_amd

    ctx = hite_amd.Context(0)
    ctx.helitron_scan(seqs[:50], hp, tp)            # warm-up: the code objects load
    best, rec, stats = None, None, None
    for _ in range(3):
        st = {}
        t0 = time.perf_counter()
        rec = ctx.helitron_scan(seqs, hp, tp, stats=st)
        dt = time.perf_counter() - t0
        if best is None or dt < best:
            best, stats = dt, st
    ctx.profile(on=True, reset=True)
    ctx.helitron_scan(seqs, hp, tp)
    kernels = {k: v for k, v in ctx.profile(on=False).items() if k.startswith("heli_")}
    same = sum(len(r) for r in host_rec) == len(rec) and all(
        np.array_equal(r[:, 1:], rec[np.isin(rec[:, 0], np.arange(k, len(seqs), a.processes))][:, 1:]) for k, r in enumerate(host_rec))

    by_cand = {}
    for r in rec.tolist():
        by_cand.setdefault(r[0], []).append(r)
    cells = {c: [0, 0, 0, 0] for c in CLASSES}         # planted, recalled, records in planted candidates, exact records
    for c, (s, e) in truth.items():
        cl = [x for x in CLASSES if x[0] <= e - s < x[1]][0]
        rs = by_cand.get(c, [])
        good = [r for r in rs if r[3] == 0 and abs(r[1] - s) <= 3 and abs(r[2] - e) <= 3]
        cells[cl][0] += 1
        cells[cl][1] += bool(good)
        cells[cl][2] += len(rs)
        cells[cl][3] += len(good)
    out = []
    out.append("Helitron candidate scan: tools/helitron_bench.py --mbp %d --families %d" % (a.mbp, a.families))
    out.append("input: %d flanked repeats of the C2 configuration, %d bases; the tool's lists (%d head, %d tail lines), thresholds 1, lengths 200 .. 20000"
               % (len(seqs), n_bases, len(head), len(tail)))
    out.append("scan (Context.helitron_scan, host to host, best of 3): %.4f s; anchors %d (%.3g per second), heads %d, tails %d, records %d"
               % (best, stats["anchors"], stats["anchors"] / best, stats["heads"], stats["tails"], stats["pairs"]))
    for k, (ms, n) in sorted(kernels.items()):
        out.append("  %-22s %8.3f ms in %d timed group(s)" % (k, ms, n))
    out.append("scoring code compiled for the host (tests/helitron_host.py), %d processes: %.3f s (%.3g anchors per second); records equal the GPU's: %s"
               % (a.processes, host_s, stats["anchors"] / host_s, same))
    out.append("HelitronScanner.jar itself was not run (no java, no source of its scan classes): its own time is not measured; the reference grants it "
               "30 minutes per 50 kb part")
    out.append("planted elements (one candidate each, %d families): element length | planted | recalled (a record with both ends within 3 bases) | "
               "records in those candidates | of them within 3 bases" % len(lines))
    tot = [0, 0, 0, 0]
    for cl in CLASSES:
        v = cells[cl]
        tot = [x + y for x, y in zip(tot, v)]
        out.append("  %5d .. %4d | %5d | %5d (%.3f) | %6d | %5d (%.3f)" % (cl[0], cl[1] - 1, v[0], v[1], v[1] / v[0] if v[0] else 0.0, v[2], v[3],
                                                                          v[3] / v[2] if v[2] else 0.0))
    out.append("  all           | %5d | %5d (%.3f) | %6d | %5d (%.3f)" % (tot[0], tot[1], tot[1] / max(tot[0], 1), tot[2], tot[3], tot[3] / max(tot[2], 1)))
    out.append("misses: elements under the 200-base minimum; elements with a tail match nearer than their own at >= 200 bases from the head "
               "(each head pairs with the NEAREST tail); the other records of a candidate are heads or tails that random text matches at threshold 1")
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
