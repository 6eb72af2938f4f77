#!/usr/bin/env python
"""Throughput and recall of the translated protein search (hite_protein_search, where the reference runs
`blastx -evalue 1e-20 -outfmt 6`) on synthetic data of the size of the largest bundled library:
    python tools/protein_bench.py [--queries 1000] [--proteins 4642] [--residues 2900000] [--per-cell 40] [--out profiles/r07_protein_search.json]
Library: `--proteins` random proteins (uniform residues, log-normal lengths scaled to `--residues` in all; only these two numbers are
taken from TIRPeps.lib).  Queries: random DNA of 1-4 kb; into `--per-cell` of them per (divergence, length) cell a window of a
library protein is planted: every residue replaced with the cell's probability (independently), back-translated with random
codons, on a random strand.  Records per-kernel time (hite_profile_*), seed hits / survivors / tasks per query, queries per second,
and per cell: of the planted domains whose best Smith-Waterman alignment against their source protein (the twin's exhaustive
mode, all six frames, the whole matrix) reaches E <= 1e-20 in the search space of the whole library, the share the seeded search
reports on that frame and protein, and the share reported with both ends within 5 residues (15 bases) of it.
Synthetic proteins with independent substitutions: single exact 4-mers are a lower bound for real, block-conserved families."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DIVS = (0.2, 0.3, 0.4, 0.5)
LENS = (120, 200, 300)


def make(rng, n_query, n_prot, n_res, per_cell):
    import protein_cases as PC

    ln = np.exp(rng.normal(0.0, 0.6, n_prot))
    ln = np.clip(np.round(ln * (n_res / ln.sum())), 40, 6000).astype(int)
    prots = [PC.rand_protein(rng, int(n)) for n in ln]
    queries = [PC.rand_dna(rng, int(rng.integers(1000, 4001))) for _ in range(n_query)]
    planted = []                 # (query, protein, divergence, length)
    long_enough = [p for p, s in enumerate(prots) if len(s) >= max(LENS)]
    q = 0
    for div in DIVS:
        for length in LENS:
            for _ in range(per_cell):
                if q >= n_query:
                    break
                p = long_enough[int(rng.integers(0, len(long_enough)))]
                a = int(rng.integers(0, len(prots[p]) - length + 1))
                dom = PC.back_translate(rng, PC.diverge(rng, prots[p][a:a + length], div))
                host = queries[q]
                at = int(rng.integers(0, max(1, len(host) - len(dom))))
                s = host[:at] + dom + host[at + len(dom):]
                queries[q] = s if rng.random() < 0.5 else PC.revcomp(s)
                planted.append((q, p, div, length))
                q += 1
    return queries, prots, planted


def recall(queries, prots, planted, rec, evalue):
    """per (divergence, length): [planted, exhaustive hits at E <= evalue, of those reported, of those with both ends within 5 residues]"""
    import protein_twin as T

    n_res = sum(len(p) for p in prots)
    by_pair = {}
    for r in rec:
        by_pair.setdefault((int(r[0]), int(r[1])), []).append([int(v) for v in r])
    cells = {}
    for (q, p, div, length) in planted:
        c = cells.setdefault("%d%%_%daa" % (round(div * 100), length), [0, 0, 0, 0])
        c[0] += 1
        y = T.encode(prots[p])
        best = None
        for f, aa in enumerate(T.translate6(queries[q])):
            x = T.encode_frame(aa)
            if len(x):
                h = T.gapped(x, 0, len(x) - 1, y, -(1 << 40), 1 << 40)
                if best is None or h[0] > best[1][0]:
                    best = (f, h)
        if best is None or best[1][0] < T.smin(len(queries[q]) // 3, n_res, evalue):
            continue
        c[1] += 1
        f, (sc, si, sj, ei, ej, _idn, _cols) = best
        L, o = len(queries[q]), f % 3
        qs, qe = (o + 3 * si + 1, o + 3 * ei + 3) if f < 3 else (L - (o + 3 * si), L - (o + 3 * ei + 2))
        frame = f + 1 if f < 3 else -(f - 2)
        same = [r for r in by_pair.get((q, p), []) if r[2] == frame and min(r[6], ej + 1) >= max(r[5], sj + 1)]
        if same:
            c[2] += 1
            if any(abs(r[5] - (sj + 1)) <= 5 and abs(r[6] - (ej + 1)) <= 5 and abs(r[3] - qs) <= 15 and abs(r[4] - qe) <= 15 for r in same):
                c[3] += 1
    return cells


def main(ctx=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--proteins", type=int, default=4642)
    ap.add_argument("--residues", type=int, default=2_900_000)
    ap.add_argument("--per-cell", type=int, default=40)
    ap.add_argument("--evalue", type=float, default=1e-20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_protein_search.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(707)
    queries, prots, planted = make(rng, a.queries, a.proteins, a.residues, a.per_cell)
    if ctx is None:
        import hite_amd

        ctx = hite_amd.Context(0)
    t0 = time.perf_counter()
    lib = ctx.protein_lib(prots)
    build_s = time.perf_counter() - t0
    ctx.protein_search(queries[:50], lib, evalue=a.evalue)            # warm-up: the arena grows, the code objects load
    best_s, rec, stats = None, None, None
    for _ in range(3):
        st = {}
        t0 = time.perf_counter()
        rec = ctx.protein_search(queries, lib, evalue=a.evalue, stats=st)
        dt = time.perf_counter() - t0
        if best_s is None or dt < best_s:
            best_s, stats = dt, st
    kernels = {}
    if hasattr(ctx, "profile"):
        ctx.profile(on=True, reset=True)
        ctx.protein_search(queries, lib, evalue=a.evalue)
        kernels = {k: {"ms": round(ms, 3), "launches": n} for k, (ms, n) in ctx.profile(on=False).items() if k.startswith("prot_")}
    t0 = time.perf_counter()
    cells = recall(queries, prots, planted, rec, a.evalue)
    line = {"queries": len(queries), "query_bases": sum(len(s) for s in queries), "proteins": len(prots), "library_residues": sum(len(p) for p in prots),
            "evalue": a.evalue, "lib_build_s": round(build_s, 4), "search_s_best_of_3": round(best_s, 4),
            "queries_per_s": round(len(queries) / best_s, 1), "hsps": int(len(rec)),
            "seed_hits_per_query": round(stats.get("hits", 0) / len(queries), 1), "survivors_per_query": round(stats.get("survivors", 0) / len(queries), 2),
            "tasks_per_query": round(stats.get("tasks", 0) / len(queries), 3), "kernels": kernels,
            "recall": {k: {"planted": v[0], "exhaustive_hits": v[1], "reported": v[2], "ends_within_5": v[3],
                           "reported_share": round(v[2] / v[1], 3) if v[1] else None, "ends_share": round(v[3] / v[1], 3) if v[1] else None}
                       for k, v in cells.items()},
            "recall_twin_s": round(time.perf_counter() - t0, 1),
            "note": "synthetic uniform-residue proteins, independent substitutions; exhaustive = the twin's full Smith-Waterman of the six "
                    "frames against the source protein, E in the search space of the whole library, no length adjustment"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(line, indent=1) + "\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
