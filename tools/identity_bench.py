#!/usr/bin/env python
"""Throughput and effect of the pairwise identity (hite_pair_identity) under the cd-hit-est stand-in (util.remove_redundant_sequences,
where the reference runs `cd-hit-est -aS 0.95 -aL 0.95 -c <c> -G 0 -g 1 -A 80`):
    python tools/identity_bench.py [--families 600] [--copies 5] [--twin-pairs 2000] [--out profiles/r07_pair_identity.txt]
Library: `--families` consensus sequences of hite_amd/synth.py (TIR families, 150 - 3 000 bases), `--copies` copies of each, every copy
0 - 15 % away from its consensus (substitutions, a tenth of that rate again as single-base indels), shuffled.  The library goes
through remove_redundant_sequences with the switch off and with it on (c = 0.8 and c = 0.95).  Records: the pairs the identity step
sends, the kernel's pairs per second and band cells per second (HIP events around ident_pair_kernel, and the wall time of
Context.pair_identity with its copies), the twin's on the same host on `--twin-pairs` of the same pairs, the wall time of the whole
function both ways and the share the identity step adds, and how many planted families come out as exactly one record."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def make(rng, n_fam, n_copy):
    from hite_amd import synth

    fams = synth.make_families(rng, n_fam, 0)
    recs = []
    for f, fam in enumerate(fams):
        for k in range(n_copy):
            div = float(rng.uniform(0.0, 0.15))
            s = synth._mutate_copy(rng, fam["cons"], div, div / 10)
            recs.append(("fam%d_c%d" % (f, k), np.frombuffer(b"ACGT", np.uint8)[s].tobytes().decode()))
    order = rng.permutation(len(recs))
    return [recs[i] for i in order]


def band_cells(pairs, band):
    """cells (i, j) inside the band, summed over the pairs"""
    total = 0
    for (_a, a0, a1, _b, b0, b1, _s) in pairs:
        m, n = a1 - a0, b1 - b0
        lo, hi = min(0, n - m) - band, max(0, n - m) + band
        i = np.arange(m + 1)
        total += int((np.minimum(n, i + hi) - np.maximum(0, i + lo) + 1).clip(min=0).sum())
    return total


class Recorder:
    """the context, remembering what the identity step sends and how long the call takes"""

    def __init__(self, ctx):
        self._ctx = ctx
        self.sent = None
        self.seconds = 0.0

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    def pair_identity(self, seqs, pairs, band=32):
        t0 = time.perf_counter()
        out = self._ctx.pair_identity(seqs, pairs, band=band)
        self.seconds = time.perf_counter() - t0
        self.sent = (seqs, pairs, band)
        return out


def run(util, ctx, inp, out, **kw):
    t0 = time.perf_counter()
    util.remove_redundant_sequences(inp, out, ctx=ctx, **kw)
    return time.perf_counter() - t0, util.read_fasta(out)[0]


def once(names, n_fam):
    per = {}
    for n in names:
        f = n.split("_")[0]
        per[f] = per.get(f, 0) + 1
    return sum(1 for f in range(n_fam) if per.get("fam%d" % f, 0) == 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--families", type=int, default=600)
    ap.add_argument("--copies", type=int, default=5)
    ap.add_argument("--twin-pairs", type=int, default=2000)
    ap.add_argument("--commit", default=None, help="the commit the numbers are taken on (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_pair_identity.txt"))
    a = ap.parse_args()
    import tempfile

    import hite_amd
    import identity_twin as T
    from hite_amd import util

    rng = np.random.default_rng(707)
    recs = make(rng, a.families, a.copies)
    d = tempfile.mkdtemp(prefix="identity_bench_")
    inp = os.path.join(d, "lib.fa")
    with open(inp, "w") as f:
        f.write("".join(">%s\n%s\n" % r for r in recs))
    ctx = hite_amd.Context(0)
    rec = Recorder(ctx)
    devnull = open(os.devnull, "w")
    stderr, sys.stderr = sys.stderr, devnull
    try:
        run(util, ctx, inp, os.path.join(d, "warm.fa"))                                   # warm-up: code objects, scratch, the index
        run(util, rec, inp, os.path.join(d, "warm.fa"), c=0.8, identity="gpu")
        t_off, n_off = min((run(util, ctx, inp, os.path.join(d, "off.fa")) for _ in range(3)), key=lambda r: r[0])
        t_80, n_80 = min((run(util, rec, inp, os.path.join(d, "on80.fa"), c=0.8, identity="gpu") for _ in range(3)), key=lambda r: r[0])
        t_95, n_95 = min((run(util, rec, inp, os.path.join(d, "on95.fa"), c=0.95, identity="gpu") for _ in range(3)), key=lambda r: r[0])
    finally:
        sys.stderr = stderr
    seqs, pairs, band = rec.sent
    cells = band_cells(pairs, band)
    wall = min(_timed(ctx, seqs, pairs, band) for _ in range(3))
    ctx.profile(on=True, reset=True)
    ctx.pair_identity(seqs, pairs, band=band)
    k_ms, k_n = ctx.profile(on=False).get("ident_pair_kernel", (0.0, 0))
    sub = pairs[:a.twin_pairs]
    T.clib()
    t0 = time.perf_counter()
    tw = T.pair_identity(seqs, sub, band)
    t_twin = time.perf_counter() - t0
    same = bool((ctx.pair_identity(seqs, sub, band=band) == tw).all())
    sub_cells = band_cells(sub, band)
    try:
        commit = a.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    lens = [len(s) for _n, s in recs]
    lines = [
        "pairwise identity under the cd-hit-est stand-in (tools/identity_bench.py); taken on the tree above commit %s" % commit,
        "library: %d families x %d copies = %d sequences of %d - %d bases (%d bases), copies 0 - 15 %% from their consensus" %
        (a.families, a.copies, len(recs), min(lens), max(lens), sum(lens)),
        "pairs sent (chain records that pass both coverage tests, each once): %d, band %d, %d band cells" % (len(pairs), band, cells),
        "kernel (HIP events, %d launch(es)): %.3f ms -> %.0f pairs/s, %.3g band cells/s" %
        (k_n, k_ms, len(pairs) / (k_ms / 1e3) if k_ms else 0.0, cells / (k_ms / 1e3) if k_ms else 0.0),
        "Context.pair_identity wall time (copies included, best of 3): %.4f s -> %.0f pairs/s, %.3g band cells/s" %
        (wall, len(pairs) / wall, cells / wall),
        "twin on the same host (%d of the pairs, one CPU thread): %.3f s -> %.0f pairs/s, %.3g band cells/s; HIP == twin on them: %s" %
        (len(sub), t_twin, len(sub) / t_twin, sub_cells / t_twin, same),
        "remove_redundant_sequences, best of 3: switch off %.3f s; on, c = 0.8: %.3f s; on, c = 0.95: %.3f s" % (t_off, t_80, t_95),
        "the identity step (pair list, Context.pair_identity, the test) adds %.1f %% (c = 0.8) / %.1f %% (c = 0.95) to the switch-off time" %
        (100.0 * (t_80 - t_off) / t_off, 100.0 * (t_95 - t_off) / t_off),
        "records out: switch off %d; c = 0.8: %d; c = 0.95: %d" % (len(n_off), len(n_80), len(n_95)),
        "planted families that come out as exactly one record, of %d: switch off %d; c = 0.8: %d; c = 0.95: %d" %
        (a.families, once(n_off, a.families), once(n_80, a.families), once(n_95, a.families)),
        "(copies up to 15 % from the consensus are up to ~28 % from each other: at c = 0.95 a family is expected to split; "
        "parity with cd-hit-est itself is unpinned)",
    ]
    txt = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(txt)
    sys.stdout.write(txt)
    ctx.close()


def _timed(ctx, seqs, pairs, band):
    t0 = time.perf_counter()
    ctx.pair_identity(seqs, pairs, band=band)
    return time.perf_counter() - t0


if __name__ == "__main__":
    main()
