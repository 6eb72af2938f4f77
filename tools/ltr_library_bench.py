#!/usr/bin/env python
"""FiLTR's step 4, the full-length copy support of the intact LTR elements, host to host on one GPU: planted LTR families on a genome
of `--genome-mbp` (hite_amd/synth.make_workload), every planted full-length copy an element and a candidate line.
  (a) Context.ltr_copy_support: the copy finder and the two kernels of hite_ltrcopy.hip with the copy table left on the device --
      wall seconds (best of `--repeat`, after a warming call; the index of the genome is built before and not counted), the library's
      own HIP-event times of the finder's stages and of the two kernels, the bytes that come down;
  (b) the alternative it replaces: Context.find_copies(..., clips=True) brings the whole table down and
      tests/ltrcopy_twin.support_records applies the same rule on the host -- wall seconds of the download as arrays
      (find_copies_table), as the tuples the host rule reads (find_copies), and of the rule; the bytes that come down.
Both give the same copies (asserted).  minimap2 is on no machine of the project: it is not run and nothing is extrapolated to it.
    python tools/ltr_library_bench.py [--out profiles/r17_ltr_library.txt]"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mbp", type=int, default=100)
    ap.add_argument("--families", type=int, default=300)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_ltr_library.txt"))
    a = ap.parse_args()

    import ltrcopy_twin as LT
    import hite_amd
    from hite_amd import synth

    try:
        commit = a.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    t0 = time.perf_counter()
    w = synth.make_workload(genome_bp=a.genome_mbp * 1_000_000, n_tir=0, n_ltr=a.families, cands_per_family=1, seed=1701)
    off = w["contig_off"]
    genome = w["genome"]
    contigs = [genome[off[k]:off[k + 1]].tobytes() for k in range(len(off) - 1)]
    p = w["planted"]
    keep = np.flatnonzero(p["full"])
    std = [(int(p["contig"][i]), int(p["start"][i]), int(p["start"][i] + p["length"][i])) for i in keep]
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    elements = []
    for i in keep:
        s = contigs[int(p["contig"][i])][int(p["start"][i]):int(p["start"][i] + p["length"][i])]
        elements.append(s.translate(comp)[::-1] if p["minus"][i] else s)
    t_make = time.perf_counter() - t0
    ctx = hite_amd.Context(0)
    ctx.genome_pack(contigs)
    t0 = time.perf_counter()
    ctx.copy_index_build()
    t_index = time.perf_counter() - t0
    st = {}
    got = ctx.ltr_copy_support(elements, std, stats=st)          # warming call
    walls = []
    for _ in range(a.repeat):
        ctx.profile(on=True, reset=True)
        t0 = time.perf_counter()
        got = ctx.ltr_copy_support(elements, std)
        walls.append(time.perf_counter() - t0)
        prof = ctx.profile(on=False)
    ours = ("ltrcopy_match", "ltrcopy_element")
    finder_ms = sum(ms for k, (ms, _n) in prof.items() if k not in ours)
    down_fused = st["kept"] * 20 + len(elements) * 12 + 32
    # the alternative: the table down, the rule on the host
    t_tab, t_tup, t_rule = [], [], []
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        tab = ctx.find_copies_table(elements, clips=True)
        t_tab.append(time.perf_counter() - t0)
    n_rec = len(tab[1])
    for _ in range(max(1, a.repeat - 1)):
        t0 = time.perf_counter()
        rows = ctx.find_copies(elements, clips=True)
        t_tup.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        st_h = {}
        exp = LT.support_records([len(e) for e in elements], [[(r[0], r[1], r[2], r[5]) for r in rr] for rr in rows], std, [len(c) for c in contigs],
                                 stats=st_h)
        t_rule.append(time.perf_counter() - t0)
    assert got == exp and st == st_h, "the device and the host rule differ"
    down_table = n_rec * 33 + (len(elements) + 1) * 4
    lines = ["FiLTR step 4, full-length copy support of the intact LTR elements (Context.ltr_copy_support; hite_amd/csrc/hite_ltrcopy.hip) -- "
             "tools/ltr_library_bench.py; taken on the tree above commit %s, one MI355X" % commit,
             "planted genome: %d LTR families on %.0f Mbp in %d chromosomes, %d planted copies, %d of them full length = %d elements of %d .. %d "
             "bases (%.1f Mbp) = %d candidate lines (built in %.1f s; not part of the stage); index of the genome built in %.2f s, not counted below"
             % (a.families, a.genome_mbp, len(contigs), w["n_planted"], len(keep), len(elements), min(len(e) for e in elements),
                max(len(e) for e in elements), sum(len(e) for e in elements) / 1e6, len(std), t_make, t_index),
             "records: %(records)d in the copy table, %(covered)d pass the coverage rule at 0.985, %(matched)d of them coincide with a candidate "
             "line, %(kept)d kept after the redundancy rule" % st,
             "",
             "(a) copy table left on the device, host to host: wall best of %d = %.3f s (all: %s)" % (a.repeat, min(walls), " ".join("%.3f" % x for x in walls)),
             "    HIP-event times of the last call: finder stages %.1f ms, ltrcopy_match %.3f ms, ltrcopy_element %.3f ms; the rest of the wall "
             "time is the upload of the elements, host work and the download" % (finder_ms, prof.get(ours[0], (0.0, 0))[0], prof.get(ours[1], (0.0, 0))[0]),
             "    bytes down: %d (20 per kept copy, 12 per element)" % down_fused,
             "(b) whole table down, rule on the host (tests/ltrcopy_twin.support_records, plain Python):",
             "    finder + download as arrays (find_copies_table, clips): best %.3f s; bytes down: %d (33 per record)" % (min(t_tab), down_table),
             "    finder + download as the tuples the host rule reads (find_copies, clips): best %.3f s" % min(t_tup),
             "    the rule on the host: best %.3f s" % min(t_rule),
             "",
             "what was found: the table is %.2f MB against %.3f MB of kept copies (%.0f x fewer bytes down); finder + table as arrays takes %.3f s, the "
             "fused call %.3f s host to host (difference %+.3f s), the tuples add %.3f s and the rule in Python %.3f s.  Whether the download of "
             "the table dominates at cereal size (10^5 elements) is NOT MEASURED here: this genome has %d elements."
             % (down_table / 1e6, down_fused / 1e6, down_table / max(down_fused, 1), min(t_tab), min(walls), min(t_tab) - min(walls),
                min(t_tup) - min(t_tab), min(t_rule), len(elements))]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
