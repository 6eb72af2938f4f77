#!/usr/bin/env python
"""Writes tests/golden/ltr_flank_filter.json.gz: seeded `.matrix` inputs and what the REFERENCE's own decision code of FiLTR's step 3
makes of them -- generate_sort_matrix (bin/FiLTR-main/utils/data_util.py), filter_ltr_by_flanking_cluster_sub, get_low_copy_LTR_sub,
get_high_copy_LTR_sub and judge_both_ends_frame (bin/FiLTR-main/src/Util.py), loaded from the reference tree and run unchanged.
The one thing replaced is the tool they shell out to: `os.system` inside the two modules recognises `cd-hit-est ... -i X -o Y`,
clusters X with the twin (tests/framecluster_twin.py) at the options on the command line and writes Y and Y.clstr in the tool's
format (the technique of low_copy_rescue.json.gz, whose blastx table is made up in the same way).  So the fixture pins the rules
around the clustering, not cd-hit-est itself.  Runs in the build container only (it needs the reference tree); regenerable byte for
byte:
    PYTHONHASHSEED=0 python tools/gen_ltr_filter_fixture.py [--reference /root/reference]"""
import argparse
import gzip
import importlib.util
import json
import os
import shlex
import shutil
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
FLANK = 100


def load_data_util(reference):
    """utils/data_util.py of the vendored FiLTR, with the imports this machine lacks stubbed (none of them is on the path of
    generate_sort_matrix)"""
    for name in ("pandas", "openpyxl", "openpyxl.utils", "sklearn", "sklearn.preprocessing", "sklearn.cluster", "PIL", "PIL.Image", "configs",
                 "configs.config", "matplotlib", "matplotlib.pyplot", "seaborn", "torch"):
        try:
            importlib.import_module(name)
        except Exception:
            mod = types.ModuleType(name)
            mod.__getattr__ = lambda attr: object          # `from x import Anything` succeeds
            sys.modules[name] = mod
    spec = importlib.util.spec_from_file_location("filtr_data_util", os.path.join(reference, "bin", "FiLTR-main", "utils", "data_util.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def fake_system(real_system, log):
    """os.system for the reference modules: cd-hit-est runs as the twin, everything else (cp, rm) as it is"""
    import framecluster_twin as T

    def system(cmd):
        words = shlex.split(cmd.split(">")[0]) if cmd.lstrip().startswith("cd-hit-est") else []
        if not words:
            return real_system(cmd)
        opt = {words[k]: words[k + 1] for k in range(1, len(words) - 1, 2)}
        names, seqs = [], []
        with open(opt["-i"]) as f:
            for line in f:
                if line.startswith(">"):
                    names.append(line[1:].strip())
                    seqs.append("")
                elif names:
                    seqs[-1] += line.strip()
        kw = dict(ident=float(opt["-c"]), cov_short=float(opt.get("-aS", 0.0)), cov_long=float(opt.get("-aL", 0.0)), min_cov=int(opt.get("-A", 0)),
                  min_len=10, both_strands=True)
        log.append(kw)
        clusters = T.frame_cluster([seqs], **kw)[0]
        with open(opt["-o"], "w") as f:
            for cl in clusters:
                f.write(">%s\n%s\n" % (names[cl[0]], seqs[cl[0]]))
        with open(opt["-o"] + ".clstr", "w") as f:
            for c, cl in enumerate(clusters):
                f.write(">Cluster %d\n" % c)
                for k, r in enumerate(cl):
                    f.write("%d\t%dnt, >%s... %s\n" % (k, len(seqs[r]), names[r], "*" if k == 0 else "at +/100.00%"))
        return 0
    return system


# ---- seeded inputs ----------------------------------------------------------------------------------------------------------------
def dna(rng, n):
    return "".join("ACGT"[k] for k in rng.integers(0, 4, n))


def diverge(rng, s, rate):
    return "".join("ACGT"[rng.integers(0, 4)] if rng.random() < rate else ch for ch in s)


def frame(rng, seq, side, gaps=0.03, short=0):
    """a frame of FLANK columns as get_both_ends_frame writes it: the bases next to the terminal sequence, '-' where the row has a
    gap, '-' padding away from the element when the row is shorter"""
    seq = "".join("-" if rng.random() < gaps else ch for ch in seq[:FLANK - short])
    return "-" * (FLANK - len(seq)) + seq if side == "left" else seq + "-" * (FLANK - len(seq))


def make_matrix(rng, n_rows, left_homo, right_homo, twins=0, short_rows=0, extend_l=0, extend_r=0):
    """n_rows rows; left_homo / right_homo: the share of rows whose flank on that side descends from one ancestor (a terminal cut
    out of a longer repeat); twins: rows that repeat both flanks of row 0 (an element inside another, transposed again);
    short_rows: rows whose frames keep 10 bases or fewer; extend_l / extend_r: bases next to the element that every row shares (a
    terminal sequence cut short of the element's end: too few bases for the clustering, enough for the frame vote)"""
    anc_l, anc_r = dna(rng, FLANK), dna(rng, FLANK)
    rows = []
    for k in range(n_rows):
        ls = diverge(rng, anc_l, 0.05) if rng.random() < left_homo else dna(rng, FLANK)
        rs = diverge(rng, anc_r, 0.05) if rng.random() < right_homo else dna(rng, FLANK)
        ls, rs = ls[:FLANK - extend_l] + anc_l[FLANK - extend_l:], anc_r[:extend_r] + rs[extend_r:]
        short = FLANK - int(rng.integers(0, 11)) if k < short_rows else 0
        rows.append([frame(rng, ls, "left", short=short), frame(rng, rs, "right", short=short)])
    for k in range(1, min(twins, n_rows - 1) + 1):
        rows[k] = [frame(rng, rows[0][0].replace("-", "A"), "left", gaps=0.01), frame(rng, rows[0][1].replace("-", "C"), "right", gaps=0.01)]
    return rows


def inputs():
    rng = np.random.default_rng(20251019)
    plan = [(1, 0, 0, 0, 0), (2, 0, 0, 0, 0), (3, 0, 0, 0, 0), (5, 0, 0, 0, 0), (6, 0, 0, 0, 0), (12, 0, 0, 0, 0), (19, 0, 0, 0, 0),
            (20, 0, 0, 0, 0), (40, 0, 0, 0, 0), (100, 0, 0, 0, 0),
            (3, 1, 1, 0, 0), (12, 1, 1, 0, 0), (30, 1, 1, 0, 0), (12, 1, 0, 0, 0), (12, 0, 1, 0, 0), (30, 0.95, 0, 0, 0),
            (10, 0.7, 0.7, 0, 0), (19, 0.75, 0.2, 0, 0), (20, 0.75, 0.2, 0, 0), (25, 0.85, 0.85, 0, 0), (25, 0.3, 0.95, 0, 0),
            (4, 0, 0, 1, 0), (6, 0, 0, 2, 0), (8, 0, 0, 3, 0), (9, 0, 0, 4, 0), (12, 0, 0, 5, 0), (12, 0, 0, 7, 0), (5, 0.5, 0.5, 1, 0),
            (6, 0, 0, 0, 2), (3, 0, 0, 0, 2), (2, 0, 0, 0, 1), (14, 0.4, 0.4, 2, 3),
            (12, 0, 0, 0, 0, 25, 25), (4, 0, 0, 0, 0, 25, 0), (12, 0, 0, 0, 0, 0, 28), (8, 0, 0, 0, 0, 10, 0)]
    return [("ltr_%d" % k, make_matrix(rng, *p)) for k, p in enumerate(plan)]


def read_matrix(path):
    with open(path) as f:
        return [line.replace("\n", "").split("\t") for line in f]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("HITE_REFERENCE", "/root/reference"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ref_harness

    ref_harness.REFERENCE_ROOT = a.reference
    U = ref_harness.load_filtr_util()
    calls = []
    restore = os.system          # the reference modules call os.system of the shared os module: swapped for the time of the run
    os.system = fake_system(restore, calls)
    try:
        try:
            D = load_data_util(a.reference)
            sort_pinned = True
        except Exception as e:          # the sort rule then stays restated and unpinned
            print("data_util.py cannot be imported here (%s: %s): the fixture holds the Util.py rules only" % (type(e).__name__, e))
            D, sort_pinned = None, False
        work = tempfile.mkdtemp(prefix="ltr_filter_fixture_")
        cases = []
        for name, rows in inputs():
            d = os.path.join(work, name)
            for sub in ("in", "sort", "keep", "low", "high", "tmp"):
                os.makedirs(os.path.join(d, sub))
            src = os.path.join(d, "in", name + ".matrix")
            with open(src, "w") as f:
                for left, right in rows:
                    f.write(left + "\t" + right + "\n")
            case = {"name": name, "matrix": rows, "sort": None, "sort_pinned": sort_pinned}
            cur = src
            if D is not None:
                kept = os.path.join(d, "sort", name + ".matrix")
                is_keep = D.generate_sort_matrix(src, kept, os.path.join(d, "tmp", "s.fa"), os.path.join(d, "tmp", "s.cons"))
                assert bool(is_keep) == os.path.exists(kept)
                case["sort_keep"] = bool(is_keep)
                if is_keep:
                    case["sort"] = read_matrix(kept)
                    cur = kept
            # the later rules on the matrix that reaches them (the input itself where the sort rule dropped it: every rule is pinned on every case)
            q, flank_keep = U.filter_ltr_by_flanking_cluster_sub(cur, os.path.join(d, "keep"), os.path.join(d, "tmp", "j.fa"), os.path.join(d, "tmp", "j.fa.cons"))
            assert q == name and bool(flank_keep) == os.path.exists(os.path.join(d, "keep", name + ".matrix"))
            U.get_low_copy_LTR_sub([cur], os.path.join(d, "low"), 5)
            U.get_high_copy_LTR_sub([cur], os.path.join(d, "high"), 5)
            q, is_ltr = U.judge_both_ends_frame(cur, 20, FLANK)
            case.update(flank_keep=bool(flank_keep), low=bool(os.listdir(os.path.join(d, "low"))), high=bool(os.listdir(os.path.join(d, "high"))),
                        vote=bool(is_ltr))
            cases.append(case)
        shutil.rmtree(work)
    finally:
        os.system = restore
    assert {json.dumps(c, sort_keys=True) for c in calls} == {json.dumps(c, sort_keys=True) for c in (
        dict(ident=0.8, cov_short=0.3, cov_long=0.0, min_cov=20, min_len=10, both_strands=True),
        dict(ident=0.95, cov_short=0.95, cov_long=0.95, min_cov=50, min_len=10, both_strands=True))}, "the options the reference passes"
    path = os.path.join(ROOT, "tests", "golden", "ltr_flank_filter.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps({"flank": FLANK, "cases": cases}, separators=(",", ":"), sort_keys=True).encode())
    n = lambda key: sum(1 for c in cases if c.get(key))  # noqa: E731
    print("wrote %s: %d matrices (sort keeps %d, joined rule keeps %d, low %d, high %d, vote passes %d), %d bytes" %
          (path, len(cases), n("sort_keep"), n("flank_keep"), n("low"), n("high"), n("vote"), os.path.getsize(path)))


if __name__ == "__main__":
    main()
