#!/usr/bin/env python
"""Writes tests/golden/ltr_deep.json.gz and tests/golden/ltr_deep_model.npy: seeded `.matrix` inputs and what the REFERENCE's own
hybrid CNN makes of them -- hybridLTR_feature_extractor.py (FeatureExtractor.process_file_chunk, called per file, without the
process pool), hybridLTR_model.py (class CNNCAT) and hybridLTR_predicter.py (CNNPredictor: the normalisation and the model on the
CPU in fp32) of bin/FiLTR-main/src/Deep_Learning, and alter_deep_learning_results of bin/FiLTR-main/src/Util.py, all loaded from
the reference tree and run unchanged, with models/production_model.pth.  Per matrix the fixture holds the SHA-256 of the reference's
image ([3][100][200], int64, C order: the reference's [100][200][3] array with the plane axis moved to the front) and of its
k-mer array ([2][3872], int64, C order), a few raw rows of each, the reference's fp32 logits and its decision at 0.5; then made-up
table triples with what the reference's merge makes of them; then the tolerance of the logits: the largest |reference fp32 logit -
twin binary64 logit| over the matrices (3 significant digits) and T = 32 x that.  ltr_deep_model.npy is the checkpoint as the
canonical flat fp32 array of include/hite_gpu.h.  Runs in the build container only (it needs the reference tree and its Python
dependencies); regenerable byte for byte:
    PYTHONHASHSEED=0 python tools/gen_ltr_deep_fixture.py [--reference /root/reference]"""
import argparse
import gzip
import hashlib
import importlib.util
import json
import os
import shutil
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
FLANK = 100
MIN_GAP = 0.05          # |l1 - l0| of every kept matrix: no test may call a case "too close to the threshold"


def dna(rng, n):
    return "".join("ACGT"[k] for k in rng.integers(0, 4, n))


def diverge(rng, s, rate):
    return "".join("ACGT"[rng.integers(0, 4)] if rng.random() < rate else ch for ch in s)


def gapped(rng, s, rate):
    return "".join("-" if rng.random() < rate else ch for ch in s)


def make_matrix(rng, kind, n_rows):
    """conserved: the flanks of all copies descend from one ancestor (a terminal cut out of a longer repeat: not an LTR); random: every
    copy sits in its own neighbourhood (an LTR); sparse: random with most cells missing; mixed: half and half"""
    anc_l, anc_r = dna(rng, FLANK), dna(rng, FLANK)
    rows = []
    for k in range(n_rows):
        homo = kind == "conserved" or (kind == "mixed" and k % 2 == 0)
        ls = diverge(rng, anc_l, 0.06) if homo else dna(rng, FLANK)
        rs = diverge(rng, anc_r, 0.06) if homo else dna(rng, FLANK)
        rate = 0.6 if kind == "sparse" else 0.03
        rows.append([gapped(rng, ls, rate), gapped(rng, rs, rate)])
    return rows


def put(rows, r, c, ch):
    side, at = divmod(c, FLANK)
    rows[r][side] = rows[r][side][:at] + ch + rows[r][side][at + 1:]


def special(rng, what):
    if what == "support pairs":        # columns whose (count, total) are (29, 100), (57, 100), (58, 100) and (29, 50)
        rows = make_matrix(rng, "random", 100)
        for r in range(100):
            put(rows, r, 10, "A" if r < 29 else "C")
            put(rows, r, 11, "G" if r < 57 else "T")
            put(rows, r, 12, "T" if r < 58 else "A")
            put(rows, r, 113, ("A" if r < 29 else "G") if r < 50 else "-")
        return rows
    if what == "gap, N and lower-case columns":
        rows = make_matrix(rng, "random", 40)
        for r in range(40):
            put(rows, r, 0, "-")               # an all-gap column at the edge
            put(rows, r, 57, "-")
            put(rows, r, 58, "N")              # a column whose only non-gap bytes are N
            put(rows, r, 199, "acgtn"[r % 5])  # lower-case bytes are gaps
            put(rows, r, 120, "acgt"[r % 4] if r % 3 else "G")
        return rows
    if what == "an all-gap half":
        rows = make_matrix(rng, "conserved", 30)
        return [[left, "-" * FLANK] for left, _right in rows]
    raise ValueError(what)


PLAN = [("random", 6), ("random", 7), ("random", 63), ("random", 64), ("random", 65), ("random", 99), ("random", 100),
        ("conserved", 6), ("conserved", 7), ("conserved", 64), ("conserved", 99), ("conserved", 100), ("conserved", 20),
        ("sparse", 12), ("sparse", 65), ("sparse", 100), ("mixed", 30), ("mixed", 63), ("random", 20), ("conserved", 40),
        ("special", "support pairs"), ("special", "gap, N and lower-case columns"), ("special", "an all-gap half"), ("random", 5)]


def load_deep_learning(reference):
    """the three Deep_Learning modules of the vendored FiLTR, unchanged (they import each other by bare name)"""
    d = os.path.join(reference, "bin", "FiLTR-main", "src", "Deep_Learning")
    sys.path.insert(0, d)
    mods = {}
    for name in ("hybridLTR_model", "hybridLTR_feature_extractor", "hybridLTR_predicter"):
        spec = importlib.util.spec_from_file_location(name, os.path.join(d, name + ".py"))
        mods[name] = importlib.util.module_from_spec(spec)
        sys.modules[name] = mods[name]
        spec.loader.exec_module(mods[name])
    return mods


def reference_run(mods, model_path, work, named):
    """-> per matrix (image [3][100][200] int64, kmer [2][3872] int64, fp32 logits [2], decision at 0.5)"""
    import logging

    import torch

    torch.set_num_threads(1)
    quiet = logging.getLogger("ltr_deep_fixture")
    quiet.setLevel(logging.ERROR)
    src = os.path.join(work, "in")
    os.makedirs(src)
    for name, rows in named:
        with open(os.path.join(src, name + ".matrix"), "w") as f:
            for left, right in rows:
                f.write(left + "\t" + right + "\n")
    ext = mods["hybridLTR_feature_extractor"].FeatureExtractor(src, 1, logger=quiet)
    res = [ext.process_file_chunk(os.path.join(src, name + ".matrix")) for name, _rows in named]
    assert all(r is not None and r["name"] == name for r, (name, _rows) in zip(res, named))
    img = torch.stack([torch.from_numpy(r["features"]) for r in res]).permute(0, 3, 1, 2)
    freq = torch.unsqueeze(torch.stack([torch.from_numpy(r["freqs"]) for r in res]), dim=2)
    assert tuple(img.shape[1:]) == (3, 100, 200) and tuple(freq.shape[1:]) == (2, 1, 3872)
    pred = mods["hybridLTR_predicter"].CNNPredictor(model_path, 0.5, "cpu", logger=quiet)
    with torch.no_grad():
        logits = pred.model(pred._normalize_features(img), pred._normalize_features(freq))
        probs = torch.nn.functional.softmax(logits, dim=1)
    decisions = np.where(probs.numpy()[:, 1] > pred.threshold, 1, 0)
    out = []
    for k in range(len(named)):
        out.append((img[k].numpy().astype(np.int64), freq[k, :, 0, :].numpy().astype(np.int64), logits[k].numpy().astype(np.float32), int(decisions[k])))
    state = {k: v.numpy() for k, v in pred.model.state_dict().items()}
    return out, state


def reference_merge(U, work, deep, homology, names):
    d = os.path.join(work, "merge")
    shutil.rmtree(d, ignore_errors=True)
    os.makedirs(os.path.join(d, "high"))
    for n in names:
        open(os.path.join(d, "high", n + ".matrix"), "w").write("-\t-\n")
    for table, f in ((deep, "dl.txt"), (homology, "hc.txt")):
        if table:
            with open(os.path.join(d, f), "w") as fh:
                for n, v in table.items():
                    fh.write("%s\t%d\n" % (n, v))
    log = types.SimpleNamespace(logger=types.SimpleNamespace(debug=lambda *_a: None, info=lambda *_a: None))
    U.alter_deep_learning_results(os.path.join(d, "dl.txt"), os.path.join(d, "hc.txt"), os.path.join(d, "out.txt"), os.path.join(d, "high"), log)
    with open(os.path.join(d, "out.txt")) as fh:
        return {line.split("\t")[0]: int(line.split("\t")[1]) for line in fh if line.strip()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("HITE_REFERENCE", "/root/reference"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ltrdeep_twin as T
    import ref_harness
    from hite_amd import util

    ref_harness.REFERENCE_ROOT = a.reference
    U = ref_harness.load_filtr_util()
    mods = load_deep_learning(a.reference)
    model_path = os.path.join(a.reference, "bin", "FiLTR-main", "models", "production_model.pth")
    work = tempfile.mkdtemp(prefix="ltr_deep_fixture_")
    try:
        rng = np.random.default_rng(20261021)
        named = [("deep_%d" % k, special(rng, p[1]) if p[0] == "special" else make_matrix(rng, *p)) for k, p in enumerate(PLAN)]
        ref, state = reference_run(mods, model_path, os.path.join(work, "a"), named)
        for attempt in range(1, 20):          # a matrix too close to the threshold is drawn again (never observed)
            close = [k for k, r in enumerate(ref) if abs(float(r[2][1]) - float(r[2][0])) < MIN_GAP and PLAN[k][0] != "special"]
            if not close:
                break
            for k in close:
                named[k] = (named[k][0], make_matrix(rng, *PLAN[k]))
            ref, state = reference_run(mods, model_path, os.path.join(work, "a%d" % attempt), named)
        assert all(abs(float(r[2][1]) - float(r[2][0])) >= MIN_GAP for r in ref), "a matrix within MIN_GAP of the threshold"
        assert {r[3] for r in ref} == {0, 1}, "both decisions occur"
        params = util.ltr_model_params(state)
        np.save(os.path.join(ROOT, "tests", "golden", "ltr_deep_model.npy"), params)
        twin_logits, status = T.ltr_deep(params, [rows for _n, rows in named])
        assert not status.any()
        measured = max(float(np.abs(twin_logits[k] - r[2].astype(np.float64)).max()) for k, r in enumerate(ref))
        measured = float("%.3g" % measured)
        cases = []
        for (name, rows), (img, kmer, logits, decision) in zip(named, ref):
            cases.append({"name": name, "matrix": rows, "img_sha256": hashlib.sha256(np.ascontiguousarray(img).tobytes()).hexdigest(),
                          "kmer_sha256": hashlib.sha256(np.ascontiguousarray(kmer).tobytes()).hexdigest(),
                          "img_rows": {"%d,%d" % (p, r): img[p, r].tolist() for p in range(3) for r in (0, len(rows) - 1, 99)},
                          "kmer_head": kmer[:, :130].tolist(), "kmer_sum": [int(x) for x in kmer.sum(axis=1)],
                          "logits": [float(logits[0]), float(logits[1])], "decision": decision})
        triples = [({}, {}, ["a", "b"]), ({}, {"a": 1, "b": 0}, ["a", "b"]), ({"a": 0, "b": 1}, {}, ["a", "b"]),
                   ({"a": 1, "b": 1, "c": 0, "d": 0}, {"a": 1, "b": 0, "c": 1, "d": 0}, ["a", "b", "c", "d"]),
                   ({"a": 1}, {"a": 1, "absent": 1, "vetoed": 0}, ["a", "absent", "vetoed"])]
        merges = [{"deep": d, "homology": h, "names": n, "result": reference_merge(U, work, d, h, n)} for d, h, n in triples]
        assert "absent" not in merges[-1]["result"] and merges[-1]["result"]["vetoed"] == 0
    finally:
        shutil.rmtree(work, ignore_errors=True)
    doc = {"cases": cases, "merge": merges, "threshold": 0.5, "min_gap": MIN_GAP,
           "tolerance": {"measured": measured, "factor": 32, "T": 32 * measured}}
    path = os.path.join(ROOT, "tests", "golden", "ltr_deep.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(doc, separators=(",", ":"), sort_keys=True).encode())
    gaps = [abs(c["logits"][1] - c["logits"][0]) for c in cases]
    print("wrote %s: %d matrices (%d LTR, %d not), smallest |l1 - l0| %.3f, largest |reference - twin| %.3g, T %.3g, %d bytes; %s: %d bytes" %
          (path, len(cases), sum(c["decision"] for c in cases), sum(1 - c["decision"] for c in cases), min(gaps), measured, 32 * measured,
           os.path.getsize(path), "tests/golden/ltr_deep_model.npy", os.path.getsize(os.path.join(ROOT, "tests", "golden", "ltr_deep_model.npy"))))


if __name__ == "__main__":
    main()
