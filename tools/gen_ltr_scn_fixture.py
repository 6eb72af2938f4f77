#!/usr/bin/env python
"""Writes tests/golden/ltr_scn_filter.json.gz: a seeded genome of planted LTR elements with its `.scn` candidate table, and what the
REFERENCE's own code of FiLTR's steps 1 and 2 makes of it -- read_scn, get_recombination_ltr -> is_recombination,
get_all_potential_ltr_lines -> get_ltr_from_line, remove_dirty_LTR, filter_ltr_by_flank_seq_v2 -> judge_scn_line_by_flank_seq_v2 and
its rewriting of the lines (bin/FiLTR-main/src/Util.py), loaded from the reference tree and run unchanged (the technique of
tools/gen_ltr_filter_fixture.py).  Two things are replaced: the process pool by an in-process one, and `subprocess.run`, which
recognises the `blastn -subject S -query Q -outfmt 6 ... -out O` command line, computes the HSPs of the two FASTA files with the twin
(tests/pairhsp_twin.py; diag_min = 500 where a sequence is searched against itself, as util.get_all_potential_ltr_lines does) and
writes twelve blast6 columns.  So the fixture pins the rules around the search, not blastn itself.  It holds the inputs, the HSP
tables (keyed by the SHA-1 of the two sequences) and the reference's outputs, and no program text.  Runs in the build container only
(it needs the reference tree); regenerable byte for byte:
    PYTHONHASHSEED=0 python tools/gen_ltr_scn_fixture.py [--reference /root/reference]"""
import argparse
import gzip
import hashlib
import json
import os
import shutil
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PLAN = [("clean", 5), ("recomb", 3), ("nested", 3), ("overhang", 3), ("shifted", 3), ("dirty", 2), ("dup", 2)]
SEED = 20251019


def read_one_fasta(path):
    with open(path) as f:
        return "".join(line.strip() for line in f if not line.startswith(">"))


def sha(seq):
    return hashlib.sha1(seq.encode()).hexdigest()


def fake_run(table):
    """subprocess.run for the reference module: blastn on two FASTA files runs as the twin"""
    import pairhsp_twin as T

    def run(cmd, **_kw):
        assert cmd[0] == "blastn" and cmd[cmd.index("-outfmt") + 1] == "6", cmd
        q_path, s_path, out = cmd[cmd.index("-query") + 1], cmd[cmd.index("-subject") + 1], cmd[cmd.index("-out") + 1]
        q, s = read_one_fasta(q_path), read_one_fasta(s_path)
        diag_min = 500 if q_path == s_path else None
        hsps = T.one(q, s, diag_min)
        assert hsps is not None
        table.append({"q": sha(q), "s": sha(s), "diag_min": diag_min, "hsps": [list(h) for h in hsps]})
        with open(out, "w") as f:
            for qs, qe, ss, se, score, matches, columns in hsps:
                f.write("\t".join(str(x) for x in ("q", "s", "%.3f" % (100.0 * matches / columns), columns, columns - matches, 0, qs, qe, ss, se,
                                                   "0.0", score)) + "\n")
        return types.SimpleNamespace(returncode=0, stdout="", stderr="")
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("HITE_REFERENCE", "/root/reference"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ref_harness
    from hite_amd import synth

    ref_harness.REFERENCE_ROOT = a.reference
    U = ref_harness.load_filtr_util()
    table = []
    U.subprocess = types.SimpleNamespace(run=fake_run(table), PIPE=None)
    U.ProcessPoolExecutor = ref_harness.SyncExecutor
    U.as_completed = lambda jobs: list(jobs)
    quiet = lambda *_a, **_k: None  # noqa: E731
    log = types.SimpleNamespace(logger=types.SimpleNamespace(info=quiet, debug=quiet, error=quiet))

    g = synth.make_ltr_element_genome(PLAN, seed=SEED)
    work = tempfile.mkdtemp(prefix="ltr_scn_fixture_")
    try:
        scn, ref = os.path.join(work, "in.scn"), os.path.join(work, "ref.fa")
        with open(scn, "w") as f:
            f.write(g["scn"])
        with open(ref, "w") as f:
            for name, seq in g["contigs"].items():
                f.write(">%s\n%s\n" % (name, seq))
        for sub in ("recomb", "potential", "flank"):
            os.makedirs(os.path.join(work, sub))
        _names, ref_contigs = U.read_fasta(ref)
        out = {"contigs": g["contigs"], "scn": g["scn"], "truth": g["truth"]}
        cand_raw, lines_raw = U.read_scn(scn, log)
        cand, lines = U.read_scn(scn, log, remove_dup=True)
        out["read_scn"] = {"candidates": [list(cand_raw[k]) for k in sorted(cand_raw)], "lines": [lines_raw[k] for k in sorted(lines_raw)]}
        out["read_scn_remove_dup"] = {"candidates": [list(cand[k]) for k in sorted(cand)], "lines": [lines[k] for k in sorted(lines)]}
        # step 1a
        n0 = len(table)
        recomb = sorted(U.get_recombination_ltr(cand, ref_contigs, 1, os.path.join(work, "recomb"), log))
        out["recombination_candidates"] = recomb
        confident = [lines[k] for k in cand if k not in recomb]
        # step 1b
        n1 = len(table)
        side = os.path.join(work, "all_potential_ltr.json")
        potential = U.get_all_potential_ltr_lines(confident, ref, 1, side, os.path.join(work, "potential"), log)
        out["potential_lines"] = potential
        with open(side, encoding="utf-8") as f:
            out["potential_json"] = f.read()
        out["dirty_dicts"] = U.remove_dirty_LTR(potential, log)
        recomb_scn, final_scn = os.path.join(work, "remove_recomb.scn"), os.path.join(work, "filter_terminal_align.scn")
        U.store_scn(potential, recomb_scn)
        with open(recomb_scn) as f:
            out["remove_recomb_scn"] = f.read()
        # step 2
        n2 = len(table)
        U.filter_ltr_by_flank_seq_v2(recomb_scn, final_scn, ref, 1, os.path.join(work, "flank"), log)
        with open(final_scn) as f:
            out["filter_terminal_align_scn"] = f.read()
        out["hsp_tables"] = {"recombination": table[n0:n1], "potential_lines": table[n1:n2], "flank_align": table[n2:]}
    finally:
        shutil.rmtree(work)
    path = os.path.join(ROOT, "tests", "golden", "ltr_scn_filter.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(out, separators=(",", ":"), sort_keys=True).encode())
    final = out["filter_terminal_align_scn"].splitlines()
    tab, wrong = synth.ltr_element_decisions(g["truth"], out["remove_recomb_scn"].splitlines(), final, out["dirty_dicts"])
    print("wrote %s: %d lines in, %d recombinant, %d after step 1, %d after step 2, %d searches, as planted %s (not: %s), %d bytes" %
          (path, len(lines), len(recomb), len(potential), len(final), len(table), dict(sorted(tab.items())), wrong, os.path.getsize(path)))


if __name__ == "__main__":
    main()
