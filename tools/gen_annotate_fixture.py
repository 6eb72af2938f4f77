#!/usr/bin/env python
"""Writes tests/golden/annotate_gff.json.gz: a fixed hand-made table of annotation records, the GFF this build's writer
(util.write_repeatmasker_gff) makes of it, and what the REFERENCE's own reader of that file -- get_full_length_copies_from_gff_v1 with
its chaining FMEA_new (module/Util.py), loaded from the reference tree and run unchanged -- makes of the GFF.  The reader is the one
piece of reference code that consumes the annotation, so the fixture pins the writer's coordinates and format and the restated reader
(util.get_full_length_copies_from_gff_v1) to it.  The fixture holds data only: the library, the genome, the records, the GFF text and
the reader's three dictionaries, once with a transposon as the last line and once with a Helitron-named entry last (the reader takes
its flank length from the last line).  Runs where the reference tree is; regenerable byte for byte:
    python tools/gen_annotate_fixture.py [--reference DIR]"""
import argparse
import gzip
import importlib
import importlib.util
import json
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIB = [("TE_tir#DNA/hAT", 1000), ("TE_ltr#LTR/Gypsy", 2000), ("TE_short#DNA/MITE", 200), ("TE_line#LINE/L1", 3000), ("TE_frag#Unknown", 600),
       ("Chr1-Helitron_7#RC/Helitron", 400)]
CONTIGS = [("chrA", 60000), ("chrB", 40000), ("scaffold_3", 9000)]


def load_reference_util(reference):
    """module/Util.py of the reference, with the imports this machine lacks stubbed (none is on the path of the two functions)"""
    for name in ("Levenshtein", "PyPDF2", "fuzzysearch", "pysam", "seaborn"):
        try:
            importlib.import_module(name)
        except Exception:
            mod = types.ModuleType(name)
            mod.__getattr__ = lambda attr: object
            sys.modules[name] = mod
    spec = importlib.util.spec_from_file_location("hite_reference_util", os.path.join(reference, "module", "Util.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def record(seq, g_start, lib, strand, q_start, q_end, g_len=None):
    """an exact record: (seq, g_start, g_end, lib, strand, q_start, q_end, score, matches, columns)"""
    n = q_end - q_start
    g_len = n if g_len is None else g_len
    m = min(n, g_len)
    gaps = abs(n - g_len)
    return (seq, g_start, g_start + g_len, lib, strand, q_start, q_end, 2 * m - 5 * gaps, m, m + gaps)


def records():
    """about 60 records over 3 contigs and 6 entries.  skip_gap of an entry of L bases is 0.05 L (50 for TE_tir, 100 for TE_ltr)"""
    r = []
    # whole copies on both strands
    r += [record(0, 1000, 0, 0, 0, 1000), record(0, 4000, 0, 1, 0, 1000), record(1, 500, 1, 0, 0, 2000), record(1, 5000, 1, 1, 0, 2000)]
    # a copy just below and just above 95 % of the entry: 949 / 950 / 951 of 1 000, 1 899 / 1 900 of 2 000
    r += [record(0, 7000, 0, 0, 0, 949), record(0, 9000, 0, 0, 0, 950), record(0, 11000, 0, 1, 49, 1000), record(1, 9000, 1, 0, 0, 1899),
          record(1, 12000, 1, 0, 100, 2000), record(2, 100, 0, 0, 50, 1000)]
    # two fragments that chain across gaps just below and just above skip_gap, on the genome and in the entry
    for k, (g_gap, q_gap) in enumerate([(49, 0), (50, 0), (51, 0), (0, 49), (0, 50), (10, 49), (49, 49), (-20, 0), (-20, -20)]):
        at = 14000 + 2000 * k
        r += [record(0, at, 0, k & 1, 0, 500), record(0, at + 500 + g_gap, 0, k & 1, 500 + q_gap, 1000)]
    for k, (g_gap, q_gap) in enumerate([(99, 0), (100, 0), (0, 99), (0, 100)]):
        at = 15000 + 3000 * k
        r += [record(1, at, 1, 0, 0, 1200), record(1, at + 1200 + g_gap, 1, 0, 1200 + q_gap, 2000)]
    # three fragments in a row, a fragment that fits two chains, a fragment inside another, fragments out of order in the entry
    r += [record(0, 34000, 3, 0, 0, 1000), record(0, 35010, 3, 0, 1005, 2000), record(0, 36020, 3, 0, 2010, 3000)]
    r += [record(0, 40000, 4, 0, 0, 300), record(0, 40100, 4, 0, 100, 320), record(0, 40310, 4, 0, 310, 600)]
    r += [record(0, 42000, 4, 0, 0, 600), record(0, 42100, 4, 0, 100, 300)]
    r += [record(0, 44000, 4, 0, 300, 600), record(0, 44310, 4, 0, 0, 300)]
    # short entries, the same entry on another contig, gapped alignments (the genome interval shorter / longer than the entry's)
    r += [record(2, 2000, 2, 0, 0, 200), record(2, 2300, 2, 1, 0, 195), record(2, 2600, 2, 0, 0, 189), record(2, 3000, 2, 1, 10, 200)]
    r += [record(2, 4000, 0, 0, 0, 1000, g_len=990), record(2, 5500, 0, 1, 0, 1000, g_len=1012)]
    # a Helitron-named entry: whole, and a copy at the first bases of a contig (the flank would begin before it)
    r += [record(0, 50000, 5, 0, 0, 400), record(1, 30000, 5, 1, 0, 400), record(1, 20, 5, 0, 0, 400), record(1, 3, 2, 0, 0, 200),
          record(0, 52000, 5, 0, 0, 379), record(0, 53000, 5, 0, 0, 380)]
    # copies at the last bases of a contig
    r += [record(2, 8800, 2, 0, 0, 200), record(1, 39000, 0, 0, 0, 1000)]
    return sorted(r, key=lambda x: x[:7])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("HITE_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference")))
    a = ap.parse_args()
    from hite_amd import util

    ref = load_reference_util(a.reference)
    rng = np.random.default_rng(2024)
    draw = lambda n: "".join("ACGT"[k] for k in rng.integers(0, 4, size=n))  # noqa: E731
    lib = [(name, draw(n)) for name, n in LIB]
    genome = [(name, draw(n)) for name, n in CONTIGS]
    recs = records()
    out = {"lib": lib, "genome": genome, "records": recs, "full_length_threshold": 0.95, "variants": []}
    with tempfile.TemporaryDirectory() as d:
        lib_path, ref_path = os.path.join(d, "lib.fa"), os.path.join(d, "genome.fa")
        for path, seqs in ((lib_path, lib), (ref_path, genome)):
            with open(path, "w") as f:
                for name, s in seqs:
                    f.write(">%s\n%s\n" % (name, s))
        te_classes = {name.split("#")[0]: name.split("#")[1] for name, _s in lib}
        is_heli = lambda x: "Helitron" in LIB[x[3]][0]  # noqa: E731
        # the reader takes the flank length from the last line: once a transposon last (the order of the records), once a Helitron
        for label, order in (("transposon last", recs), ("helitron last", [x for x in recs if not is_heli(x)] + [x for x in recs if is_heli(x)])):
            gff_path = os.path.join(d, "annot.gff")
            util.write_repeatmasker_gff(order, [n for n, _s in genome], [n for n, _s in lib], gff_path)
            copies, flank, annotations = ref.get_full_length_copies_from_gff_v1(lib_path, ref_path, gff_path, 0.95, te_classes)
            out["variants"].append({"label": label, "records": order, "gff": open(gff_path).read(), "full_length_copies": copies,
                                    "flank_full_length_copies": flank, "full_length_annotations": annotations})
    path = os.path.join(ROOT, "tests", "golden", "annotate_gff.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(out, sort_keys=False).encode())
    n_full = [sum(len(v) for v in var["full_length_annotations"].values()) for var in out["variants"]]
    print("wrote %s: %d records, %s full-length copies, %d bytes" % (path, len(recs), n_full, os.path.getsize(path)))


if __name__ == "__main__":
    main()
