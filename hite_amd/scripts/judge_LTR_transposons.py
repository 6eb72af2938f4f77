#!/usr/bin/env python
"""Drop-in for HiTE's module/judge_LTR_transposons.py (the argv main.py:673-679 builds): the LTR stage, genome in and, in
<tmp_output_dir>, intact_LTR.list, intact_LTR.fa, intact_LTR.fa.classified, confident_ltr.terminal.fa, confident_ltr.internal.fa,
confident_ltr_cut.fa and filtered_single_copy_LTRs.txt out.

As the reference does (run_judge_LTR_detection, :98-302): the genome is renamed (chr_0, chr_1, ...; chr_name.map), the transposons
of --prev_TE are masked in it (util.mask_genome_intactTE), FiLTR runs on the result -- here util.ltr_library, the in-tree stages on
the MI355X -- its library becomes confident_ltr_cut.fa, the labels of the classified intact elements are given to the three
libraries (assign_label_to_lib) and added to the list.  Every file is published through a temporary name and a rename.

Not part of this build, and said on stderr when it matters:
  --use_FiLTR 0, the LTR_retriever branch (LTR_harvest, LTR_FINDER, LTR_retriever): exits 2;
  the classification (NeuralTE's models, TEClass): --classified FILE (an extension of this build: a FASTA whose names are
  <chr>:<start>..<end>#<label>, what either classifier leaves in intact_LTR.fa.classified) gives the labels; without it every
  element is LTR/Unknown, and intact_LTR.fa.classified is written with that label."""
import argparse
import csv
import os
import shutil
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _stage  # noqa: E402,F401
from _stage import util  # noqa: E402

OUTPUTS = ("confident_ltr.terminal.fa", "confident_ltr.internal.fa", "confident_ltr_cut.fa", "intact_LTR.list", "intact_LTR.fa",
           "filtered_single_copy_LTRs.txt")
UNKNOWN = "LTR/Unknown"


def build_parser():
    p = argparse.ArgumentParser(description="run HiTE LTR module on the MI355X path")
    p.add_argument("-g"); p.add_argument("-t", type=int, default=1); p.add_argument("--tmp_output_dir")
    p.add_argument("--recover", type=int, default=0); p.add_argument("--use_FiLTR", type=int, default=1)
    p.add_argument("--use_NeuralTE", type=int, default=1); p.add_argument("--miu", default="1.3e-8"); p.add_argument("--is_wicker", default="0")
    p.add_argument("--is_output_lib", type=int, default=1); p.add_argument("--debug", type=int, default=0)
    p.add_argument("-w", "--work_dir", nargs="?", default="/tmp"); p.add_argument("--prev_TE", default=None)
    p.add_argument("--classified", default=None, help="labels of the intact elements: FASTA with <chr>:<start>..<end>#<label> names -- extension of this build")
    return p


def publish(src, dst):
    """copy under a temporary name, then rename: the file is there whole or not at all"""
    tmp = dst + ".tmp"
    shutil.copy(src, tmp)
    os.replace(tmp, dst)


def add_labels_to_list(ltr_list, labels):
    """judge_LTR_transposons.py:286-302: the label of every element before the last column of the list ('NA' when it has none)"""
    temp_file = ltr_list + ".temp.tsv"
    with open(ltr_list, "r") as infile, open(temp_file, "w", newline="") as outfile:
        writer = csv.writer(outfile, delimiter="\t")
        for row in csv.reader(infile, delimiter="\t"):
            if not row[0].startswith("#"):
                writer.writerow(row[:-1] + [labels.get(row[0], "NA")] + row[-1:])
    os.replace(temp_file, ltr_list)


def run(a, work, library=None):
    """the stage in directory work; library: replaces util.ltr_library (the tests pass one with the twins in place of the device)"""
    ref_rename_path, chr_name_map = os.path.join(work, "genome.rename.fa"), os.path.join(work, "chr_name.map")
    util.rename_reference(a.g, ref_rename_path, chr_name_map)
    if a.prev_TE and os.path.exists(a.prev_TE) and util.read_fasta(a.prev_TE)[0]:
        util.set_reference(ref_rename_path)
        ref_rename_path = util.mask_genome_intactTE(a.prev_TE, ref_rename_path, os.path.join(work, "mask"), a.t, 0, a.debug)
    else:
        shutil.copy(ref_rename_path, ref_rename_path + ".masked")
        ref_rename_path += ".masked"
    out_dir = os.path.join(work, "FiLTR_output")
    paths = (library or util.ltr_library)(ref_rename_path, out_dir, miu=float(a.miu), is_output_lib=a.is_output_lib, threads=a.t, debug=a.debug)
    final = {name: os.path.join(work, name) for name in OUTPUTS}
    for name in OUTPUTS:
        src = paths["confident_ltr.fa" if name == "confident_ltr_cut.fa" else name]
        if os.path.exists(src):
            shutil.copy(src, final[name])
    if not os.path.exists(final["confident_ltr_cut.fa"]):
        sys.stderr.write("judge_LTR_transposons (MI355X path): no LTR library (is_output_lib 0, or no LTR retrotransposon in the genome)\n")
        open(final["confident_ltr_cut.fa"], "w").close()
    classified = final["intact_LTR.fa"] + ".classified"
    names, contigs = util.read_fasta(final["intact_LTR.fa"])
    labels = {}
    if a.classified:
        for name in util.read_fasta(a.classified)[0]:
            parts = name.split("#")
            labels[parts[0]] = parts[1]
        shutil.copy(a.classified, classified)
    else:
        if names:
            sys.stderr.write("judge_LTR_transposons (MI355X path): the intact LTR elements are NOT classified (NeuralTE / TEClass are not "
                             "part of this build; --classified FILE gives their labels): all %d are %s\n" % (len(names), UNKNOWN))
        labels = {n: UNKNOWN for n in names}
        util.store_fasta({n + "#" + UNKNOWN: contigs[n] for n in names}, classified)
    for n in names:
        labels.setdefault(n, UNKNOWN)
    for name in ("confident_ltr_cut.fa", "confident_ltr.terminal.fa", "confident_ltr.internal.fa"):
        util.assign_label_to_lib(final[name], labels)
    add_labels_to_list(final["intact_LTR.list"], labels)
    return list(final.values()) + [classified, chr_name_map]


def main(argv=None, library=None):
    a = build_parser().parse_args(argv)
    if not a.use_FiLTR:
        sys.stderr.write("judge_LTR_transposons (MI355X path): --use_FiLTR 0, the LTR_retriever branch (LTR_harvest, LTR_FINDER, LTR_retriever), "
                         "is not part of this build\n")
        return 2
    out_dir = os.path.abspath(a.tmp_output_dir or os.getcwd())
    os.makedirs(out_dir, exist_ok=True)
    if a.recover and all(os.path.exists(os.path.join(out_dir, n)) for n in OUTPUTS):
        return 0
    a.g = os.path.realpath(a.g)
    os.makedirs(os.path.abspath(a.work_dir), exist_ok=True)
    work = tempfile.mkdtemp(prefix="judge_LTR_transposons_", dir=os.path.abspath(a.work_dir))
    try:
        for path in run(a, work, library):
            publish(path, os.path.join(out_dir, os.path.basename(path)))
    finally:
        if not a.debug:
            shutil.rmtree(work, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
