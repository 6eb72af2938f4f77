#!/usr/bin/env python
"""Drop-in for panHiTE's module/pan_annotate_genome.py (same argv, module/pan_annotate_genome.py:84-93; same files):

  <output_dir>/<genome_name>.gff  .tbl  .out       the annotation of --reference with --panTE_lib, when --annotate is 1
  <output_dir>/<genome_name>.full_length.copies    JSON {entry: {"seq:start-end": bases}} of the full-length copies
  <output_dir>/<genome_name>.full_length.gff       one line per full-length copy, by sequence and start (lines 36-80 there)

RepeatMasker runs when it is installed; otherwise, or with HITE_ANNOTATOR=gpu, the build's own annotation (Context.annotate;
include/hite_gpu.h, "genome annotation": parity with RepeatMasker unpinned).  The full-length copies come from the GFF through
util.get_full_length_copies_from_gff_v1, the restated reader of the reference.  Every file is written under a temporary name and
renamed."""
import argparse
import json
import logging
import os
import shutil
import sys
from datetime import datetime, timezone

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from hite_amd import util  # noqa: E402


def build_parser():
    p = argparse.ArgumentParser(description="panHiTE annotate genome.")
    p.add_argument("--panTE_lib", type=str)
    p.add_argument("--reference", type=str)
    p.add_argument("--genome_name", type=str)
    p.add_argument("--annotate", type=int, default=1)
    p.add_argument("--threads", type=int, default=1)
    p.add_argument("--output_dir", nargs="?", default=os.getcwd())
    p.add_argument("-w", "--work_dir", nargs="?", default="/tmp")
    return p


def run_annotation(output_dir, threads, panTE_lib, reference, annotate, genome_name, log, ctx=None, annot=None):
    """run_repeat_masker (pan_annotate_genome.py:26) with the in-tree stage beside the tool"""
    if annotate != 1:
        return
    stem = os.path.join(output_dir, genome_name)
    util.annotate_genome(output_dir, panTE_lib, reference, annotate, threads, log, ctx=ctx, annot=annot)
    for suffix in ("gff", "tbl", "out"):
        shutil.copyfile(os.path.join(output_dir, "HiTE." + suffix), stem + "." + suffix + ".tmp")
        os.replace(stem + "." + suffix + ".tmp", stem + "." + suffix)
        os.remove(os.path.join(output_dir, "HiTE." + suffix))
    te_classes, _contigs = util.get_TE_class(panTE_lib)
    copies, _flank, annotations = util.get_full_length_copies_from_gff_v1(panTE_lib, reference, stem + ".gff", 0.95, te_classes)
    util._publish(stem + ".full_length.copies", [json.dumps(copies)])
    header = ["##gff-version 3\n", "##date %s\n" % datetime.now(timezone.utc).strftime("%Y-%m-%d %H:%M:%S UTC")]
    util._publish(stem + ".full_length.gff", header + util.full_length_gff_lines(annotations))


def main(argv=None):
    a = build_parser().parse_args(argv)
    out_dir = os.path.abspath(a.output_dir)
    os.makedirs(out_dir, exist_ok=True)
    logging.basicConfig(filename=os.path.join(out_dir, "panHiTE.log"), level=logging.DEBUG)
    run_annotation(out_dir, a.threads, os.path.abspath(a.panTE_lib), os.path.abspath(a.reference), a.annotate, a.genome_name,
                   logging.getLogger("pan_annotate_genome"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
