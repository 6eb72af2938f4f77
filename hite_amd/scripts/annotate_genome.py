#!/usr/bin/env python
"""Drop-in for HiTE's module/annotate_genome.py (same argv, module/annotate_genome.py:30-41; same files):

  <tmp_output_dir>/HiTE.out  HiTE.gff  HiTE.tbl   the annotation of -r with --classified_TE_consensus, when --annotate is 1

RepeatMasker runs when it is installed; otherwise, or with HITE_ANNOTATOR=gpu, the build's own annotation (util.annotate_genome ->
Context.annotate; include/hite_gpu.h, "genome annotation": parity with RepeatMasker unpinned, no HiTE.cat.gz).  Every file is
written under a temporary name and renamed."""
import argparse
import logging
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from hite_amd import util  # noqa: E402


def build_parser():
    p = argparse.ArgumentParser(description="run HiTE annotating genome...")
    p.add_argument("-t", metavar="threads number", default=1)
    p.add_argument("--classified_TE_consensus", metavar="classified_TE_consensus")
    p.add_argument("--tmp_output_dir", metavar="tmp_output_dir", default=None)
    p.add_argument("--annotate", metavar="annotate")
    p.add_argument("-r", metavar="reference")
    p.add_argument("-w", "--work_dir", nargs="?", default="/tmp")
    return p


def main(argv=None):
    a = build_parser().parse_args(argv)
    out_dir = os.path.abspath(a.tmp_output_dir or os.getcwd())
    os.makedirs(out_dir, exist_ok=True)
    logging.basicConfig(filename=os.path.join(out_dir, "HiTE_annotate_genome.log"), level=logging.DEBUG)
    util.annotate_genome(out_dir, os.path.abspath(a.classified_TE_consensus), os.path.abspath(a.r), a.annotate, int(a.t),
                         logging.getLogger("annotate_genome"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
