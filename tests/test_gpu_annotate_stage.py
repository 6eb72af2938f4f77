"""GPU: the two drop-in scripts of the annotation (hite_amd/scripts/annotate_genome.py, pan_annotate_genome.py) end to end on the
miniature genome of tests/test_annotate_files.py with HITE_ANNOTATOR=gpu, each as the process the pipeline starts: the files exist and
parse, the .out and the .gff carry the same records, <genome_name>.full_length.gff lists every planted full-length copy, and the
records are the twin's."""
import os
import subprocess
import sys

import pytest

import annotate_twin as AT
from hite_amd import util
from test_annotate_files import check_annotation_files, check_full_length, miniature

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(script, args):
    env = dict(os.environ, HITE_ANNOTATOR="gpu")
    subprocess.run([sys.executable, os.path.join(ROOT, "hite_amd", "scripts", script)] + args, check=True, env=env, timeout=120)


def _twin_lines(lib_path, ref_path):
    ref_names, ref = util.read_fasta(ref_path)
    lib_names, lib = util.read_fasta(lib_path)
    recs, _status = AT.annotate([ref[n] for n in ref_names], [lib[n] for n in lib_names])
    return (util.repeatmasker_out_lines(recs, ref_names, [len(ref[n]) for n in ref_names], lib_names, [len(lib[n]) for n in lib_names]),
            util.repeatmasker_gff_lines(recs, ref_names, lib_names))


def test_annotate_genome_script(tmp_path):
    lib_path, ref_path, _planted = miniature(tmp_path)
    out_dir = tmp_path / "out"
    _run("annotate_genome.py", ["-t", "4", "--classified_TE_consensus", lib_path, "--tmp_output_dir", str(out_dir), "--annotate", "1", "-r", ref_path,
                                "-w", str(tmp_path)])
    assert sorted(f for f in os.listdir(out_dir) if f.startswith("HiTE.")) == ["HiTE.gff", "HiTE.out", "HiTE.tbl"]
    check_annotation_files(str(out_dir / "HiTE.out"), str(out_dir / "HiTE.gff"), str(out_dir / "HiTE.tbl"), 6)
    out_lines, gff_lines = _twin_lines(lib_path, ref_path)
    assert open(out_dir / "HiTE.out").readlines() == out_lines and open(out_dir / "HiTE.gff").readlines() == gff_lines
    assert "HiTE.cat.gz" in open(out_dir / "HiTE_annotate_genome.log").read()


def test_pan_annotate_genome_script(tmp_path):
    lib_path, ref_path, planted = miniature(tmp_path)
    out_dir = tmp_path / "pan"
    _run("pan_annotate_genome.py", ["--panTE_lib", lib_path, "--reference", ref_path, "--genome_name", "g1", "--annotate", "1", "--threads", "4",
                                    "--output_dir", str(out_dir), "-w", str(tmp_path)])
    assert sorted(f for f in os.listdir(out_dir) if f.startswith("g1.")) == ["g1.full_length.copies", "g1.full_length.gff", "g1.gff", "g1.out", "g1.tbl"]
    assert not [f for f in os.listdir(out_dir) if f.startswith("HiTE.") or f.endswith(".tmp")]
    check_annotation_files(str(out_dir / "g1.out"), str(out_dir / "g1.gff"), str(out_dir / "g1.tbl"), 6)
    assert open(out_dir / "g1.gff").readlines() == _twin_lines(lib_path, ref_path)[1]
    check_full_length(str(out_dir), "g1", planted, ref_path)
