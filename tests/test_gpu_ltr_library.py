"""GPU: util.ltr_library, genome in and LTR library out, on the genome of planted families: through the real context (the scan, the
pair search, the clustering of frames, the frame vote and the full-length copy support on the device) it writes the same files as the
same call with the CPU twins in their place."""
import os

import pytest

import framecluster_twin as FT
import ltrcopy_twin as CT
import ltrscan_twin as LT
import oracle_lib as O
import pairhsp_twin as PT
from conftest import load_golden

pytestmark = pytest.mark.gpu
FILES = ("msa_flank.txt", "intact_LTR_homo.txt", "filtered_single_copy_LTRs.txt", "confident_ltr.scn", "intact_LTR.list", "intact_LTR.fa",
         "confident_ltr.terminal.fa", "confident_ltr.internal.fa", "confident_ltr.fa")


def frame_vote(matrices, flank, window, side):
    return [O.ltr_frame(list(rows), flank, window, side) for rows in matrices]


def test_device_equals_twins_file_for_file(tmp_path, monkeypatch):
    from hite_amd import util

    monkeypatch.delenv("HITE_FILTR_DIR", raising=False)
    gold = load_golden("ltr_library")
    names = list(gold["contigs"])
    contigs = [gold["contigs"][n] for n in names]
    ref = str(tmp_path / "genome.fa")
    util.store_fasta(gold["contigs"], ref)
    ctx = util.set_reference(ref)
    seconds, calls = {}, []

    def support(elements, std, cover, thr):
        calls.append(len(elements))
        return CT.support(contigs, elements, std, cover, thr)

    paths = util.ltr_library(ref, str(tmp_path / "gpu"), ctx=ctx, seconds=seconds)
    ctx = util.set_reference(ref)          # (the de-duplication of the library packed the library in the genome's place)
    paths_t = util.ltr_library(ref, str(tmp_path / "twin"), ctx=ctx, scan=LT.scan_array, hsps=PT.pair_hsps, cluster=FT.frame_cluster,
                               frame_vote=frame_vote, support=support)
    assert set(paths) == set(util.LTR_LIBRARY_FILES) == set(paths_t) and len(calls) == 1 and calls[0] >= 4
    for name in FILES:
        got = open(os.path.join(str(tmp_path), "gpu", name), "rb").read()
        assert got == open(os.path.join(str(tmp_path), "twin", name), "rb").read(), name
        assert got or name == "filtered_single_copy_LTRs.txt", name
    assert {"scan", "copy_support", "single_copy", "sequences", "library"} <= set(seconds)
    # something is kept by its copies, and the list has the twelve columns of the reference's
    homo = dict(ln.split("\t") for ln in open(os.path.join(str(tmp_path), "gpu", "intact_LTR_homo.txt")).read().splitlines())
    assert sum(v == "1" for v in homo.values()) >= 1
    rows = [ln.split("\t") for ln in open(paths["intact_LTR.list"]).read().splitlines()]
    assert len(rows) >= 1 and all(len(r) == 12 and r[1] == "pass" for r in rows)
    lib_names, _ = util.read_fasta(paths["confident_ltr.fa"])
    assert lib_names and all("LTR" in n for n in lib_names)
