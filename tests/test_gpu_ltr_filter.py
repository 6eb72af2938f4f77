"""GPU: the LTR flank filter (util.ltr_flank_filter; FiLTR's step 3, bin/FiLTR-main/src/LTR_filter.py:44-170) on a miniature genome
(450 kbp, hite_amd/synth.py::make_ltr_flank_genome) with four kinds of planted family --
  (a) LTR terminals whose copies sit in random flanks, with 3 and with 12 copies: kept, as low and as high copy;
  (b) terminals cut out of the middle of a longer repeat (both flanks homologous across the copies): dropped by the sort rule;
  (c) one flank homologous, the other random: dropped by the sort rule;
  (d) a single-copy terminal: dropped by the sort rule (one row)
-- against the same function driven through the twins (tests/framecluster_twin.py for the clustering, the oracle for the frame
vote) on the same alignments, and the wrappers under the reference's names on `.matrix` directories against the driver."""
import os

import pytest

import framecluster_twin as T
import oracle_lib as O
from hite_amd import synth, util

pytestmark = pytest.mark.gpu

PLAN = [("ltr", 3), ("ltr", 12), ("ltr", 4), ("ltr", 7), ("inner", 8), ("inner", 3), ("left", 8), ("right", 8), ("left", 20), ("ltr", 1)]
FLANK = 100


def frame_vote(matrices, flank, window, side):
    return [O.ltr_frame(list(rows), flank, window, side) for rows in matrices]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """the genome and the terminal sequences as FASTA files, the genome resident in util's context, the frames computed once"""
    d = tmp_path_factory.mktemp("ltr_filter")
    g = synth.make_ltr_flank_genome(PLAN, seed=5)
    ref, cand = str(d / "genome.fa"), str(d / "terminals.fa")
    util.store_fasta({"chr_%d" % k: c for k, c in enumerate(g["contigs"])}, ref)
    util.store_fasta(g["terminals"], cand)
    ctx = util.set_reference(ref)
    frames, full = util.ltr_terminal_frames(g["terminals"], ref, FLANK, ctx=ctx)
    return dict(g=g, ref=ref, cand=cand, ctx=ctx, frames=frames, full=full, dir=d)


def test_frames_of_every_family(world):
    g, frames = world["g"], world["frames"]
    for n in g["names"]:
        assert n in frames and len(frames[n]) == g["copies"][n], (n, len(frames.get(n, ())))
        assert all(len(left) == FLANK and len(right) == FLANK for left, right in frames[n])


def test_device_equals_twins_on_the_same_alignments(world):
    frames = world["frames"]
    got = util.ltr_flank_decide(frames, FLANK, ctx=world["ctx"])
    assert got == util.ltr_flank_decide(frames, FLANK, cluster=T.frame_cluster, frame_vote=frame_vote)
    # each half on its own: the device's clustering under the oracle's vote, the twin's clustering under the device's vote
    assert got == util.ltr_flank_decide(frames, FLANK, cluster=world["ctx"].frame_cluster, frame_vote=frame_vote)
    assert got == util.ltr_flank_decide(frames, FLANK, cluster=T.frame_cluster, frame_vote=world["ctx"].ltr_frame)


def test_planted_families(world):
    g = world["g"]
    seconds = {}
    table, high = util.ltr_flank_filter(world["cand"], world["ref"], FLANK, ctx=world["ctx"], seconds=seconds)
    assert (table, high) == util.ltr_flank_decide(world["frames"], FLANK, cluster=T.frame_cluster, frame_vote=frame_vote)
    assert list(table) == g["names"]
    for n in g["names"]:
        kind, copies = g["kind"][n], g["copies"][n]
        if kind == "ltr" and copies > 1:
            assert table[n] == (True, "low" if copies <= 5 else "high", None), (n, table[n])
        else:
            assert table[n] == (False, None, "sort"), (n, table[n])
    assert sorted(high) == sorted(n for n in g["names"] if g["kind"][n] == "ltr" and g["copies"][n] > 5)
    assert sorted(seconds) == ["both_ends", "cluster_joined", "cluster_left", "cluster_right", "copies", "frame_vote", "msa", "windows"]
    nowhere = synth.make_ltr_flank_genome([("ltr", 1)], genome_bp=150_000, seed=77)["terminals"]        # of another genome
    assert util.ltr_flank_filter(nowhere, world["ref"], FLANK, ctx=world["ctx"])[0] == {"ltr_1_0": (False, None, "frames")}


def test_directory_wrappers_write_the_same_table(world):
    """the reference's sequence of calls (LTR_filter.py:66-170 without the deep model)"""
    d = {k: str(world["dir"] / k) for k in ("tmp", "frames", "full", "sort", "keep", "low", "high")}
    util.generate_both_ends_frame_from_seq_minimap2(world["cand"], world["ref"], FLANK, 1, d["tmp"], d["frames"], d["full"], 100)
    assert util._read_matrix_dir(d["frames"]) == {n: [tuple(r) for r in m] for n, m in world["frames"].items()}
    for n, rows in world["full"].items():
        assert open(os.path.join(d["full"], n + ".matrix")).read().split("\n")[:-1] == rows
    n_in, n_keep = util.sort_matrix_dir(d["frames"], d["sort"], d["tmp"], 1)
    util.filter_ltr_by_flanking_cluster(d["sort"], d["keep"], d["tmp"], 1, None)
    util.get_low_copy_LTR(d["keep"], d["low"], 1, copy_num_threshold=5)
    util.get_high_copy_LTR(d["keep"], d["high"], 1, copy_num_threshold=5)
    lc, hc = str(world["dir"] / "is_LTR_homo.lc.txt"), str(world["dir"] / "is_LTR_homo.hc.txt")
    util.judge_ltr_from_both_ends_frame(d["low"], lc, 1, "Low copy", FLANK, None)
    util.judge_ltr_from_both_ends_frame(d["high"], hc, 1, "High copy", FLANK, None)
    got = {}
    for path, label in ((lc, "low"), (hc, "high")):
        for line in open(path):
            name, flag = line.split()
            got[name] = (flag == "1", label)
    table, high = util.ltr_flank_decide(world["frames"], FLANK, ctx=world["ctx"])
    assert got == {n: (v[0], v[1]) for n, v in table.items() if v[1] is not None}
    assert (n_in, n_keep) == (len(world["frames"]), sum(1 for v in table.values() if v[2] != "sort"))
    assert util._read_matrix_dir(d["high"]) == {n: [tuple(r) for r in m] for n, m in high.items()}
