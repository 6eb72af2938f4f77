"""CPU-only: the host layer of the LTR candidate scan -- the `.scn` lines util.ltr_candidate_scan writes (against a hand-written
expectation and util.read_scn), and util.ltr_detect end to end with the twins as callables: the scan and the pair search through
their twins; the flank stage (util.ltr_flank_filter), whose copy finder and star alignment exist on the device only, is replaced by
a rule on the names, so that what is checked is the chain of files and the choice of the confident lines.  The device runs the same
chain in tests/test_gpu_ltr_detect.py."""
import os

import numpy as np

import ltrscan_cases as LC
import ltrscan_twin as LT
import pairhsp_twin as PT


def test_scn_line_format(tmp_path):
    from hite_amd import util

    recs = np.array([[1, 10, 110, 500, 603, 180, 95, 103], [0, 0, 150, 150, 300, 300, 150, 150], [1, 999, 1120, 4000, 4123, 214, 107, 123]], dtype=np.int32)
    calls = []

    def scan(seqs, **kw):
        calls.append((seqs, kw))
        return recs

    ref = {"chrB": "ACGT" * 1100, "chrA": "TTGCA" * 100}
    scn = str(tmp_path / "out.scn")
    lines = util.ltr_candidate_scan(ref, scn, scan=scan, max_ltr=3000, identity=80)
    assert calls == [([ref["chrB"], ref["chrA"]], dict(max_ltr=3000, identity=80))]
    assert lines == ["11 603 593 11 110 100 501 603 103 92.23 NA chrA",
                     "1 300 300 1 150 150 151 300 150 100.00 NA chrB",
                     "1000 4123 3124 1000 1120 121 4001 4123 123 86.99 NA chrA"]
    text = open(scn).read().splitlines()
    assert text[0].startswith("# ") and text[1:] == lines
    cands, by_index = util.read_scn(scn, None)
    assert cands == {0: ("chrA", 11, 110, 501, 603), 1: ("chrB", 1, 150, 151, 300), 2: ("chrA", 1000, 1120, 4001, 4123)}
    assert by_index == dict(enumerate(lines))
    # a FASTA path gives the same lines, in the order of the file
    fa = str(tmp_path / "ref.fa")
    util.store_fasta(ref, fa)
    assert util.ltr_candidate_scan(fa, str(tmp_path / "again.scn"), scan=scan) == lines and calls[-1][1] == {}
    assert util.ltr_candidate_scan({}, str(tmp_path / "none.scn"), scan=lambda seqs, **kw: np.zeros((0, 8), dtype=np.int32)) == []
    assert len(open(str(tmp_path / "none.scn")).read().splitlines()) == 1


def test_ltr_detect_with_the_twins(tmp_path, monkeypatch):
    from hite_amd import util

    names, seqs, truth, places = LC.planted()
    ref = str(tmp_path / "genome.fa")
    util.store_fasta(dict(zip(names, seqs)), ref)
    seen = {}

    def flank_filter(terminals, reference, flanking_len=100, max_copy_num=100, ctx=None, cluster=None, frame_vote=None, seconds=None):
        seen.update(terminals=dict(terminals), reference=reference, flank=flanking_len, cluster=cluster, frame_vote=frame_vote)
        return {n: (int(n.split("-")[1]) % 2 == 0, "low", None) for n in terminals}, {}

    monkeypatch.setattr(util, "ltr_flank_filter", flank_filter)
    seconds = {}
    conf, table = util.ltr_detect(ref, str(tmp_path / "out"), flanking_len=80, scan=LT.scan_array, hsps=PT.pair_hsps, cluster="c", frame_vote="v",
                                  seconds=seconds)
    out = str(tmp_path / "out")
    total = open(os.path.join(out, "total.scn")).read().splitlines()
    assert total[1:] == util.ltr_scn_lines(LT.scan(seqs), names) and len(total) == 42
    # what went into the flank stage is what the scn filter kept of the scan's own table
    final, _dirty, terminals = util.ltr_scn_filter(os.path.join(out, "total.scn"), ref, str(tmp_path / "again"), hsps=PT.pair_hsps)
    assert seen["terminals"] == terminals and seen["reference"] == ref and (seen["flank"], seen["cluster"], seen["frame_vote"]) == (80, "c", "v")
    assert open(final).read() == open(os.path.join(out, "filter_terminal_align.scn")).read()
    assert set(table) == set(terminals) and len(table) >= 26
    kept = open(conf).read().splitlines()
    assert conf == os.path.join(out, "confident_ltr.scn") and 0 < len(kept) < len(table)
    lines = open(final).read().splitlines()
    assert kept == [ln for ln in lines if int(ln.split(" ")[3]) % 2 == 0]
    assert "scan" in seconds and "flank_align" in seconds
