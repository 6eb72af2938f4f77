"""GPU: util.ltr_detect, genome in and is_LTR table out, on the genome of 32 planted elements: through the real context (the scan,
the pair search, the clustering of frames and the frame vote on the device) it writes the same files and returns the same table as
the same call with the CPU twins in their place."""
import os

import pytest

import framecluster_twin as FT
import ltrscan_cases as LC
import ltrscan_twin as LT
import oracle_lib as O
import pairhsp_twin as PT

pytestmark = pytest.mark.gpu
FILES = ("total.scn", "remove_recomb.scn", "filter_terminal_align.scn", "all_potential_ltr.json", "confident_ltr.scn")


def frame_vote(matrices, flank, window, side):
    return [O.ltr_frame(list(rows), flank, window, side) for rows in matrices]


def test_device_equals_twins_file_for_file(tmp_path):
    from hite_amd import util

    names, seqs, truth, places = LC.planted()
    ref = str(tmp_path / "genome.fa")
    util.store_fasta(dict(zip(names, seqs)), ref)
    ctx = util.set_reference(ref)
    seconds = {}
    conf, table = util.ltr_detect(ref, str(tmp_path / "gpu"), ctx=ctx, seconds=seconds)
    conf_t, table_t = util.ltr_detect(ref, str(tmp_path / "twin"), ctx=ctx, scan=LT.scan_array, hsps=PT.pair_hsps, cluster=FT.frame_cluster,
                                      frame_vote=frame_vote)
    for name in FILES:
        got = open(os.path.join(str(tmp_path), "gpu", name), "rb").read()
        assert got == open(os.path.join(str(tmp_path), "twin", name), "rb").read() and got, name
    assert table == table_t and os.path.basename(conf) == "confident_ltr.scn" and conf != conf_t
    assert {"scan", "recombination", "flank_align", "copies"} <= set(seconds)
    total = open(os.path.join(str(tmp_path), "gpu", "total.scn")).read().splitlines()
    assert total[0].startswith("#") and len(total) == 1 + 41
    # the confident lines are lines of filter_terminal_align.scn whose left terminal the flank filter kept
    final = open(os.path.join(str(tmp_path), "gpu", "filter_terminal_align.scn")).read().splitlines()
    kept = open(conf).read().splitlines()
    assert set(kept) <= set(final) and len(kept) == sum(v[0] for v in table.values()) and len(table) >= 20
