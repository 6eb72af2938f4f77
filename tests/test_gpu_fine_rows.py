"""The front of a fine-stage pass on the device (hite_amd/csrc/hite_pipeline.hip: select_rows_kernel, row_meta_kernel,
row_gather_kernel with emit_padded, emit_span / emit_span4, clip_probe_kernel) at the limits of its own code, through hite_fine_rows --
which runs the launches of the stage itself -- and hite_clip_probe, against the twin (tests/oracle_pipeline.py: pass_rows, the rows
fine_stage_candidate judges) on the tables of tests/fine_row_cases.py: the same check_* functions that test_fine_row_cases.py runs with
the twin in the device's place, where every case is also shown to reach its limit.  Rows, their order, the truncation flag, the
lengths and every window byte, both passes: exact equality.
   * select_rows_kernel: 0 .. 513 copies with windows that do not exist between them, exactly 100 and 101 eligible, rows on both sides
     of the chunks of 256; window lengths 99 / 100 / 1000 / 1001; more than 100 equal lengths, where the name alone decides (decimal
     strings of different digit counts, one start with several ends, both strands, a record given twice, contigs whose name order is
     not the packing order, with and without the order set);
   * row_meta_kernel: 0, 1, 4, 5 rows per call, an empty last candidate; rows, window bytes and the longest row, also as the stage
     reports them in its stats;
   * row_gather_kernel: every length 100 .. 163 and 1023 .. 1041 on both strands, windows at genome position 0, at the last base and
     at the first base of a later contig, runs of N of 1 .. 33 bases at every offset of a 32-base word, the first500 + last500 form;
   * emit_padded: front and back pads 0 .. 17, 31 .. 33 on all four strand combinations, a centre with clips of its own, pads past
     the centre's end, a centre of N, pads of 499 / 500 / 501 under the first500 + last500 form;
   * clip_probe_kernel: the lengths around 21 and 42, 5 / 6 mismatches, ties, the second attempt, the offset bounds, N and lower
     case, the fall-back and its clamps, contig ends, record counts around a block of 256 threads; the probed words as pads;
   * every candidate alone and the batch reversed; the stage's answers on a thinned set; the consensus pool at its cap."""
import ctypes as C

import numpy as np
import pytest

import fine_row_cases as FR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import hite_amd

    c = hite_amd.Context(0)
    yield c
    c.close()


def test_select_rows(ctx):
    FR.check_select(ctx)


def test_length_ties_follow_the_names(ctx):
    FR.check_ties(ctx)


def test_row_slots_and_totals(ctx):
    FR.check_slots(ctx)


def test_stage_stats_are_the_totals(ctx):
    FR.check_stage_stats(ctx)


def test_stage_stats_of_pass_b(ctx):
    FR.check_stage_stats_passing(ctx)


@pytest.mark.parametrize("name", FR.gather_names())
def test_gather(ctx, name):
    FR.check_gather(ctx, name)


@pytest.mark.parametrize("name", FR.pad_names())
def test_pads(ctx, name):
    FR.check_pads(ctx, name)


def test_clip_probe(ctx):
    FR.check_probe(ctx)


@pytest.mark.parametrize("part", range(3))
def test_candidates_are_independent(ctx, part):
    FR.check_independence(ctx, part, 3)


@pytest.mark.parametrize("te_type", ("tir", "helitron", "non_ltr"))
def test_stage_on_the_row_cases(ctx, te_type):
    assert 6 <= FR.check_end_to_end(ctx, te_type) <= 12


def _stage(ctx, cands, copies, cap):
    """hite_flank_region_align_clip itself, with the consensus pool the caller sizes"""
    from hite_amd._lib import CALL_DTYPE, _arr, _p

    n = len(cands)
    cb = [c.encode() for c in cands]
    coff = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(c) for c in cb], out=coff[1:])
    cbuf = np.frombuffer(b"".join(cb) + b"\0" * 16, dtype=np.uint8)
    cf = np.zeros(n + 1, dtype=np.int32)
    np.cumsum([len(c) for c in copies], out=cf[1:])
    flat = [t for c in copies for t in c]
    calls = np.zeros(n, dtype=CALL_DTYPE)
    cons = np.zeros(cap + 16, dtype=np.uint8)
    stats = np.zeros(12, dtype=np.int64)
    rc = ctx.lib.hite_flank_region_align_clip(ctx.h, 0, 1, n, _p(cbuf), _p(coff), _p(cf), C.c_int64(len(flat)), _p(_arr([t[0] for t in flat], np.int32)),
                                              _p(_arr([t[1] for t in flat], np.int64)), _p(_arr([t[2] for t in flat], np.int64)),
                                              _p(_arr([t[3] for t in flat], np.uint8)), None, 50, _p(calls), _p(cons), C.c_int64(cap), _p(stats))
    return rc, calls, cons, stats


def test_consensus_pool_at_its_cap(ctx):
    """cons_cap = the need (stats[10]): the calls and bytes of a generous cap; one byte less: HITE_ECAP, and stats[10] still says the need"""
    from hite_amd._lib import INFO

    t = FR.cons_pool_table()
    ctx.genome_pack(t["contigs"])
    ctx._fine_row_genome = None
    rc, calls, cons, stats = _stage(ctx, t["cands"], t["copies"], 1 << 20)
    need = int(stats[10])
    assert rc == 0 and need > 0 and need == int(sum(c["cons_len"] for c in calls if c["is_te"]))
    got = [[bool(c["is_te"]), INFO[int(c["info"])], cons[c["cons_off"]:c["cons_off"] + c["cons_len"]].tobytes().decode() if c["is_te"] else "",
            int(c["row_num"])] for c in calls]
    assert got == t["expect"]
    rc1, calls1, cons1, stats1 = _stage(ctx, t["cands"], t["copies"], need)
    assert rc1 == 0 and calls1.tobytes() == calls.tobytes() and cons1[:need].tobytes() == cons[:need].tobytes() and list(stats1) == list(stats)
    rc2, _calls2, _cons2, stats2 = _stage(ctx, t["cands"], t["copies"], need - 1)
    assert rc2 == -4 and int(stats2[10]) == need
