"""All-vs-all seeding on the device (hite_seed_allvsall[_dev], hite_amd/csrc/hite_copies.hip from SEED_MAXOCC down) at the limits of
its own kernels, on the genomes of tests/seed_limit_cases.py -- each shown on the CPU (test_seed_limit_cases.py) to reach the limit
it is named for.  The device's records are compared with the plain model's (and its `stats` with the model's M, na, clusters and
records), with the closed forms the cases carry, and with the CPU twin's (orc_seed_allvsall), array for array:
   * runs of the index against the tiles of seed_count2_kernel: across a tile border, first / last entry on it, 1000 entries
     eight words into either halo (10-bit fields at 999), 1001 entries, the run at entry 0 and at entry M, M <= 1024, M = 4096;
   * seed_anchor_coop_kernel: a ragged last wavefront, 64 seeds without a partner, one seed of 999 partners among 63 empty ones;
   * seed_opens: a copy across a contig border on either side and strand, the cut at each of the 8 places of a thread's row, gaps of
     300 / 301, diagonals 63 | 64;
   * the start bits per 2048 anchors: a cluster across a tile border, starts at 2048 and 2047, na = 4096, 2049, 6, 1;
   * pieces: 2 / 3 anchors, spans 59 / 60, 19 / 20 bases beside a border on either side and strand, borders of both sides in one
     loop, three segments, an HSP in the second select tile;
   * 65 535 segments work, 65 536 are an error; shares whose edge lies between two designed buckets; the auto-split; the
     device-resident form; degenerate genomes and a small `cap`;
   * everything once more in fresh processes with HITE_SEED_COUNT2=0, HITE_SEED_PACK=0 and the HITE_SEED_PLACE forms."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import seed_limit_cases as SC
from oracle_ctx import OracleCtx

pytestmark = pytest.mark.gpu

GROUPS = ("runs", "contigs", "clusters", "pieces", "shards")
# one case per group for the device-resident form and the shares (the shard-edge cases: all)
ONE_PER_GROUP = ("run_straddles_tile", "border_inv_3", "cluster_starts_at_2047", "piece_query_and_subject_border", "shard_edge_2_of_7")
SHARD_CASES = SC.names("shards") + ["run_straddles_tile", "border_inv_3", "cluster_starts_at_2047", "anchors_one_per_share",
                                    "anchors_2049_in_share", "piece_query_and_subject_border", "two_copies_inverted"]
FORMS = ({"HITE_SEED_COUNT2": "0"}, {"HITE_SEED_PACK": "0"}, {"HITE_SEED_PLACE": "1"},
         {"HITE_SEED_PLACE": "1", "HITE_SEED_PLACE_CNT": "1", "HITE_SEED_PLACE_LDS": "0", "HITE_SORT_WIDE_MIN": "2"},
         {"HITE_SEED_COUNT2": "0", "HITE_SEED_PLACE": "1"})
# a child (process start, context, every test of this file but the form test itself, cases and models loaded) was measured at 5 s,
# the file without children at 13 s: twenty times the child's time, so that only a hang reaches it
CHILD_TIMEOUT = 100


@pytest.fixture(scope="module")
def ctx():
    import hite_amd

    c = hite_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def twin():
    return OracleCtx()


@pytest.mark.parametrize("group", GROUPS)
def test_group(ctx, group):
    """records == the model's == the closed form's == the twin's; stats == (M, na, clusters, records) of the model"""
    for name in SC.names(group):
        got = SC.check_case(ctx, name)
        SC.check_closed_form(name)
        c = SC.get(name)
        SC.same_table(got, O.seed_allvsall(c["contigs"], seg_len=c["seg_len"]), (name, "twin"))


@pytest.mark.parametrize("name", ONE_PER_GROUP)
def test_device_resident_form(ctx, name):
    """coarse_stage_dev (the table never leaves the device): the intervals of fmea_chain on the host table, the same stats"""
    c, m = SC.get(name), SC.model_of(name)
    got = SC.check_case(ctx, name)
    assert len(got["qseg"]) > 0
    sc, so = ctx.seed_segments(c["seg_len"])
    oc, os_, oe = ctx.fmea_chain(got["qseg"], got["sseg"], got["qs"], got["qe"], got["ss"], got["se"], sc, so, 2000, 30000)
    (dc, ds, de), st = ctx.coarse_stage_dev(c["seg_len"], sc, so, 2000, 30000)
    assert np.array_equal(oc, dc) and np.array_equal(os_, ds) and np.array_equal(oe, de) and st == m["stats"], (name, st, m["stats"])


@pytest.mark.parametrize("world", (2, 3, 7))
def test_shares(ctx, twin, world):
    """each rank's table == the model's share == the twin's; together, in rank order and stably sorted, the whole table"""
    for name in SHARD_CASES:
        SC.check_shares(ctx, name, world, twin)


def test_auto_split(ctx):
    """max_anchors just below na: Context.seed_allvsall goes through the shares by itself and gives the same table"""
    for name in ("cluster_longer_than_a_tile", "gap_300_and_301"):
        c, m = SC.get(name), SC.model_of(name)
        ctx.genome_pack(c["contigs"])
        ctx.release_copy_index()
        got = ctx.seed_allvsall(seg_len=c["seg_len"], max_anchors=m["stats"][1] - 1)
        assert got.get("shares", 1) >= 2 and got["stats"][1] == m["stats"][1] and got["stats"][3] == m["stats"][3], (name, got["stats"])
        SC.same_table(got, SC.table(m), name)
    SC.check_case(ctx, "anchors_six")                    # the context is unsharded afterwards


def test_segment_guard(ctx):
    """65 535 segments (the 16 bits of the final sort key) work; one more is HITE_EINVAL, and the context goes on"""
    import hite_amd

    contigs, m = SC.guard_genome(0), SC.guard_model()
    ctx.genome_pack(contigs)
    ctx.release_copy_index()
    got = ctx.seed_allvsall(seg_len=1_000_000)
    SC.same_table(got, SC.table(m), "guard")
    assert tuple(got["stats"]) == m["stats"] and len(got["qseg"]) == 2 and int(got["qseg"][0]) == SC.MAXSEG - 1
    SC.same_table(got, O.seed_allvsall(contigs, seg_len=1_000_000), "guard twin")
    assert len(ctx.seed_segments(1_000_000)[0]) == SC.MAXSEG
    ctx.genome_pack(SC.guard_genome(1))
    ctx.release_copy_index()
    with pytest.raises(hite_amd.HiteError, match=r"hite_seed_allvsall failed: -1\b"):
        ctx.seed_allvsall(seg_len=1_000_000)
    SC.check_case(ctx, "anchors_six")


@pytest.mark.parametrize("name", sorted(SC.DEGENERATE))
def test_degenerate(ctx, name):
    """M = 0, M = 1, na = 0, np = 0 (na = 1: test_one_anchor_in_a_share)"""
    contigs, m = SC.degenerate(name)
    ctx.genome_pack(contigs)
    ctx.release_copy_index()
    got = ctx.seed_allvsall(seg_len=1_000_000)
    assert tuple(got["stats"]) == m["stats"] and len(got["qseg"]) == 0, (name, got["stats"], m["stats"])
    (dc, _ds, _de), st = ctx.coarse_stage_dev(1_000_000, *ctx.seed_segments(1_000_000), 2000, 30000)
    assert len(dc) == 0 and st == m["stats"]


def test_one_anchor_in_a_share(ctx):
    """na = 1 (anchors come in pairs: only a share holds one): rank 0 of 3 of anchors_one_per_share, both forms"""
    name = "anchors_one_per_share"
    c, m = SC.get(name), SC.model_of(name, (0, 3))
    assert m["stats"][1:] == (1, 1, 0)
    ctx.genome_pack(c["contigs"])
    ctx.release_copy_index()
    try:
        ctx.seed_shard(0, 3)
        got = ctx.seed_allvsall(seg_len=c["seg_len"])
        assert tuple(got["stats"]) == m["stats"] and len(got["qseg"]) == 0, got["stats"]
        (dc, _ds, _de), st = ctx.coarse_stage_dev(c["seg_len"], *ctx.seed_segments(c["seg_len"]), 2000, 30000)
        assert len(dc) == 0 and st == m["stats"]
    finally:
        ctx.seed_shard(0, 0)
    SC.check_case(ctx, name)


def test_small_cap(ctx):
    """cap below the record count: HITE_ECAP with *n_out set and nothing written behind `cap` (seen at the entry point itself:
    Context.seed_allvsall would ask again with that room by itself), then correct calls"""
    import ctypes as C

    c, m = SC.get("gap_300_and_301"), SC.model_of("gap_300_and_301")
    ctx.genome_pack(c["contigs"])
    ctx.release_copy_index()
    ctx.seed_allvsall(seg_len=c["seg_len"])                    # (the index state exists)
    nrec = len(m["records"])
    for cap in (1, nrec - 1):
        i32 = [np.full(nrec + 8, -7, dtype=np.int32) for _ in range(2)]
        i64 = [np.full(nrec + 8, -7, dtype=np.int64) for _ in range(4)]
        n, stats = C.c_int64(0), (C.c_int64 * 4)()
        rc = ctx.lib.hite_seed_allvsall(ctx.h, C.byref(ctx._copy_state), C.c_int64(c["seg_len"]), C.c_int64(1 << 30), C.c_int64(cap),
                                        *[a.ctypes.data_as(C.c_void_p) for a in i32 + i64], C.byref(n), stats)
        assert rc == -4 and n.value == nrec and tuple(stats) == m["stats"], (cap, rc, n.value, tuple(stats))      # HITE_ECAP
        assert all((a[cap:] == -7).all() for a in i32 + i64), cap
    for cap in (1, len(m["records"]) - 1, len(m["records"])):
        got = ctx.seed_allvsall(seg_len=c["seg_len"], cap=cap)
        SC.same_table(got, SC.table(m), ("cap", cap))
        assert tuple(got["stats"]) == m["stats"]
    SC.check_case(ctx, "gap_300_and_301")


def test_other_forms(tmp_path):
    """the switches are read once per process: every test above once more in a fresh process per form -- the run arrays of round 5
    (HITE_SEED_COUNT2=0), unpacked anchor records, the grouped placement of the seeds' records with both scatter forms.  The
    children load the cases and models this process has built; one after the other, and none after one that failed."""
    assert "SEED_LIMIT_MEMO" not in os.environ, "a child must not start children"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for name in SC.names():
        SC.model_of(name)
    memo = str(tmp_path / "seed_limit_memo.pickle")
    SC.dump_memo(memo)
    for extra in FORMS:
        rc = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k", "not test_other_forms"],
                            env=dict(os.environ, SEED_LIMIT_MEMO=memo, **extra), capture_output=True, text=True, cwd=root, timeout=CHILD_TIMEOUT)
        assert rc.returncode == 0, (extra, rc.stdout[-3000:] + rc.stderr[-2000:])
        assert " passed" in rc.stdout and "skipped" not in rc.stdout and "deselected" in rc.stdout, (extra, rc.stdout[-1000:])
