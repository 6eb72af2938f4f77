"""The genomes of tests/seed_limit_cases.py on the CPU: every case reaches the limit it is named for (the builders assert it with
the model), the model's records are the twin's (oracle/hite_oracle_copies.c: orc_seed_allvsall) and the closed forms', the sharded
twin partitions every table, and the case set as a whole contains every event of the run, wavefront, contig-cache, anchor-tile and
piece limits (test_coverage).  tests/test_gpu_seed_limits.py runs the same checks with the device in the twin's place."""
import pytest

import oracle_lib as O
import seed_limit_cases as SC
from oracle_ctx import OracleCtx

SHARD_WORLDS = (2, 3, 7)
# the sharded twin runs on the shard-edge cases and on one case of every other group (the 10^6 anchors of the 1000-entry run once)
SHARD_CASES = SC.names("shards") + ["run_straddles_tile", "border_inv_3", "cluster_starts_at_2047", "anchors_one_per_share",
                                    "anchors_2049_in_share", "piece_query_and_subject_border", "two_copies_inverted"]


@pytest.fixture(scope="module")
def twin():
    return OracleCtx()


@pytest.mark.parametrize("name", SC.names())
def test_model_is_the_twin(twin, name):
    """the builder's own assertions, then model records == twin records and segment table == orc_seed_segments"""
    c, m = SC.get(name), SC.model_of(name)
    exp = O.seed_allvsall(c["contigs"], seg_len=c["seg_len"])
    SC.same_table(SC.table(m), exp, name)
    assert list(exp["seg_chrom"]) == m["seg_chrom"] and list(exp["seg_off"]) == m["seg_off"]
    SC.check_case(twin, name, stats=False)


def test_closed_forms():
    n = sum(SC.check_closed_form(name) for name in SC.names())
    assert n >= 8, n


@pytest.mark.parametrize("world", SHARD_WORLDS)
@pytest.mark.parametrize("name", SHARD_CASES)
def test_sharded_twin(twin, name, world):
    SC.check_shares(twin, name, world, stats=False)


@pytest.mark.parametrize("name", sorted(SC.DEGENERATE))
def test_degenerate(name):
    contigs, m = SC.degenerate(name)
    exp = O.seed_allvsall(contigs, seg_len=1_000_000)
    SC.same_table(SC.table(m), exp, name)


def test_segment_guard_genome():
    for extra in (0, 1):
        contigs = SC.guard_genome(extra)
        sc, so = SC.segments(contigs, 1_000_000)
        assert len(sc) == SC.MAXSEG + extra
    m = SC.guard_model()
    exp = O.seed_allvsall(SC.guard_genome(0), seg_len=1_000_000)
    SC.same_table(SC.table(m), exp, "guard")
    assert len(m["records"]) == 2 and all(r[0] == r[1] == SC.MAXSEG - 1 for r in m["records"])


def test_shard_edge_is_the_twins():
    """the restated edge formula gives the twin's shares: a share's records are the unsharded records of its diagonals (checked by
    test_sharded_twin); here: monotone edges, multiples of 64, the ends"""
    for G in (1, 63, 3034, 40_000, 1 << 30):
        for world in (2, 3, 7, 256):
            e = [SC.shard_edge(G, k, world) for k in range(world + 1)]
            assert e[0] == 0 and e[-1] == 4 * G + 64 and all(a <= b for a, b in zip(e, e[1:]))
            assert all((x - (2 * G if x >= 2 * G else 0)) % 64 == 0 for x in e[1:-1])


def test_coverage():
    """no event of the run / wavefront / contig-cache / anchor-tile / piece limits is missing from the case set"""
    cov = SC.coverage()
    missing = [e for e in SC.REQUIRED if cov.get(e, 0) == 0]
    assert not missing, missing
