"""GPU parity of the pairwise aligner behind the star alignment (hite_amd/csrc/hite_align.hip), through the C ABI:
   * HIP == twin (oracle/hite_oracle_msa.c) per pair: cost, certificate, status, band, and the alignment byte for byte;
   * a CERTIFIED pair is the textbook global alignment (mismatch 1, gap 3) of oracle/hite_oracle_nw.c (cost and canonical path);
   * an uncertified pair is a valid alignment whose cost bounds the optimum from above."""
import numpy as np
import pytest

import oracle_lib as O
from align_check import check_pairs, check_pairs_once, pair_matrix  # noqa: F401  (the checker, shared with test_gpu_align_limits.py)
from test_align_oracle import make_pair, mutate, rnd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import hite_amd

    c = hite_amd.Context(0)
    yield c
    c.close()


def test_align_families_all_modes(ctx):
    """random families of 60 - 900 columns, every kernel mix at every cap.  All 160 pairs are certified by the 4-word band, so the four
    caps run the SAME work -- the 4-word forward kernels and the traceback: no wider level, no fall-back.  The caps differ only in
    the schedule around that work (at 16 and 32 the lists of the overlap path are built and found empty).  The wider levels, the
    certificate's and the schedule's thresholds and the fall-back are reached by test_gpu_align_limits.py."""
    rng = np.random.default_rng(7001)
    pairs = [make_pair(rng, int(rng.integers(60, 900))) for _ in range(160)]
    for cap in (0, 8, 16, 32):
        n_cert, n_opt, n_drop, classes = check_pairs(ctx, pairs, cap)
        assert set(classes) == {(4, 0, 1)}         # (what the docstring says; measured with the twin)
        assert n_drop == 0
        assert n_opt >= 0.98 * len(pairs)          # these families never need more than the narrow band
        if cap >= 16:
            assert n_cert >= 0.9 * len(pairs)


def test_align_long_indels_exact(ctx):
    """65-400 bp insertions / deletions: certified == textbook optimum; the fast mode may be worse, never certified wrongly"""
    rng = np.random.default_rng(7002)
    pairs = [make_pair(rng, int(rng.integers(500, 900)), big_indel=int(rng.integers(65, 401))) for _ in range(60)]
    n_cert, n_opt, n_drop, _ = check_pairs(ctx, pairs, 32)
    assert n_drop == 0 and n_cert >= 0.8 * len(pairs) and n_opt >= n_cert
    check_pairs(ctx, pairs, 0)
    check_pairs(ctx, pairs, 16)


def test_align_ragged_and_edge(ctx):
    rng = np.random.default_rng(7003)
    pairs = []
    for m, n in [(1, 1), (1, 7), (7, 1), (2, 3), (16, 16), (17, 15), (40, 33), (33, 40), (130, 64), (64, 130), (200, 95), (95, 200),
                 (300, 120), (1000, 1000), (1500, 1490)]:
        for _ in range(3):
            pairs.append((rnd(rng, m), rnd(rng, n)))
    # identical sequences, all-N rows, N runs
    s = rnd(rng, 333)
    pairs.append((s, s.copy()))
    pairs.append((s, np.full(300, ord("N"), np.uint8)))
    t = s.copy(); t[100:140] = ord("N")
    pairs.append((s, t))
    pairs.append((t, s))
    for cap in (0, 16):
        n_cert, n_opt, n_drop, _ = check_pairs(ctx, pairs, cap)
        assert n_drop >= 3       # (7, 1), (130, 64)-like rows shorter than half the centre are dropped


def test_align_long_pairs_lane_kernels(ctx):
    """windows of 2 000 - 11 000 columns -- what the automatic schedule hands to the lane-parallel kernels: several rounds of
    64 strips per wavefront in the traceback, long runs of up steps, pairs whose path leaves the slice (fall-back), all three
    kernel mixes of check_pairs, with and without wider bands"""
    rng = np.random.default_rng(7006)
    pairs = [make_pair(rng, L) for L in (1000, 1030, 2000, 2100, 3100, 5000, 8000, 11000)]
    pairs += [make_pair(rng, L, big_indel=bi) for L, bi in ((2500, 40), (4000, 70), (6000, 150), (3000, 300))]
    for cap in (8, 0, 16):
        check_pairs(ctx, pairs, cap)


def test_align_many_pairs_in_the_lane_kernels(ctx):
    """several hundred pairs in the lane-parallel class at once: wavefronts of 16 / 8 pairs whose pairs end in different strips
    (the whole-strip fast path of the forward kernels ends where the shortest pair of the wavefront does), lengths 40 - 2 500"""
    rng = np.random.default_rng(7007)
    pairs = [make_pair(rng, int(rng.integers(40, 700))) for _ in range(560)]
    pairs += [make_pair(rng, L, big_indel=bi) for L, bi in ((2500, 0), (1800, 50), (1200, 90), (900, 200))]
    for cap in (8, 0):
        check_pairs(ctx, pairs, cap)


def test_align_group_with_dropped_rows(ctx):
    """a row that cannot be aligned leaves the alignment; the other rows are unaffected (HIP == twin)"""
    rng = np.random.default_rng(7004)
    te = rnd(rng, 400)
    wins = [bytes(np.concatenate([rnd(rng, 50), mutate(rng, te, 0.05, 0.01), rnd(rng, 50)])) for _ in range(7)]
    wins.insert(3, bytes(rnd(rng, 90)))         # far shorter than half the centre
    wins.insert(6, bytes(rnd(rng, 120)))
    got = ctx.star_msa([wins, wins[:3]])
    exp, kept = O.star_msa(wins, rows=True)
    assert kept == len(wins) - 2 and got[0].shape == exp.shape and np.array_equal(got[0], exp)
    assert np.array_equal(got[1], O.star_msa(wins[:3]))
    sp = ctx.star_msa([wins], sparse=True)[0]
    keep = O.sparse_cols(exp).astype(bool)
    assert np.array_equal(sp, exp[:, keep])


def test_align_stats_counters(ctx):
    rng = np.random.default_rng(7005)
    pairs = [make_pair(rng, 300) for _ in range(20)]
    ctx.align_stats(reset=True)
    ctx.align_config(16)
    ctx.star_msa([[bytes(a), bytes(b)] for a, b in pairs])
    st = ctx.align_stats()
    ctx.align_config(8)
    assert st["pairs"] == 20 and st["dropped"] == 0 and st["exact_cap"] == 16      # ONE alignment per logical call (hite_star_msa_once)
    assert st["certified"] >= 18 and st["columns"] == sum(len(b) for _, b in pairs)
