"""The pairwise aligner (hite_amd/csrc/hite_align.hip) at the limits of its band levels, its certificate and its fall-back: HIP == the twin
(oracle/hite_oracle_msa.c) byte for byte on the pairs of tests/align_limit_cases.py, each of which test_align_limit_cases.py proves
on the CPU to end in the class it is named for -- (band words of the run kept, status, certified) per exact cap.

Every run goes through the three kernel mixes of align_check.check_pairs (hite_align_lanes -2, 0, 400) and asserts, per pair: info (U,
certificate, status, k*, band words) and alignment bytes == twin; cost recomputed from the matrix == U; a certified pair == the
band-free definition, ops and cost; any other pair U >= the definition's cost; and per run: the tally of classes == what the cases
promise, the counters of hite_align_stats == the sums over the twin's results.  The tallies are printed (pytest -s) for the record.

Which kernels a class reaches (hite_align_run):
  every pair                       align_fwd4_kernel (lanes -2) / align_fwd_lanes_kernel<4> (lanes 0)
  (8, ., .) at cap 8               align_fwd8_pair_kernel (lanes -2) / align_fwd_lanes_kernel<8> (lanes 0)
  (8 | 16 | 32, ., .) at cap >= 16 align_fwd_kernel<8 | 16 | 32>, then align_tb_kernel twice (the pairs that are final after the
                                   4-word run beside the wider bands, the others after them)
  no wider run in the call         align_tb_kernel (lanes -2) / align_tb_strips_kernel (lanes 0)
  (320, ., .)                      align_wide_fwd_kernel, align_wide_tb_kernel

The two pairs at the window limit of 32 767 columns are compared with the twin and with the definition's COST only: its traceback
keeps the whole matrix, 4 GB.  No other pair is excused from anything."""
import pytest

import align_limit_cases as AC
from align_check import FALLBACK, LANE_MODES, check_groups, check_pairs

pytestmark = pytest.mark.gpu

assert FALLBACK == AC.FB


@pytest.fixture(scope="module")
def ctx():
    import hite_amd

    c = hite_amd.Context(0)
    yield c
    c.close()


def tally(classes):
    out = {}
    for c in classes:
        out[c] = out.get(c, 0) + 1
    return out


def run(ctx, what, cases, cap, no_nw_pair=()):
    """one list of cases at one cap through the three kernel mixes: every per-pair assertion of the checker, then the classes"""
    res = check_pairs(ctx, [(c.a, c.b) for c in cases], cap, no_nw_pair)
    for c, got in zip(cases, res.classes):
        assert got == c.cls[cap], (c.name, cap, got, c.cls[cap])
    assert tally(res.classes) == AC.tally(cases, cap)
    print("\n[align limits] %s: cap %d, lanes %s, %d pairs: %s" % (what, cap, "/".join(str(x) for x in LANE_MODES), len(cases),
                                                               ", ".join("%s x %d" % kv for kv in sorted(tally(res.classes).items()))))
    return res


def test_classes_a_b_c(ctx):
    """both sides of the certificate bound and of the three level thresholds; pairs kept uncertified from 8 and 16 words; pairs
    escalated twice; the fall-back after a kept run of 4, 8, 16 and 32 words, at its own limit and beyond it -- at every cap"""
    cases = AC.class_a() + AC.class_b() + AC.class_c()
    for cap in AC.CAPS:
        res = run(ctx, "A + B + C", cases, cap)
        t = tally(res.classes)
        assert t.get((AC.FB, 1, 0), 0) >= 4 and t.get((AC.FB, 0, 0), 0) >= 1 and res.n_drop == t[(AC.FB, 1, 0)]
        for lvl in (8, 16, 32):
            assert ((lvl, 0, 1) in t) == (cap >= lvl)
        assert ((8, 0, 0) in t) == (cap == 8) and ((16, 0, 0) in t) == (cap == 16)


def test_class_d_geometry(ctx):
    """lengths around 16, 32, 512 and 1024 columns in every combination, rows just too short and just long enough, N runs and pad
    bytes inside a pair that reaches 8 words"""
    cases = AC.class_d()
    for cap in AC.D_CAPS:
        res = run(ctx, "D", cases, cap)
        assert res.n_drop == 4 and ((8, 0, 1) in res.classes) == (cap == 8)


def test_class_d_window_limit(ctx):
    cases = AC.class_d_window_limit()
    assert not any(c.nw_pair for c in cases)
    for cap in AC.D_CAPS:
        res = run(ctx, "D at 32 767 columns", cases, cap, no_nw_pair=range(len(cases)))
        assert res.n_cert == res.n_opt == len(cases)


def test_class_e_grains_of_the_8_word_level(ctx):
    """1 .. 129 pairs that all reach 8 words at cap 8: blocks of 32 pairs in align_fwd8_pair_kernel, waves of 8 / 16 pairs in
    align_fwd_lanes_kernel<8> / <4>, filled, one short and one over; then a wave whose pairs end in different strips"""
    cases = AC.grains_8()
    for n in AC.GRAINS_8:
        res = run(ctx, "E, %d pairs to 8 words" % n, cases[:n], 8)
        assert res.classes == ((8, 0, 1),) * n and res.n_cert == n
    mix = AC.mixed_wave()
    run(ctx, "E, 40 beside 3 000 columns", mix, 8)


def test_class_e_grains_of_the_16_and_32_word_levels(ctx):
    """1 .. 65 pairs to 16 words and as many to 32 at cap 32, with as many 8-word pairs between them: align_fwd_kernel<8 | 16 | 32> on
    lists around the block of 64 pairs, the overlap path with its two align_tb_kernel launches"""
    e8, e16, e32 = AC.grains_8(), AC.grains_16(), AC.grains_32()
    for n in AC.GRAINS_WIDE:
        cases = [c for three in zip(e16[:n], e8[:n], e32[:n]) for c in three]
        res = run(ctx, "E, %d pairs each to 8, 16 and 32 words" % n, cases, 32)
        assert tally(res.classes) == {(8, 0, 1): n, (16, 0, 1): n, (32, 0, 1): n}


def test_class_f_one_centre_many_fates(ctx):
    """rows of ONE centre that end at 4, 8, 16 and 32 words, in the fall-back, dropped by it and dropped as too short: the centre's
    planes are shared by all of them; a second group without drops beside it"""
    groups, classes = AC.one_centre_many_fates()
    got = check_groups(ctx, groups, AC.F_CAP)
    assert list(got) == [tuple(c) for c in classes]
    print("\n[align limits] F: cap %d, lanes %s: %s" % (AC.F_CAP, "/".join(str(x) for x in LANE_MODES),
                                                     "; ".join(", ".join("%s x %d" % kv for kv in sorted(tally(g).items())) for g in got)))
    # and alone: the same bytes whatever shares the call
    for g, cl in zip(groups, classes):
        assert check_groups(ctx, [g], AC.F_CAP) == (tuple(cl),)
