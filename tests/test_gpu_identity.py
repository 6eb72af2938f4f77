"""GPU: the pairwise identity (hite_pair_identity, hite_amd/csrc/hite_ident.hip) == its twin (tests/identity_twin.py) on (cost, matches)
for every pair, and the host layer on it: the -c / -A of the cd-hit-est stand-in (util.remove_redundant_sequences, identity="gpu" /
HITE_CLUSTER_IDENTITY=gpu), its callers _stage.run_cd_hit and deredundant_for_LTR_v5.  No cd-hit-est is on PATH."""
import os
import shutil
import sys

import numpy as np
import pytest

import casegen
import identity_cases as IC
import identity_twin as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    import hite_amd

    T.clib()
    c = hite_amd.Context(0)
    yield c
    c.close()


def _same(ctx, cases):
    for label, seqs, pairs, band in cases:
        exp = T.pair_identity(seqs, pairs, band)
        got = ctx.pair_identity(seqs, pairs, band=band)
        bad = np.flatnonzero((got != exp).any(axis=1))
        assert got.shape == exp.shape and got.dtype == np.int32 and len(bad) == 0, (label, [(int(k), pairs[k], got[k].tolist(), exp[k].tolist()) for k in bad[:5]])
    return exp


def test_degenerate_pairs(ctx):
    """m = 0, n = 0 and both; lengths 1 and 2; identical sequences and sequences without a base in common; all-N; lower and mixed
    case; bytes outside ACGTN -- every pair of them on both strands"""
    exp = _same(ctx, IC.degenerate())
    assert (exp[:, 0] >= 0).all() and (exp[:, 1] == 0).any() and (exp[:, 0] == 0).any()


def test_reverse_strand_and_sub_intervals(ctx):
    """sub-intervals that touch the first and the last base of their sequence, both intervals from one sequence, an interval of
    length 0 in the middle of a sequence; each on both strands"""
    exp = _same(ctx, IC.reverse_strand())
    assert exp[:9].tolist() != exp[9:].tolist()


def test_band_widths_at_strip_edges_and_the_widest_band(ctx):
    """band = 8, |n - m| = 46, 47, 48, 110, 111, 112 (widths 63 .. 65 and 127 .. 129) with the longer sequence on either side; the
    widest band allowed (2 048 diagonals) and one more: that pair is refused (-1, 0) and its neighbours in the batch are not"""
    exp = _same(ctx, IC.band_widths())
    assert [r[0] >= 0 for r in exp.tolist()] == [True] * 21 + [False] * 3 + [True] * 3


def test_row_counts(ctx):
    """m, n = 63, 64, 65, 255, 256, 257 in every combination (the kernel does not tile rows: the strip width is its only tile)"""
    _same(ctx, IC.row_counts())


def test_paths_along_lo_and_hi(ctx):
    """one long insertion or deletion at the very start, at the very end, or split between them, with band = 0 (exactly d + 1
    diagonals: the path runs along the band's edge); and indels longer than the band allows: the band-limited cost of the twin"""
    cases = IC.edge_paths()
    _same(ctx, cases)
    label, seqs, pairs, band = cases[0]
    exp = T.pair_identity(seqs, pairs, band)
    assert exp[0].tolist() == [1, 150] and exp[6].tolist() == [5, 150]          # the inserted bases and nothing else
    label, seqs, pairs, band = cases[1]
    free = T.pair_identity(seqs, pairs, 64)
    assert (T.pair_identity(seqs, pairs, band)[:, 0] > free[:, 0]).all()        # the band of 3 did limit every one of them


def test_longest_pair_and_one_base_more(ctx):
    """32 767 x 32 767 at 5 % substitutions, band 8; an interval of 32 768 bases is refused"""
    exp = _same(ctx, IC.longest())
    assert 1300 < exp[0, 0] < 2000 and exp[0, 0] + exp[0, 1] >= IC.MAX_LEN
    assert exp[1:].tolist()[:2] == [[-1, 0], [-1, 0]] and exp[3, 0] >= 0


def test_batch_of_3000_random_pairs_in_small_batches(ctx, monkeypatch):
    """lengths 0 - 600, both strands, 0 - 40 % apart with indels, shuffled: more pairs than a launch has wavefronts per block, and
    (HITE_IDENT_BATCH = 700) five internal batches, the last one partial"""
    monkeypatch.setenv("HITE_IDENT_BATCH", "700")
    cases = IC.batch()
    exp = _same(ctx, cases)
    assert len(exp) == 3000 and (exp[:, 0] >= 0).all()
    monkeypatch.delenv("HITE_IDENT_BATCH")
    _same(ctx, [(c[0], c[1], c[2][:900], c[3]) for c in cases])                   # ... and in one batch


def test_no_pairs_one_sequence_and_refused_pairs(ctx):
    assert ctx.pair_identity(["ACGT"], []).shape == (0, 2)
    assert ctx.pair_identity([], []).shape == (0, 2)
    assert ctx.pair_identity(["ACGTACGT"], [(0, 0, 8, 0, 0, 8, 1), (0, 0, 8, 0, 0, 8, 0)], band=2).tolist() == [[0, 8], [0, 8]]      # (its own reverse complement)
    _same(ctx, IC.invalid())
    import hite_amd

    with pytest.raises(hite_amd.HiteError):
        ctx.pair_identity(["ACGT"], [(0, 0, 4, 0, 0, 4, 0)], band=-1)


# ---- the host layer ------------------------------------------------------------------------------------------------------------------
DIV_FAR = 0.08       # the divergence of the far variant (the issue's first choice; it must stay above 5 % for c = 0.95 to separate it)


class TwinIdentityCtx:
    """the context with the twin in place of Context.pair_identity"""

    def __init__(self, ctx):
        self._ctx = ctx
        self.calls = 0

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    def pair_identity(self, seqs, pairs, band=32):
        self.calls += 1
        return T.pair_identity(seqs, pairs, band)


@pytest.fixture(scope="module")
def family_lib(tmp_path_factory):
    """three families: a 1.5 kb parent, a 2 % and an 8 % variant by substitutions only (3 and 6 bases shorter: the parent is the
    longest), an 80 % fragment of every parent, unrelated sequences; shuffled"""
    assert shutil.which("cd-hit-est") is None
    rng = np.random.default_rng(2025)
    recs = []
    for f in range(3):
        parent = casegen.rand_seq(rng, 1500)
        recs.append(("fam%d_parent" % f, parent))
        recs.append(("fam%d_near" % f, casegen.mutate(rng, parent, 0.02)[:-3]))
        recs.append(("fam%d_far" % f, casegen.mutate(rng, parent, DIV_FAR)[:-6]))
        recs.append(("fam%d_frag" % f, parent[:1200]))
    recs += [("other_a", casegen.rand_seq(rng, 1100)), ("other_b", casegen.rand_seq(rng, 400)), ("other_c", casegen.rand_seq(rng, 1500))]
    d = tmp_path_factory.mktemp("identity_lib")
    inp = d / "lib.fa"
    inp.write_text("".join(">%s\n%s\n" % recs[i] for i in rng.permutation(len(recs))))
    return str(inp), d, dict(recs)


def _names(path):
    from hite_amd import util

    names, seqs = util.read_fasta(path)
    lens = [len(seqs[n]) for n in names]
    assert lens == sorted(lens, reverse=True), "the output order is longest first"
    return sorted(names)


ALWAYS = ["fam%d_%s" % (f, k) for f in range(3) for k in ("parent", "frag")] + ["other_a", "other_b", "other_c"]
FAR = ["fam%d_far" % f for f in range(3)]


def test_stand_in_merges_the_far_variant_on_coverage_alone(ctx, family_lib, monkeypatch):
    """the precondition: with the switch off the 8 % variant is merged with its parent, whatever c is"""
    from hite_amd import util

    monkeypatch.delenv("HITE_CLUSTER_IDENTITY", raising=False)
    inp, d, _ = family_lib
    for k, kw in enumerate(({}, {"c": 0.95}, {"c": 0.95, "identity": "off"})):
        out = str(d / ("off%d.fa" % k))
        util.remove_redundant_sequences(inp, out, ctx=ctx, **kw)
        assert _names(out) == sorted(ALWAYS), kw
    assert open(str(d / "off0.fa")).read() == open(str(d / "off2.fa")).read()


def test_stand_in_honours_c_with_the_switch_on(ctx, family_lib, monkeypatch, capfd):
    from hite_amd import util

    monkeypatch.delenv("HITE_CLUSTER_IDENTITY", raising=False)
    inp, d, _ = family_lib
    out80, out95 = str(d / "on80.fa"), str(d / "on95.fa")
    util.remove_redundant_sequences(inp, out80, ctx=ctx, c=0.8, identity="gpu")
    capfd.readouterr()
    util.remove_redundant_sequences(inp, out95, ctx=ctx, c=0.95, identity="gpu")
    err = capfd.readouterr().err
    assert err.count("\n") == 1 and "0 refused" in err
    assert _names(out80) == sorted(ALWAYS)                           # c = 0.8 merges both variants
    assert _names(out95) == sorted(ALWAYS + FAR)                     # c = 0.95 merges the 2 % variant and keeps the 8 % one
    # the same host code with the twin in place of the kernel writes the same files
    for c, ref in ((0.8, out80), (0.95, out95)):
        tw = TwinIdentityCtx(ctx)
        out = str(d / ("twin%d.fa" % round(100 * c)))
        util.remove_redundant_sequences(inp, out, ctx=tw, c=c, identity="gpu")
        assert tw.calls == 1 and open(out).read() == open(ref).read()
    # the switch through the environment gives the same file; an argument other than "gpu" overrides it
    monkeypatch.setenv("HITE_CLUSTER_IDENTITY", "gpu")
    env95, envoff = str(d / "env95.fa"), str(d / "envoff.fa")
    util.remove_redundant_sequences(inp, env95, ctx=ctx, c=0.95)
    util.remove_redundant_sequences(inp, envoff, ctx=ctx, c=0.95, identity="off")
    assert open(env95).read() == open(out95).read() and _names(envoff) == sorted(ALWAYS)
    util.remove_redundant_sequences(inp, envoff, ctx=ctx)            # without c there is nothing to test: today's path
    assert _names(envoff) == sorted(ALWAYS)


def test_min_aligned_and_run_cd_hit(ctx, tmp_path, monkeypatch):
    """-A 80: two near-identical sequences of 70 bases are merged with the switch off and kept apart with it on; _stage.run_cd_hit
    (which passes c = 0.8, min_aligned = 80) honours the switch"""
    from hite_amd import util

    sys.path.insert(0, os.path.join(ROOT, "hite_amd", "scripts"))
    import _stage

    assert shutil.which("cd-hit-est") is None
    monkeypatch.delenv("HITE_CLUSTER_IDENTITY", raising=False)
    util._CTX = ctx
    rng = np.random.default_rng(70)
    s = casegen.rand_seq(rng, 70)
    recs = [("short_a", s), ("short_b", s[:-2]), ("other", casegen.rand_seq(rng, 300))]
    inp = tmp_path / "in.fa"
    inp.write_text("".join(">%s\n%s\n" % r for r in recs))
    off, on, lax = str(tmp_path / "off.fa"), str(tmp_path / "on.fa"), str(tmp_path / "lax.fa")
    util.remove_redundant_sequences(str(inp), off, ctx=ctx, c=0.8)
    assert _names(off) == ["other", "short_a"]
    util.remove_redundant_sequences(str(inp), on, ctx=ctx, c=0.8, identity="gpu")
    assert _names(on) == ["other", "short_a", "short_b"]
    util.remove_redundant_sequences(str(inp), lax, ctx=ctx, c=0.8, min_aligned=60, identity="gpu")
    assert _names(lax) == ["other", "short_a"]
    st_off, st_on = str(tmp_path / "stage_off.fa"), str(tmp_path / "stage_on.fa")
    _stage.run_cd_hit(str(inp), st_off, 1)
    monkeypatch.setenv("HITE_CLUSTER_IDENTITY", "gpu")
    _stage.run_cd_hit(str(inp), st_on, 1)
    assert open(st_off).read() == open(off).read() and open(st_on).read() == open(on).read()


def test_deredundant_keeps_sub_families_apart_at_095(ctx, tmp_path, monkeypatch):
    """deredundant_for_LTR_v5 with coverage_threshold = 0.95 on a library of two sub-families 8 % apart (three copies each, 1 % around
    their own consensus).  The first stage of the merge clusters on coverage alone, as the reference does, and would fold the six
    copies into one consensus before the cd-hit-est step is reached; the two sub-families reach that step as two consensus sequences
    where the merge cuts a cluster in file order (the fall-back for clusters above CLUSTER_CLEAN_THRESHOLD members, here lowered to 3
    as tests/test_gpu_parity.py lowers SEED_MAX_SEGMENTS).  With the switch off the step makes one record of them, with it on two."""
    from hite_amd import util

    assert shutil.which("cd-hit-est") is None
    monkeypatch.setattr(util, "CLUSTER_CLEAN_THRESHOLD", 3)
    rng = np.random.default_rng(95)
    sub_a = casegen.rand_seq(rng, 1500)
    sub_b = casegen.mutate(rng, sub_a, DIV_FAR)
    recs = [("G%d-subA#DNA/hAT" % g, casegen.mutate(rng, sub_a, 0.01)) for g in range(3)]
    recs += [("G%d-subB#DNA/hAT" % g, casegen.mutate(rng, sub_b, 0.01)) for g in range(3)]
    recs.append(("single#Unknown", casegen.rand_seq(rng, 900)))
    counts = {}
    for mode in ("off", "gpu"):
        monkeypatch.setenv("HITE_CLUSTER_IDENTITY", mode)
        lib = tmp_path / ("lib_%s.fa" % mode)
        lib.write_text("".join(">%s\n%s\n" % r for r in recs))
        st = {}
        util.deredundant_for_LTR_v5(str(lib), str(tmp_path), 1, "x", 0.95, 0, ctx=ctx, stages=st)
        assert sorted(len(cl) for cl in st["clusters"]) == [1, 3, 3] or sorted(len(cl) for cl in st["clusters"]) == [3, 3], st["clusters"]
        tmp_names = util.read_fasta(str(lib) + ".tmp.cons")[0]
        assert sum("-subA#" in n for n in tmp_names) == 1 and sum("-subB#" in n for n in tmp_names) == 1
        names = util.read_fasta(str(lib) + ".cons")[0]
        assert "single#Unknown" in names
        counts[mode] = sum("-sub" in n for n in names)
    assert counts == {"off": 1, "gpu": 2}
