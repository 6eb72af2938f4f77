"""GPU parity: the HIP path (through the C ABI) vs the golden vectors generated from the reference's
Python and vs the C oracle on fresh seeded inputs.  Bit-exact on every integer / byte output."""
import os

import numpy as np
import pytest

import casegen
import oracle_lib as O
from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import hite_amd

    c = hite_amd.Context(0)
    yield c
    c.close()


def test_flank_gather_golden(ctx):
    for case in load_golden("gather"):
        names = case["names"]
        ctx.genome_pack(case["seqs"])
        for q, copies in case["copies"].items():
            contig = [names.index(c[0]) for c in copies]
            wins, tr = ctx.flank_gather(contig, [c[1] for c in copies], [c[2] for c in copies],
                                        [1 if c[4] == "-" else 0 for c in copies], case["flank"])
            seen = {}
            for c, w, t in zip(copies, wins, tr):
                if w is None:
                    continue
                seen["%s:%d-%d(%s)" % (c[0], c[1], c[2], c[4])] = (w.decode(), t.decode() if t else None)
            exp = case["expected"].get(q)
            if exp is None:
                assert not seen
                continue
            # the packed genome folds IUPAC codes to N (documented): compare under that folding
            fold = lambda s: "".join(ch if ch in "ACGTN" else "N" for ch in s)  # noqa: E731
            assert [[k, v[0]] for k, v in seen.items()] == [[k, fold(v)] for k, v in exp["extend"]]
            tr_exp = exp["trunc"]
            got_tr = [[k, v[1]] for k, v in seen.items() if v[1] is not None] or None
            assert got_tr == ([[k, fold(v)] for k, v in tr_exp] if tr_exp else None)


def test_flank_gather_random_vs_oracle(ctx):
    names, seqs = casegen.make_genome(77, n_chr=4, chr_len=(3000, 90000), other_frac=0.0)
    ctx.genome_pack(seqs)
    copies = casegen.make_copies(78, names, seqs, n_cand=40, per_cand=(5, 40), length=(30, 4000))
    flat = [c for v in copies.values() for c in v]
    wins, tr = ctx.flank_gather([names.index(c[0]) for c in flat], [c[1] for c in flat], [c[2] for c in flat],
                                [1 if c[4] == "-" else 0 for c in flat], 50)
    nw = 0
    for c, w, t in zip(flat, wins, tr):
        ew, et = O.flank_window(seqs[names.index(c[0])], c[1], c[2], c[4], 50)
        assert (w.decode() if w else None) == ew
        assert (t.decode() if t else None) == et
        nw += w is not None
    assert nw > 500


def _msas(cases, key="seqs"):
    return [O.msa_array(c[key]) for c in cases]


@pytest.mark.parametrize("name", ["judge_tir", "judge_non_ltr", "judge_helitron"])
def test_sparse_cols_golden(ctx, name):
    cases = load_golden(name)
    got = ctx.sparse_cols(_msas(cases))
    for c, g in zip(cases, got):
        assert ["".join(map(chr, r)) for r in g] == c["clean"]


def test_column_vote_vs_oracle(ctx):
    """hite_column_vote against the oracle's col_base_map (the structure every golden judge / search case runs through on the CPU
    side) on the cleaned alignments of all three judge fixtures"""
    n = 0
    for name in ("judge_tir", "judge_non_ltr", "judge_helitron"):
        cases = [c for c in load_golden(name) if c["clean"] and len(c["clean"][0]) > 0][:40]
        msas = [O.msa_array(c["clean"]) for c in cases]
        got = ctx.column_vote(msas)
        for m, g in zip(msas, got):
            assert np.array_equal(g, O.column_vote(m))
            n += 1
    assert n >= 100


def test_boundary_search_golden(ctx):
    cases = [c for c in load_golden("boundary_search") if len(c["seqs"]) <= 128]
    assert len(cases) > 50
    msas = _msas(cases)
    pos = [c["pos"] for c in cases]
    side = [c["side"] for c in cases]
    thr = [c["thr"] for c in cases]
    b3, _ = ctx.boundary_search(msas, pos, side, thr, variant=3)
    assert list(b3) == [c["v3"] for c in cases]
    b4, v4 = ctx.boundary_search(msas, pos, side, thr, variant=4, int_thr=[t - 0.05 for t in thr], out_thr=thr)
    assert [[bool(v), int(b)] for v, b in zip(v4, b4)] == [c["v4"] for c in cases]


def test_boundary_search_edge_golden(ctx):
    """round 4: positions within 10 columns of the alignment's edges, homology that runs to the edge, alignments of 5-30 columns"""
    cases = load_golden("boundary_search_edge")
    msas = _msas(cases)
    pos = [c["pos"] for c in cases]
    side = [c["side"] for c in cases]
    thr = [c["thr"] for c in cases]
    b3, _ = ctx.boundary_search(msas, pos, side, thr, variant=3)
    assert list(b3) == [c["v3"] for c in cases]
    b4, v4 = ctx.boundary_search(msas, pos, side, thr, variant=4, int_thr=[t - 0.05 for t in thr], out_thr=thr)
    assert [[bool(v), int(b)] for v, b in zip(v4, b4)] == [c["v4"] for c in cases]


@pytest.mark.parametrize("mode", ["default", "block_only", "wave", "lds"])
def test_judge_edge_golden(ctx, mode, monkeypatch):
    """round 4: the reference's answers on the edge cases (tests/casegen.py: msa_edge_cases), through sparse-column removal and
    every judge kernel form"""
    env = {"default": {}, "block_only": {"HITE_JUDGE_WAVE_COLS": "0", "HITE_JUDGE_LDS": "0"},
           "wave": {"HITE_JUDGE_WAVE_MIN_BATCH": "0", "HITE_JUDGE_LDS": "0"},
           "lds": {"HITE_JUDGE_LDS": "1", "HITE_JUDGE_WAVE_MIN_BATCH": "0", "HITE_JUDGE_LDS_WAVE0": "2048", "HITE_JUDGE_LDS_WAVE1": "6000"}}[mode]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cases = load_golden("judge_edge")
    if mode == "default":
        got = ctx.sparse_cols(_msas(cases))
        for c, g in zip(cases, got):
            assert ["".join(map(chr, r)) for r in g] == c["clean"]
    n = 0
    for te_type in ("tir", "non_ltr", "helitron"):
        for plant in (0, 1):
            sub = [c for c in cases if c["plant"] == plant and c["te_type"] == te_type]
            if not sub:
                continue
            got = ctx.judge(te_type, _msas(sub, "clean"), [c["cand"] for c in sub], plant=plant)
            for i, (c, g) in enumerate(zip(sub, got)):
                exp = c["expected"]
                if exp[0] == "EXC":
                    assert g[1] == "EXC", (i, g, exp)
                else:
                    assert [g[0], g[1], g[2], g[3]] == exp, (te_type, plant, i, c["aim"], g, exp)
                n += 1
    assert n == len(cases)


def test_threshold_ties_golden_on_gpu(ctx):
    """thr / thr - 0.1 ties in binary64: columns at exactly k/R of the rows, through the HIP searches"""
    cases = load_golden("thr_ties_search")
    msas = _msas(cases)
    pos = [c["pos"] for c in cases]
    side = [c["side"] for c in cases]
    thr = [c["thr"] for c in cases]
    b3, _ = ctx.boundary_search(msas, pos, side, thr, variant=3)
    assert list(b3) == [c["v3"] for c in cases]
    b4, v4 = ctx.boundary_search(msas, pos, side, thr, variant=4, int_thr=[t - 0.05 for t in thr], out_thr=thr)
    assert [[bool(v), int(b)] for v, b in zip(v4, b4)] == [c["v4"] for c in cases]
    # and the single windows of thr_ties.json.gz: a 12-column window is what the 'start' search evaluates first when the
    # alignment has 24 columns and pos = 0 ... only if 12 >= 10 valid columns exist, which they do (no gaps)
    for c in load_golden("thr_ties"):
        rows = [s + s for s in c["seqs"]]
        m = O.msa_array(rows)
        g, _ = ctx.boundary_search([m], [0], ["start"], [c["thr"]], variant=3)
        assert int(g[0]) == O.search_v3(m, 0, 0, c["thr"])


@pytest.mark.parametrize("name,te_type", [("judge_tir", "tir"), ("judge_non_ltr", "non_ltr"), ("judge_helitron", "helitron")])
def test_judge_golden(ctx, name, te_type):
    cases = load_golden(name)
    for plant in (0, 1):
        sub = [c for c in cases if c["plant"] == plant]
        if not sub:
            continue
        got = ctx.judge(te_type, _msas(sub, "clean"), [c["cand"] for c in sub], plant=plant)
        for i, (c, g) in enumerate(zip(sub, got)):
            exp = c["expected"]
            if exp[0] == "EXC":
                assert g[1] == "EXC", (i, g, exp)
            else:
                assert [g[0], g[1], g[2], g[3]] == exp, (i, g, exp)


@pytest.mark.parametrize("mode", ["block_only", "wave_default", "wave_rows_32", "wave_wide", "lds_block", "lds_wave", "lds_wave_small_tiles",
                                  "block_two_kernels", "wave_two_kernels"])
@pytest.mark.parametrize("name,te_type", [("judge_tir", "tir"), ("judge_non_ltr", "non_ltr"), ("judge_helitron", "helitron")])
def test_judge_golden_kernel_forms(ctx, name, te_type, mode, monkeypatch):
    """the four judge kernels ({one wavefront, one workgroup} per alignment x {alignment read from HBM, alignment held in LDS}) give
    the same calls: every golden through the workgroup kernel on HBM only, through the wave kernel on HBM as a large batch got it
    before the LDS forms, with the row limit at 32 (the 64-row mask path stays in the workgroup kernel), with the column limit
    lifted (anchor text of wide alignments in global scratch); then through the LDS forms (HITE_JUDGE_LDS=1; off by default, they
    measured slower): workgroup, wavefront with the default tiles, wavefront with tiles so small that the classes split the
    goldens between all kernels; the last two modes run the two classes on HBM as an anchor kernel + the rest (round 6,
    HITE_JUDGE_SPLIT: measured, not faster, off by default)"""
    env = {"block_only": {"HITE_JUDGE_WAVE_COLS": "0", "HITE_JUDGE_LDS": "0"},
           "block_two_kernels": {"HITE_JUDGE_WAVE_COLS": "0", "HITE_JUDGE_LDS": "0", "HITE_JUDGE_SPLIT": "3"},
           "wave_two_kernels": {"HITE_JUDGE_WAVE_MIN_BATCH": "0", "HITE_JUDGE_LDS": "0", "HITE_JUDGE_SPLIT": "3"},
           "wave_rows_32": {"HITE_JUDGE_WAVE_ROWS": "32", "HITE_JUDGE_WAVE_MIN_BATCH": "0", "HITE_JUDGE_LDS": "0"},
           "wave_default": {"HITE_JUDGE_WAVE_MIN_BATCH": "0", "HITE_JUDGE_LDS": "0"},
           "wave_wide": {"HITE_JUDGE_WAVE_COLS": "60000", "HITE_JUDGE_OVERLAP": "0", "HITE_JUDGE_WAVE_MIN_BATCH": "0", "HITE_JUDGE_LDS": "0"},
           "lds_block": {"HITE_JUDGE_LDS": "1", "HITE_JUDGE_LDS_BLOCK0": "61440", "HITE_JUDGE_LDS_BLOCK1": "126976"},
           "lds_wave": {"HITE_JUDGE_LDS": "1", "HITE_JUDGE_WAVE_MIN_BATCH": "0"},
           "lds_wave_small_tiles": {"HITE_JUDGE_LDS": "1", "HITE_JUDGE_WAVE_MIN_BATCH": "0", "HITE_JUDGE_LDS_WAVE0": "2048", "HITE_JUDGE_LDS_WAVE1": "6000",
                                    "HITE_JUDGE_LDS_WAVE2": "12000", "HITE_JUDGE_LDS_BLOCK0": "20000", "HITE_JUDGE_LDS_BLOCK1": "40000"}}[mode]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cases = load_golden(name)
    if mode == "wave_wide":   # a wide alignment with few rows: above the LDS anchor limit of the wave kernel (2552 columns)
        c = casegen.make_msa_case(seed=4242, te_type=te_type, rows=9, te_len=3300, div=0.04, ins_cols=4, trunc_rows=1, tsd_len=8, tsd_frac=1.0)
        m = O.msa_array(c["seqs"])
        keep = O.sparse_cols(m).astype(bool)
        mc = np.ascontiguousarray(m[:, keep])
        exp, _ = O.judge(te_type, mc, c["cand"], 1)
        g = ctx.judge(te_type, [mc], [c["cand"]], plant=1)[0]
        assert [g[0], g[1], g[2], g[3]] == exp and mc.shape[1] > 2552
    for plant in (0, 1):
        sub = [c for c in cases if c["plant"] == plant]
        if not sub:
            continue
        got = ctx.judge(te_type, _msas(sub, "clean"), [c["cand"] for c in sub], plant=plant)
        for i, (c, g) in enumerate(zip(sub, got)):
            exp = c["expected"]
            if exp[0] == "EXC":
                assert g[1] == "EXC", (i, g, exp)
            else:
                assert [g[0], g[1], g[2], g[3]] == exp, (i, g, exp)


# the widest alignment whose ungapped anchor text + match records a judge kernel keeps in its LDS mask tile (hite_judge.hip):
WAVE_ANCHOR_LDS_COLS = 2552      # JWAV_ANCHOR_COLS at JWAV_TILE_COLS = 160: the wavefront form (jwav), and the default HITE_JUDGE_WAVE_COLS
BLOCK_ANCHOR_LDS_COLS = 5104     # ANCHOR_LDS_COLS of the workgroup form (jblk)


@pytest.fixture(scope="module")
def anchor_limit_cases():
    """the alignments of test_judge_at_anchor_lds_limits with the oracle's calls: built once, shared by the kernel forms, never changed"""
    import judge_limit_cases as JL

    cases = JL.build(WAVE_ANCHOR_LDS_COLS, BLOCK_ANCHOR_LDS_COLS)
    JL.check_conditions(cases)
    assert sorted({c["C"] for c in cases}) == [2536, 2544, 2551, 2552, 2553, 2560, 2568, 5088, 5103, 5104, 5105, 5120]
    assert sorted({c["rows"] for c in cases}) == [9, 64, 65] and len(cases) == 3 * 36
    print("alignments the oracle calls TE, by type and width:", JL.te_counts(cases))
    return cases, JL.build_repetitive(WAVE_ANCHOR_LDS_COLS, BLOCK_ANCHOR_LDS_COLS)


def _assert_call(g, exp, bounds, what):
    if exp[0] == "EXC":
        assert g[1] == "EXC", (what, g, exp)
        return
    assert [g[0], g[1], g[2], g[3]] == exp, (what, g[:2], g[3:], exp[:2], exp[3:])
    if exp[0]:
        assert (g[4], g[5]) == tuple(bounds), (what, g[4:], bounds)


@pytest.mark.parametrize("mode", ["wave_default", "wave_wide", "block_only", "wave_two_kernels", "block_two_kernels"])
def test_judge_at_anchor_lds_limits(ctx, anchor_limit_cases, mode, monkeypatch):
    """Alignments of exactly 2536 .. 2568 and 5088 .. 5120 columns x 9 / 64 / 65 rows, all three TE types, against the oracle: the
    widths either side of the two limits up to which a judge kernel keeps the ungapped anchor text and the match records in its LDS
    mask tile (above: global scratch), and the row counts either side of the wavefront class.  An off-by-one at a limit overruns
    one LDS region into its neighbour without a fault -- only a wrong call shows it.  Every alignment has a row without gaps (text
    of C bytes); per type at least a third are TE calls, and candidates that reach to 8 columns from either edge put the anchors
    into the first / last text starts.  Each alignment alone with plant 0 and 1, then all of a type as ONE batch between ~30 narrow
    goldens (both classes in the work lists, neighbours for an overrun to damage).  A second group has tandem arrays of the
    candidate's ends inside the element, which sends the anchor search through the form that uses the match records."""
    env = {"wave_default": {"HITE_JUDGE_WAVE_MIN_BATCH": "0", "HITE_JUDGE_LDS": "0"},
           "wave_wide": {"HITE_JUDGE_WAVE_COLS": "60000", "HITE_JUDGE_OVERLAP": "0", "HITE_JUDGE_WAVE_MIN_BATCH": "0", "HITE_JUDGE_LDS": "0"},
           "block_only": {"HITE_JUDGE_WAVE_COLS": "0", "HITE_JUDGE_LDS": "0"},
           "wave_two_kernels": {"HITE_JUDGE_WAVE_MIN_BATCH": "0", "HITE_JUDGE_LDS": "0", "HITE_JUDGE_SPLIT": "3"},
           "block_two_kernels": {"HITE_JUDGE_WAVE_COLS": "0", "HITE_JUDGE_LDS": "0", "HITE_JUDGE_SPLIT": "3"}}[mode]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    limit_cases, repetitive = anchor_limit_cases
    if mode == "wave_default":
        # the class border itself (hite_judge_classify_dev, as hite_judge_dev splits a batch): 64 rows x 2552 columns is the last
        # alignment of the wavefront class (JUDGE_CLS_WAVE = 1), one more row or column goes to the workgroup (JUDGE_CLS_BLOCK = 0)
        import ctypes as C

        import torch

        dev = torch.device("cuda", 0)
        d_rows = torch.tensor([9, 9, 64, 64, 65, 1], dtype=torch.int32).to(dev)
        d_cols = torch.tensor([WAVE_ANCHOR_LDS_COLS, WAVE_ANCHOR_LDS_COLS + 1, WAVE_ANCHOR_LDS_COLS, WAVE_ANCHOR_LDS_COLS + 1, WAVE_ANCHOR_LDS_COLS, 1],
                              dtype=torch.int32).to(dev)
        d_cls = torch.full((6,), 255, dtype=torch.uint8).to(dev)
        torch.cuda.synchronize()
        rc = ctx.lib.hite_judge_classify_dev(ctx.h, 6, C.c_void_p(d_rows.data_ptr()), C.c_void_p(d_cols.data_ptr()), C.c_void_p(d_cls.data_ptr()), None)
        assert rc == 0
        assert ctx.download(d_cls.data_ptr(), 6, np.uint8).tolist() == [1, 0, 1, 0, 0, 1]
    n_alone = n_batch = 0
    for name, te_type in (("judge_tir", "tir"), ("judge_non_ltr", "non_ltr"), ("judge_helitron", "helitron")):
        sub = [c for c in limit_cases + repetitive if c["te_type"] == te_type]
        for plant in (0, 1):
            for c in sub:
                g = ctx.judge(te_type, [c["mc"]], [c["cand"]], plant=plant)[0]
                _assert_call(g, *c["exp"][plant], (mode, te_type, c["rows"], c["C"], plant, "alone"))
                n_alone += 1
        golden = [c for c in load_golden(name) if c["clean"] and len(c["clean"][0]) > 0]
        n_gold = 0
        for plant in (0, 1):
            gold = [c for c in golden if c["plant"] == plant][:30]
            n_gold += len(gold)
            # interleaved: a golden after every boundary alignment while they last
            order = []
            for i in range(max(len(sub), len(gold))):
                order += [("limit", sub[i])] if i < len(sub) else []
                order += [("golden", gold[i])] if i < len(gold) else []
            msas = [c["mc"] if kind == "limit" else O.msa_array(c["clean"]) for kind, c in order]
            got = ctx.judge(te_type, msas, [c["cand"] for _k, c in order], plant=plant)
            for i, ((kind, c), g) in enumerate(zip(order, got)):
                if kind == "limit":
                    _assert_call(g, *c["exp"][plant], (mode, te_type, c["rows"], c["C"], plant, "batch", i))
                elif c["expected"][0] == "EXC":
                    assert g[1] == "EXC", (mode, te_type, plant, i, g, c["expected"])
                else:
                    assert [g[0], g[1], g[2], g[3]] == c["expected"], (mode, te_type, plant, "golden in the batch", i, g, c["expected"])
                n_batch += 1
        assert n_gold >= 25, (name, n_gold)
    assert n_alone == 2 * (len(limit_cases) + len(repetitive)) and n_batch > n_alone


@pytest.mark.parametrize("te_type", ["tir", "non_ltr", "helitron"])
def test_judge_random_vs_oracle(ctx, te_type):
    """fresh seeds, sparse-col removal + judge chained on the GPU, compared with the oracle chain"""
    params = casegen.msa_param_grid(te_type, 60, 4242 + len(te_type))
    cases = [casegen.make_msa_case(**p) for p in params]
    msas = _msas(cases)
    clean = ctx.sparse_cols(msas)
    got = ctx.judge(te_type, clean, [c["cand"] for c in cases], plant=1)
    ntrue = 0
    for c, m, cl, g in zip(cases, msas, clean, got):
        keep = O.sparse_cols(m).astype(bool)
        mc = np.ascontiguousarray(m[:, keep])
        assert np.array_equal(mc, cl)
        exp, (bs, be) = O.judge(te_type, mc, c["cand"], 1)
        if exp[0] == "EXC":
            assert g[1] == "EXC"
            continue
        assert [g[0], g[1], g[2], g[3]] == exp
        if exp[0]:
            assert (g[4], g[5]) == (bs, be)
            ntrue += 1
    assert ntrue >= 1


@pytest.mark.parametrize("te_type", ["tir", "helitron"])
def test_judge_anchors_in_repetitive_rows(ctx, te_type):
    """tandem arrays of the candidate's own ends on both sides of every row: the anchor filter flags far more than 64 match ends,
    so the search takes the form with a match record per text start (blk_fnm_full) instead of the match list; same calls as
    the oracle"""
    cases = []
    for i in range(6):
        c = casegen.make_msa_case(seed=7100 + i, te_type=te_type, rows=8 + 3 * i, te_len=240, tsd_len=8, tsd_frac=1.0,
                                  shift_l=(i % 3) * 3, shift_r=-(i % 2) * 2)
        head, tail = c["cand"][:20], c["cand"][-20:]
        reps = 70 + 5 * i
        c = dict(c, seqs=[(head * reps)[: 20 * reps - (3 * r) % 7] + "-" * ((3 * r) % 7) + s + "-" * ((5 * r) % 6) + (tail * reps)[(5 * r) % 6:]
                          for r, s in enumerate(c["seqs"])])
        cases.append(c)
    msas = _msas(cases)
    clean = ctx.sparse_cols(msas)
    got = ctx.judge(te_type, clean, [c["cand"] for c in cases], plant=1)
    for c, m, cl, g in zip(cases, msas, clean, got):
        keep = O.sparse_cols(m).astype(bool)
        mc = np.ascontiguousarray(m[:, keep])
        assert np.array_equal(mc, cl)
        exp, (bs, be) = O.judge(te_type, mc, c["cand"], 1)
        if exp[0] == "EXC":
            assert g[1] == "EXC"
            continue
        assert [g[0], g[1], g[2], g[3]] == exp
        if exp[0]:
            assert (g[4], g[5]) == (bs, be)


def test_tsd_search_golden(ctx):
    cases = load_golden("tsd_search")
    for plant in (0, 1):
        sub = [c for c in cases if c["plant"] == plant]
        got = ctx.tsd_search([c["seq"] for c in sub], [c["start"] for c in sub], [c["end"] for c in sub], plant)
        for c, g in zip(sub, got):
            assert (g[0], g[1]) == (c["left"], c["right"])


def test_judge_wide_alignment(ctx):
    """full-length second pass shape: ~6 kb wide alignment (C-ABI limit is 65535 columns)"""
    c = casegen.make_msa_case(seed=31337, te_type="tir", rows=40, te_len=6000, div=0.05, ins_cols=12, trunc_rows=3,
                              shift_l=5, shift_r=-3, tsd_len=9, tsd_frac=1.0)
    m = O.msa_array(c["seqs"])
    cl = ctx.sparse_cols([m])[0]
    g = ctx.judge("tir", [cl], [c["cand"]], plant=1)[0]
    keep = O.sparse_cols(m).astype(bool)
    exp, _ = O.judge("tir", np.ascontiguousarray(m[:, keep]), c["cand"], 1)
    assert [g[0], g[1], g[2], g[3]] == exp


def _families(seed, n_fam, rows_choices=(2, 8, 30, 60), lens=(150, 400, 800, 1400)):
    rng = np.random.default_rng(seed)
    groups = []
    for f in range(n_fam):
        L = int(rng.choice(lens))
        R = int(rng.choice(rows_choices))
        div = float(rng.choice([0.0, 0.05, 0.12, 0.2]))
        indel = float(rng.choice([0.0, 0.01, 0.03]))
        cons = casegen.rand_seq(rng, L)
        wins = []
        for r in range(R):
            s = casegen.mutate(rng, cons, div if r else 0.0)
            out = []
            for ch in s:
                x = rng.random()
                if r and x < indel / 2:
                    continue
                out.append(ch)
                if r and x > 1 - indel / 2:
                    out.append(casegen.rand_seq(rng, int(rng.integers(1, 4))))
            te = "".join(out)
            if r and rng.random() < 0.1:
                te = te[: len(te) // 2] + te[len(te) // 2 + int(rng.integers(5, 60)):]  # a larger deletion
            w = casegen.rand_seq(rng, 50) + te + casegen.rand_seq(rng, 50)
            if rng.random() < 0.05:
                w = w[:30] + "NNNNN" + w[35:]
            wins.append(w)
        groups.append(wins)
    return groups


def test_star_msa_vs_twin(ctx):
    groups = _families(2024, 40)
    got = ctx.star_msa(groups)
    for g, m in zip(groups, got):
        exp = O.star_msa(g)
        assert m is not None and m.shape == exp.shape
        assert np.array_equal(m, exp)
        # every row, ungapped, is the input window
        for r, w in enumerate(g):
            assert bytes(m[r][m[r] != ord("-")]) == w.encode()


def test_star_msa_to_judge_chain(ctx):
    """windows -> star alignment -> sparse columns -> judge, all on the GPU, vs the oracle chain"""
    groups = _families(777, 24, rows_choices=(8, 30, 60), lens=(200, 500, 900))
    cands = [g[0][50 - 6: len(g[0]) - 50 + 4] for g in groups]
    msas = ctx.star_msa(groups)
    clean = ctx.sparse_cols(msas)
    got = ctx.judge("tir", clean, cands, plant=1)
    for g, cand, res in zip(groups, cands, got):
        m = O.star_msa(g)
        keep = O.sparse_cols(m).astype(bool)
        exp, _ = O.judge("tir", np.ascontiguousarray(m[:, keep]), cand, 1)
        assert [res[0], res[1], res[2], res[3]] == exp


def _synthetic_fine_inputs(seed, n_fam=14, te_types=("tir",)):
    """small genome with planted TE families + the copy table a copy finder would return"""
    import synth_small

    return synth_small.make(seed, n_fam)


@pytest.mark.parametrize("te_type", ["tir", "helitron", "non_ltr"])
def test_fine_stage_vs_oracle_chain(ctx, te_type, monkeypatch):
    """the fused pipeline per TE type (judge_TIR / judge_Helitron:86-97 / judge_Non_LTR:48-51 all run flank_region_align_v5)
    on families shaped for that type, against the oracle chain.  TIR and non-LTR with the one-wavefront-per-alignment judge
    kernel switched on for this small batch (large batches get it by default), Helitron with the workgroup kernel alone."""
    import oracle_pipeline as OP
    import synth_small

    if te_type != "helitron":
        monkeypatch.setenv("HITE_JUDGE_WAVE_MIN_BATCH", "0")

    n_te = 0
    ran_a = ran_b = 0
    for seed in (11, 12):
        g = synth_small.make(seed, n_fam=16, te_type=te_type)
        ctx.genome_pack(g["contigs"])
        got, stats = ctx.flank_region_align(te_type, g["cands"], g["copies"], plant=1)
        # the same batch with the fill fused into the judge's LDS kernels (off by default): alignments of the LDS classes never
        # reach HBM, the calls are the same
        with monkeypatch.context() as mp:
            mp.setenv("HITE_JUDGE_LDS", "1")
            fused, stats_fused = ctx.flank_region_align(te_type, g["cands"], g["copies"], plant=1)
        assert fused == got
        assert stats_fused[2] + stats_fused[6] < stats[2] + stats[6]      # alignment bytes in HBM
        for cand, copies, res in zip(g["cands"], g["copies"], got):
            exp = OP.fine_stage_candidate(te_type, cand, copies, g["contigs"], plant=1)
            assert [res[0], res[1], res[2], res[3]] == exp, (te_type, seed, res, exp)
            n_te += res[0]
        ran_a += stats[0]
        ran_b += stats[4]
    assert n_te >= 10                     # (CPU oracle chain: tir 14, helitron 19, non_ltr 16)
    assert ran_a > 0 and ran_b > 0        # both the truncated-first and the full pass ran


def test_util_mirror_file_contracts(ctx, tmp_path):
    """the host-side mirror keeps the reference's file contracts (FASTA in, FASTA out)"""
    from hite_amd import util

    util._CTX = ctx
    # flanking_seq against the golden produced by the reference (Util.py:4614)
    case = load_golden("gather")[0]
    ref = tmp_path / "genome.fa"
    fold = lambda s: "".join(ch if ch in "ACGTN" else "N" for ch in s)  # noqa: E731
    ref.write_text("".join(">%s\n%s\n" % (n, s) for n, s in zip(case["names"], case["seqs"])))
    lr = tmp_path / "lr.fa"
    lr.write_text("".join(">%s\nACGT\n" % n for n in case["flanking_in"]))
    out = tmp_path / "lr.flanked.fa"
    util.flanking_seq(str(lr), str(out), str(ref), 50)
    names, contigs = util.read_fasta(str(out))
    assert [[n, contigs[n]] for n in names] == [[n, fold(s)] for n, s in case["flanking_out"]]
    # remove_sparse_col + judge through files
    jc = [c for c in load_golden("judge_tir") if c["expected"][0] is True][0]
    aln = tmp_path / "x.maf.fa"
    aln.write_text("".join(">%s\n%s\n" % (n, s) for n, s in zip(jc["names"], jc["seqs"])))
    clean = util.remove_sparse_col_in_align_file(str(aln))
    cn, cc = util.read_fasta(clean)
    assert [cc[n] for n in cn] == jc["clean"]
    got = util.judge_boundary_v5(jc["cand"], clean, 0, "tir", jc["plant"], "cons")
    assert list(got) == jc["expected"]
    # flank_region_align_v5: candidates + copy table -> real_TEs / low-copy files
    import synth_small

    g = synth_small.make(5, n_fam=10)
    gref = tmp_path / "g.fa"
    gref.write_text("".join(">c%d\n%s\n" % (i, s) for i, s in enumerate(g["contigs"])))
    cand = tmp_path / "cand.fa"
    cand.write_text("".join(">q%d\n%s\n" % (i, s) for i, s in enumerate(g["cands"])))
    copies = {"q%d" % i: [("c%d" % c, a, b, b - a + 1, "-" if m else "+") for (c, a, b, m) in cp] for i, cp in enumerate(g["copies"])}
    real, low = tmp_path / "real.fa", tmp_path / "low.fa"
    t, l = util.flank_region_align_v5(str(cand), str(real), 50, str(gref), None, "tir", str(tmp_path), 1, 0, None, "", 1, 0, 0,
                                      str(low), all_copies=copies)
    rn, rc = util.read_fasta(str(real))
    assert set(rn) == set(t.keys()) and len(t) + len(l) >= 3
    assert all(len(s) >= 80 for s in rc.values())


def test_tsd_kmer_golden_and_oracle(ctx):
    from test_oracle_golden import check_tir_items

    cases = load_golden("tir_kmer") + load_golden("tir_kmer_edge")
    for plant in (0, 1):
        sub = [c for c in cases if c["plant"] == plant]
        got = ctx.tsd_kmer([c["seq"] for c in sub], flank=50, plant=plant)
        for c, recs in zip(sub, got):
            seq = c["seq"]
            assert recs == O.tir_kmer(seq, c["flank"] + 1, len(seq) - c["flank"], c["flank"], plant)
            items = sorted([d, seq[ts - k:ts], seq[ts:te + 1]] for (k, ts, te, d) in recs)
            check_tir_items(items, c)
    # fresh seeds vs the oracle
    seqs = []
    for i in range(200):
        s, fl = casegen.make_tir_candidate(90000 + i, te_len=int(100 + 37 * (i % 40)), tsd_len=[2, 3, 4, 5, 6, 8, 9, 10, 11][i % 9],
                                           off_l=(i * 7) % 45 - 20, off_r=(i * 11) % 45 - 20, with_n=(i % 9 == 0))
        seqs.append(s)
    got = ctx.tsd_kmer(seqs, flank=50, plant=1)
    for s, recs in zip(seqs, got):
        assert recs == O.tir_kmer(s, 51, len(s) - 50, 50, 1)


def _fmea_gpu(ctx, rows, skip_gap, max_len):
    h = O.hsp_arrays([tuple(r) for r in rows])
    oc, os_, oe = ctx.fmea_chain(h["qseg"], h["sseg"], h["qs"], h["qe"], h["ss"], h["se"], h["seg_chrom"], h["seg_off"], skip_gap, max_len)
    return ["%s:%d-%d" % (h["chrom_names"][c], s, e) for c, s, e in zip(oc, os_, oe)], h


def test_fmea_golden(ctx):
    for case in load_golden("fmea"):
        got, _ = _fmea_gpu(ctx, case["rows"], case["skip_gap"], case["max_len"])
        assert got == case["expected"]


def test_fmea_random_vs_oracle(ctx):
    for seed in range(40, 52):
        rows = casegen.make_hsp_table(seed, n_seg=3 + seed % 3, n_fam=8 + seed % 7, noise=60, frag=(1, 5), dup=seed % 4 * 10,
                                      copies=(2, 10 + seed % 9))
        for gap, mx in ((2000, 30000), (300, 8000)):
            got, h = _fmea_gpu(ctx, rows, gap, mx)
            assert got == O.fmea(h, gap, mx)
    # a larger stress table: ~60k HSPs
    rows = casegen.make_hsp_table(7, n_seg=6, n_fam=60, noise=2000, frag=(1, 4), copies=(4, 22))
    got, h = _fmea_gpu(ctx, rows, 2000, 30000)
    assert len(rows) > 20000 and got == O.fmea(h, 2000, 30000)


def test_find_copies_vs_twin(ctx):
    import synth_small

    for seed, nf in ((11, 16), (23, 24), (5, 10)):
        g = synth_small.make(seed, n_fam=nf)
        ctx.genome_pack(g["contigs"])
        ctx.release_copy_index()  # new genome -> new index
        cands = list(g["cands"]) + ["ACGT" * 3, "A" * 40, g["contigs"][0][5000:5400]]  # too short / low complexity / unique region
        got = ctx.find_copies(cands)
        exp = O.find_copies(g["contigs"], cands)
        assert got == exp
        assert sum(len(x) for x in got) > 20
    # the found copies drive the fine stage to the same calls as the oracle chain on the same table
    import oracle_pipeline as OP

    g = synth_small.make(11, n_fam=16)
    ctx.genome_pack(g["contigs"])
    ctx.release_copy_index()
    tab = ctx.find_copies(g["cands"], clips=True)
    res, _ = ctx.flank_region_align("tir", g["cands"], tab, plant=1)
    for cand, cp, r in zip(g["cands"], tab, res):
        assert [r[0], r[1], r[2], r[3]] == OP.fine_stage_candidate("tir", cand, cp, g["contigs"], plant=1)


def test_find_copies_restricted_index(ctx):
    """hite_find_copies_restricted (index built from the genome minimizers the candidates look up, stage 3.1's masking step):
    the same copy table as the full index and the twin, on a fresh handle and on a reused one; every other use of the handle
    afterwards (another candidate set, all-vs-all seeding) sees the full index again."""
    import synth_small

    for seed, nf in ((11, 16), (23, 24)):
        g = synth_small.make(seed, n_fam=nf)
        ctx.genome_pack(g["contigs"])
        ctx.release_copy_index()
        cands = list(g["cands"]) + ["ACGT" * 3, "A" * 40, g["contigs"][0][5000:5400]]
        exp = O.find_copies(g["contigs"], cands)
        got = ctx.find_copies(cands, restricted=True)           # fresh handle: no full index was ever built
        st = ctx.copy_stats()
        assert got == exp
        assert st[0] > 0
        half = cands[: len(cands) // 2]
        assert ctx.find_copies(half, restricted=True) == exp[: len(half)]      # same handle, other set: rebuilt for it
        other = [g["contigs"][-1][3000:3600]] + cands[::-1]
        assert ctx.find_copies(other) == O.find_copies(g["contigs"], other)     # plain call after a restricted one: full index
        full = ctx.seed_allvsall(seg_len=1_000_000)
        ctx.find_copies(cands[:3], restricted=True)
        again = ctx.seed_allvsall(seg_len=1_000_000)                            # seeding after a restricted build: full index
        for k in ("qseg", "sseg", "qs", "qe", "ss", "se"):
            assert np.array_equal(full[k], again[k])
        assert list(full["stats"]) == list(again["stats"]) and full["stats"][0] > 0
    # nothing to look up: empty set, candidates without a valid k-mer
    assert ctx.find_copies([], restricted=True) == []
    assert ctx.find_copies(["ACGT", "N" * 100], restricted=True) == [[], []]


def test_index_build_from_kept_minimizer_tiles(ctx):
    """the index build keeps its minimizer tiles; a build on the same genome state redoes only the tiles hite_genome_mask touched since
    (restricted index -> copies -> mask -> full index: stage 3.1's prev_TE step).  The index behind it must be the one a fresh context
    builds from the masked genome: copy tables, all-vs-all HSP table (every index entry and its rank) -- with masks at contig starts and
    ends, across tile borders (2048 window starts) and a second mask call on top; and HITE_KEEP_MINIMIZERS=0 (no kept tiles) agrees"""
    import subprocess
    import sys as _sys

    import synth_small
    from hite_amd import _lib

    g = synth_small.make(31, n_fam=20)
    contigs = list(g["contigs"])
    cands = list(g["cands"])
    ctx.genome_pack(contigs)
    ctx.release_copy_index()
    first = ctx.find_copies(cands[:8], restricted=True)          # full tile pass, tiles kept, restricted index filtered from them
    assert first == O.find_copies(contigs, cands[:8])
    assert ctx.find_copies(cands[4:12], restricted=True) == O.find_copies(contigs, cands[4:12])      # kept tiles, another filter
    lens = [len(c) for c in contigs]
    masks = [(0, 1, 30), (0, 2040, 2060), (0, 4090, 6200), (0, lens[0] - 25, lens[0]), (1, 1, 1), (1, 2047, 2049), (len(contigs) - 1, lens[-1] - 3000, lens[-1] + 50)]
    rng = np.random.default_rng(5)
    for _ in range(40):
        c = int(rng.integers(0, len(contigs)))
        a = int(rng.integers(1, lens[c]))
        masks.append((c, a, min(lens[c], a + int(rng.integers(1, 900)))))

    def masked(cs, ms):
        arrs = [np.frombuffer(c.encode(), dtype=np.uint8).copy() for c in cs]
        for c, s1, e1 in ms:
            arrs[c][max(0, s1 - 1):e1] = ord("N")
        return [a.tobytes().decode() for a in arrs]

    ctx.genome_mask([m[0] for m in masks], [m[1] for m in masks], [m[2] for m in masks])
    got_tab = ctx.find_copies(cands)                              # full index from kept tiles + the masked ones redone
    got_hsp = ctx.seed_allvsall(seg_len=1_000_000)
    more = [(0, 3000, 3100), (2, 1, 5000)]
    ctx.genome_mask([m[0] for m in more], [m[1] for m in more], [m[2] for m in more])
    got_tab2 = ctx.find_copies(cands[:6], restricted=True)        # second mask on top, restricted build from kept tiles
    ctx.copy_index_build()
    got_hsp2 = ctx.seed_allvsall(seg_len=1_000_000)
    fresh = _lib.Context(0)
    try:
        m1 = masked(contigs, masks)
        fresh.genome_pack(m1)
        assert got_tab == fresh.find_copies(cands) == O.find_copies(m1, cands)
        exp_hsp = fresh.seed_allvsall(seg_len=1_000_000)
        m2 = masked(m1, more)
        fresh.genome_pack(m2)
        fresh.release_copy_index()
        assert got_tab2 == fresh.find_copies(cands[:6]) == O.find_copies(m2, cands[:6])
        exp_hsp2 = fresh.seed_allvsall(seg_len=1_000_000)
    finally:
        fresh.close()
    for a, b in ((got_hsp, exp_hsp), (got_hsp2, exp_hsp2)):
        for k in ("qseg", "sseg", "qs", "qe", "ss", "se"):
            assert np.array_equal(a[k], b[k]), k
        assert list(a["stats"]) == list(b["stats"]) and a["stats"][0] > 0
    if os.environ.get("HITE_KEEP_MINIMIZERS") != "0":
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        rc = subprocess.run([_sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_parity.py"), "-x", "-q", "-m", "gpu", "-k",
                             "kept_minimizer_tiles or restricted_index or mask_genome_intactTE"], env=dict(os.environ, HITE_KEEP_MINIMIZERS="0"),
                            capture_output=True, text=True, cwd=root)
        assert rc.returncode == 0, rc.stdout[-3000:] + rc.stderr[-2000:]


def test_find_copies_interval_modes(ctx):
    """The records carry the ALIGNED interval, reference_start + 1 .. reference_end as get_copies_minimap2 reports it (Util.py:8026;
    the default since round 5), or -- hite_copy_config(0) / HITE_COPY_INTERVAL=whole -- the interval of the whole candidate (rounds
    2-4).  Both modes are twin-pinned; the aligned intervals lie inside the whole-candidate ones, copy for copy."""
    import synth_small

    g = synth_small.make(23, n_fam=24)
    ctx.genome_pack(g["contigs"])
    ctx.release_copy_index()
    aligned = ctx.find_copies(g["cands"])
    assert aligned == O.find_copies(g["contigs"], g["cands"])
    try:
        ctx.copy_config(False)
        O.find_copies_config(False)
        whole = ctx.find_copies(g["cands"])
        assert whole == O.find_copies(g["contigs"], g["cands"])
    finally:
        ctx.copy_config(None)
        O.find_copies_config(None)
    assert ctx.find_copies(g["cands"]) == aligned == O.find_copies(g["contigs"], g["cands"])
    n_shorter = 0
    for w, a in zip(whole, aligned):
        assert len(w) == len(a)                    # the same chains are accepted: the two filters do not see the mode
        key = lambda t: (t[0], t[3], t[4])         # noqa: E731  (contig, strand, anchors)
        for x in a:
            inside = [y for y in w if key(y) == key(x) and y[1] <= x[1] and x[2] <= y[2]]
            assert inside, (x, w)
            n_shorter += min(y[2] - y[1] for y in inside) > x[2] - x[1]
    assert n_shorter > 0                           # some copies were clipped: their aligned interval is shorter


def test_edge_cases(ctx):
    """empty / ragged / degenerate inputs the reference also meets: empty batches, single-row and
    two-row alignments, candidates without copies, candidates shorter than the 20-bp anchor, copies at contig ends"""
    # empty batches
    assert ctx.sparse_cols([]) == []
    assert ctx.judge("tir", [], [], plant=1) == []
    assert ctx.tsd_kmer([], 50, 1) == []
    oc, os_, oe = ctx.fmea_chain([], [], [], [], [], [], [0], [0], 2000, 30000)
    assert len(oc) == 0
    # FMEA: only self hits / a single HSP
    rows = [("chr1$0", "chr1$0", 1, 1000000, 1, 1000000)]
    got, h = _fmea_gpu(ctx, rows, 2000, 30000)
    assert got == O.fmea(h, 2000, 30000) == []
    rows = [("chr1$0", "chr1$1000000", 100, 500, 7000, 7400)]
    got, h = _fmea_gpu(ctx, rows, 2000, 30000)
    assert got == O.fmea(h, 2000, 30000) and len(got) == 1
    # single-row / two-row alignments and a short candidate
    base = casegen.make_msa_case(seed=4, te_type="tir", rows=6, te_len=150, tsd_len=8, tsd_frac=1.0)
    m = O.msa_array(base["seqs"])
    for sub, cand in ((m[:1], base["cand"]), (m[:2], base["cand"]), (m, base["cand"][:12]), (m, "ACGTACGTAC")):
        for te in ("tir", "helitron", "non_ltr"):
            g = ctx.judge(te, [np.ascontiguousarray(sub)], [cand], plant=1)[0]
            e, _ = O.judge(te, np.ascontiguousarray(sub), cand, 1)
            if e[0] == "EXC":
                assert g[1] == "EXC"
            else:
                assert [g[0], g[1], g[2], g[3]] == e
    # candidates without any usable copy, copies hanging over contig ends
    names, seqs = casegen.make_genome(3, n_chr=2, chr_len=(5000, 6000), other_frac=0.0)
    ctx.genome_pack(seqs)
    cands = [seqs[0][1000:1300], seqs[1][200:700], "ACGT" * 40]
    copies = [[], [(1, 1, 40, 0), (1, len(seqs[1]) - 30, len(seqs[1]), 1), (1, 201, 700, 0)], [(0, 10, 20, 0)]]
    res, _ = ctx.flank_region_align("tir", cands, copies, plant=1)
    import oracle_pipeline as OP

    for cand, cp, r in zip(cands, copies, res):
        assert [r[0], r[1], r[2], r[3]] == OP.fine_stage_candidate("tir", cand, cp, seqs, plant=1)
    assert ctx.flank_region_align("tir", [], [], plant=1)[0] == []


def test_max_size_alignment(ctx):
    """the full-length pass at max_single_repeat_len: 30 kb windows (C-ABI limit 32767) through alignment and judge"""
    rng = np.random.default_rng(99)
    L = 30000
    cons = casegen.rand_seq(rng, 14)
    cons = cons + casegen.rand_seq(rng, L - 28) + casegen.revcomp(cons[:14])
    wins = []
    for r in range(4):
        s = casegen.mutate(rng, cons, 0.04 if r else 0.0)
        if r == 2:
            s = s[:12000] + s[12040:]          # a 40-bp deletion
        if r == 3:
            s = s[:20000] + casegen.rand_seq(rng, 25) + s[20000:]  # a 25-bp insertion
        t = casegen.rand_seq(rng, 9)
        wins.append(casegen.rand_seq(rng, 41) + t + s + t + casegen.rand_seq(rng, 41))
    got = ctx.star_msa([wins])[0]
    exp = O.star_msa(wins)
    assert got is not None and exp is not None and np.array_equal(got, exp)
    clean = ctx.sparse_cols([got])[0]
    kc = O.sparse_cols(exp).astype(bool)
    assert np.array_equal(clean, exp[:, kc])
    cand = wins[0][50 - 3: 50 + L + 2]
    g = ctx.judge("tir", [clean], [cand], plant=1)[0]
    e, _ = O.judge("tir", np.ascontiguousarray(exp[:, kc]), cand, 1)
    assert [g[0], g[1], g[2], g[3]] == e


def test_dropin_scripts(ctx, tmp_path):
    """argv-compatible stage scripts: coarse_boundary (HSP table -> FMEA -> flanks) and judge_TIR (flanked
    candidates -> confident_tir_{i}.fa) keep the reference's file contract"""
    import subprocess
    import sys as _sys

    import synth_small

    root = __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__)))
    g = synth_small.make(21, n_fam=10, n_chr=2, chr_len=150_000)
    ref = tmp_path / "genome.fa"
    ref.write_text("".join(">chr%d\n%s\n" % (i + 1, s) for i, s in enumerate(g["contigs"])))
    # coarse stage from an HSP table
    rows = casegen.make_hsp_table(3, n_seg=1, n_fam=6, seg_len=140_000, noise=10, chroms=("chr1", "chr2"))
    hsp = tmp_path / "0.fa.final.out"
    hsp.write_text("".join(casegen.hsp_to_blast6_lines(rows)))
    out = tmp_path / "out"
    rc = subprocess.run([_sys.executable, root + "/hite_amd/scripts/coarse_boundary.py", "-g", str(ref), "-r", str(ref),
                         "--tmp_output_dir", str(out), "--ref_index", "0", "--fixed_extend_base_threshold", "2000",
                         "--max_repeat_len", "30000", "--thread", "1", "--flanking_len", "50", "--recover", "0",
                         "--hsp", str(hsp)], capture_output=True, text=True)
    assert rc.returncode == 0, rc.stderr
    from hite_amd import util

    names, _ = util.read_fasta(str(out / "longest_repeats_0.fa"))
    h = O.hsp_arrays([tuple(r) for r in rows])
    assert names == O.fmea(h, 2000, 30000)
    fn, fc = util.read_fasta(str(out / "longest_repeats_0.flanked.fa"))
    assert len(fn) == len(names) and all(len(fc[n]) >= 180 for n in fn)
    # fine stage: flanked candidates of the planted families
    flanked = tmp_path / "cand.flanked.fa"
    recs = []
    for i, (cand, cps) in enumerate(zip(g["cands"], g["copies"])):
        c, a, b, m = cps[0]
        s = g["contigs"][c][a - 1 - 50:b + 50]
        recs.append(">chr%d:%d-%d\n%s\n" % (c + 1, a - 50, b + 50, s))
    flanked.write_text("".join(recs))
    rc = subprocess.run([_sys.executable, root + "/hite_amd/scripts/judge_TIR_transposons.py", "--seqs", str(flanked), "-t", "1",
                         "--tmp_output_dir", str(out), "--ref_index", "0", "--plant", "1", "--flanking_len", "50", "--recover", "0",
                         "-r", str(ref), "--min_TE_len", "80"], capture_output=True, text=True)
    assert rc.returncode == 0, rc.stderr
    assert "itrsearch" not in rc.stderr      # the terminal-inverted-repeat filter is an in-tree stage: never skipped, never announced missing
    tn, tc = util.read_fasta(str(out / "confident_tir_0.fa"))
    assert len(tn) >= 2 and all(n.startswith("genome-TIR_0_") for n in tn)
    # the filter at work (search_confident_tir_batch_v1, Util.py:6598-6600): windows without a terminal inverted repeat leave the
    # candidate set, the planted TIR families stay
    fnames, fcontigs = util.read_fasta(str(flanked))
    rng_d = np.random.default_rng(6598)
    decoys = {}
    for k in range(40):
        c = int(rng_d.integers(0, len(g["contigs"])))
        p0 = int(rng_d.integers(200, len(g["contigs"][c]) - 1200))
        decoys["chr%d:%d-%d" % (c + 1, p0 + 1, p0 + 700)] = g["contigs"][c][p0:p0 + 700]
    allc = dict(fcontigs)
    allc.update(decoys)
    util._CTX = ctx
    kept = util.search_confident_tir_batch_v1(list(allc), allc, 50, 1)
    kept_q = {k.split("-tir_")[0] for k in kept}
    assert len(kept_q & set(fnames)) >= 0.8 * len(fnames)
    assert len(kept_q & set(decoys)) <= 0.3 * len(decoys), sorted(kept_q & set(decoys))
    # Helitron / non-LTR wrappers: same file contract (the synthetic TIR families are not expected to pass their rules)
    candf = tmp_path / "cand.fa"
    candf.write_text("".join(">c%d\n%s\n" % (i, s) for i, s in enumerate(g["cands"])))
    for script, outname in (("judge_Helitron_transposons.py", "confident_helitron_0.fa"), ("judge_Non_LTR_transposons.py", "confident_non_ltr_0.fa")):
        rc = subprocess.run([_sys.executable, root + "/hite_amd/scripts/" + script, "--seqs", str(flanked), "-t", "1", "--tmp_output_dir", str(out),
                             "--ref_index", "0", "--flanking_len", "50", "--recover", "0", "-r", str(ref), "--min_TE_len", "80",
                             "--candidates", str(candf)], capture_output=True, text=True)
        assert rc.returncode == 0, rc.stderr[-2000:]
        assert (out / outname).exists()
    # homology module: library entries = planted families (one mutated, one absent from the genome) -> longest genomic copy each
    lib = tmp_path / "non_LTR.lib"
    rng = np.random.default_rng(3)
    ent = [(">fam%d#LINE/L1\n" % i) + (s if i != 1 else casegen.mutate(rng, s, 0.02)) + "\n" for i, s in enumerate(g["cands"][:5])]
    ent.append(">absent#SINE/tRNA\n" + casegen.rand_seq(rng, 400) + "\n")
    lib.write_text("".join(ent))
    rc = subprocess.run([_sys.executable, root + "/hite_amd/scripts/judge_Other_transposons.py", "-t", "1", "--tmp_output_dir", str(out),
                         "--recover", "0", "-r", str(ref), "--min_TE_len", "80", "--lib", str(lib)], capture_output=True, text=True)
    assert rc.returncode == 0, rc.stderr[-2000:]
    on, oc_ = util.read_fasta(str(out / "confident_other.fa"))
    assert 3 <= len(on) <= 5 and all(n.startswith("Homology_Non_LTR_") and n.endswith("#LINE/L1") for n in on)
    genome_text = "".join(g["contigs"])
    for n in on:
        assert oc_[n] in genome_text or util.getReverseSequence(oc_[n]) in genome_text   # a genomic copy, verbatim


def test_star_msa_sparse_fused(ctx):
    """fused alignment + sparse-column removal == twin alignment followed by the oracle's remove_sparse_col
    (first / last column rules, insertion blocks that survive as prefixes, few-row groups)"""
    groups = _families(4242, 60, rows_choices=(1, 2, 3, 4, 7, 30, 101), lens=(60, 200, 700))
    rng = np.random.default_rng(5)
    # groups whose rows all carry the same leading / trailing insertions (the first / last column is an insertion column)
    for _ in range(12):
        L = int(rng.integers(40, 200))
        centre = "".join("ACGT"[i] for i in rng.integers(0, 4, L))
        rows = [centre]
        for _r in range(int(rng.integers(1, 9))):
            pre = "".join("ACGT"[i] for i in rng.integers(0, 4, int(rng.integers(0, 4))))
            suf = "".join("ACGT"[i] for i in rng.integers(0, 4, int(rng.integers(0, 4))))
            mid = int(rng.integers(5, L - 5))
            ins = "".join("ACGT"[i] for i in rng.integers(0, 4, int(rng.integers(0, 3))))
            rows.append(pre + centre[:mid] + ins + centre[mid:] + suf)
        groups.append(rows)
    got = ctx.star_msa(groups, sparse=True)
    full = ctx.star_msa(groups)
    for g, m, f in zip(groups, got, full):
        exp_full = O.star_msa(g)
        assert f is not None and np.array_equal(f, exp_full)
        keep = O.sparse_cols(exp_full).astype(bool)
        exp = np.ascontiguousarray(exp_full[:, keep])
        assert m is not None and m.shape == exp.shape, (m.shape if m is not None else None, exp.shape, len(g))
        assert np.array_equal(m, exp)


def test_star_msa_padded_rows(ctx):
    """rows that begin / end with HITE_ROW_PAD (include/hite_gpu.h): the pads are aligned as bases that match nothing and leave the
    alignment as gaps of the row -- HIP == twin, full and sparse form; the ungapped rows are the windows WITHOUT their pads; a row
    cut short at either end and padded by what is missing aligns like the whole row with those bases blanked"""
    rng = np.random.default_rng(99)
    base = _families(515, 30, rows_choices=(2, 5, 12, 40), lens=(150, 400, 1200))
    groups = []
    for g in base:
        rows = [g[0]]
        c0 = g[0]
        for w in g[1:]:
            a, b = (int(x) for x in rng.integers(0, 70, 2))
            kind = int(rng.integers(0, 4))
            # the two kinds of pad byte: '.' (matches nothing) and the centre's own bases in lower case (match what they face)
            pa, pb = ("." * a, "." * b) if rng.random() < 0.4 else (c0[:a].lower(), c0[len(c0) - b:].lower() if b else "")
            if kind == 0:
                rows.append(w)                                              # no pads
            elif kind == 1:
                rows.append(pa + w[min(a, len(w) // 3):])                   # cut in front, padded by what was cut (or more)
            elif kind == 2:
                rows.append(w[: len(w) - min(b, len(w) // 3)] + pb)         # cut behind
            else:
                rows.append(pa + w[min(a, len(w) // 3): len(w) - min(b, len(w) // 3)] + pb)
        groups.append(rows)
    groups.append(["ACGTTGCAAGGCTTAACCGGTTAAGC" * 4, "." * 104, "." * 5 + "ACGTTGCAAGGCTTAACCGGTTAAGC"[5:] + "ACGTTGCAAGGCTTAACCGGTTAAGC" + "." * 52])     # a row of pads only
    full = ctx.star_msa(groups)
    sparse = ctx.star_msa(groups, sparse=True)
    n_pad_rows = 0
    for g, f, m in zip(groups, full, sparse):
        exp_full = O.star_msa(g)
        assert f is not None and f.shape == exp_full.shape and np.array_equal(f, exp_full)
        assert not (f & 0x20)[f != ord("-")].any()             # no pad byte is left ('-' itself has bit 5)
        if f.shape[0] == len(g):                 # (a row that cannot be aligned leaves, on both sides alike)
            for r, w in enumerate(g):
                assert bytes(f[r][f[r] != ord("-")]) == w.strip(".acgtn").encode()
        n_pad_rows += sum(w != w.strip(".acgtn") for w in g)
        keep = O.sparse_cols(exp_full).astype(bool)
        exp = np.ascontiguousarray(exp_full[:, keep])
        assert m is not None and m.shape == exp.shape and np.array_equal(m, exp)
    assert n_pad_rows > 100


def test_aligned_interval_mode_pads_the_rows(ctx):
    """Records in the reference's coordinates (the aligned interval of Util.py:8026, the default) carry the candidate bases the end
    extensions clipped; hite_flank_region_align_clip pads the rows with them.  Pinned: clip words HIP == twin, the fused pipeline ==
    the oracle chain on the padded windows -- and the calls do not fall behind the whole-candidate mode's."""
    import oracle_pipeline as OP
    import synth_small

    g = synth_small.make(23, n_fam=24)
    ctx.genome_pack(g["contigs"])
    ctx.release_copy_index()
    try:
        ctx.copy_config(False)
        O.find_copies_config(False)
        whole = ctx.find_copies(g["cands"], clips=True)
        assert whole == O.find_copies(g["contigs"], g["cands"], clips=True)
    finally:
        ctx.copy_config(None)
        O.find_copies_config(None)
    assert all(cp[5] == 0 for t in whole for cp in t)            # whole-candidate intervals: nothing to pad
    res_whole, _ = ctx.flank_region_align("tir", g["cands"], whole, plant=1)
    tab = ctx.find_copies(g["cands"], clips=True)
    assert tab == O.find_copies(g["contigs"], g["cands"], clips=True)
    assert sum(cp[5] != 0 for t in tab for cp in t) > 20
    res, _ = ctx.flank_region_align("tir", g["cands"], tab, plant=1)
    for cand, cp, r in zip(g["cands"], tab, res):
        assert [r[0], r[1], r[2], r[3]] == OP.fine_stage_candidate("tir", cand, cp, g["contigs"], plant=1)
    # without the clip words the same records are aligned globally, as before (and as an external copy table would be)
    bare = [[cp[:4] for cp in t] for t in tab]
    res_bare, _ = ctx.flank_region_align("tir", g["cands"], bare, plant=1)
    for cand, cp, r in zip(g["cands"], bare, res_bare):
        assert [r[0], r[1], r[2], r[3]] == OP.fine_stage_candidate("tir", cand, cp, g["contigs"], plant=1)
    te = lambda rr: sum(bool(r[0]) for r in rr)  # noqa: E731
    print("TE calls: whole-candidate %d, aligned + pads %d, aligned without pads %d of %d" % (te(res_whole), te(res), te(res_bare), len(res)))
    assert te(res) >= te(res_bare) and te(res) >= 0.9 * te(res_whole)


def test_table_without_clip_words_is_probed_wherever_it_lives(ctx):
    """hite_find_copies_dev -> hite_flank_region_align_dev without a clip pointer (the call sequence of rounds 1-4): the clip words are
    ESTIMATED from the sequences (clip_probe_kernel) -- for the finder's own device table exactly as for a copy of it elsewhere; round
    5 recognised the finder's table by its address and took the finder's words, which made the result depend on where an array lived"""
    import synth_small
    import torch
    from hite_amd._lib import CALL_DTYPE

    g = synth_small.make(23, n_fam=24)
    ctx.genome_pack(g["contigs"])
    ctx.release_copy_index()
    ctx.copy_index_build()
    dev = torch.device("cuda", 0)
    cb = [c.encode() for c in g["cands"]]
    off = np.zeros(len(cb) + 1, dtype=np.int64)
    np.cumsum([len(c) for c in cb], out=off[1:])
    d_cand = torch.from_numpy(np.frombuffer(b"".join(cb) + b"\0" * 64, dtype=np.uint8).copy()).to(dev)
    d_off = torch.from_numpy(off).to(dev)
    n, nbytes = len(cb), int(off[-1])
    cap = nbytes + 200 * n + 4096
    outs = []
    for mode in ("finder's table", "explicit", "a copy of it"):
        d_calls = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
        d_cons = torch.zeros(cap + 64, dtype=torch.uint8, device=dev)
        nc, p_cf, p_ct, p_s1, p_e1, p_mn, _an = ctx.find_copies_dev(n, d_cand.data_ptr(), d_off.data_ptr(), nbytes)
        if mode == "a copy of it":
            s1 = torch.from_numpy(ctx.download(p_s1, nc, np.int64)).to(dev)
            p_s1 = s1.data_ptr()
        ctx.flank_region_align_dev("tir", 1, n, d_cand.data_ptr(), d_off.data_ptr(), p_cf, nc, p_ct, p_s1, p_e1, p_mn, 50, d_calls.data_ptr(),
                                   d_cons.data_ptr(), cap, d_clip=ctx.copy_clips_dev() if mode == "explicit" else 0)
        torch.cuda.synchronize()
        calls = d_calls.cpu().numpy().view(CALL_DTYPE).copy()
        cons = d_cons.cpu().numpy()
        outs.append([(int(c["is_te"]), cons[c["cons_off"]:c["cons_off"] + c["cons_len"]].tobytes() if c["is_te"] else b"") for c in calls])
    assert outs[0] == outs[2]
    print("no clip pointer: the finder's own table == a copy of it; against the finder's clip words %d of %d calls differ (%d / %d TE calls)"
          % (sum(a != b for a, b in zip(outs[0], outs[1])), n, sum(a[0] for a in outs[0]), sum(a[0] for a in outs[1])))


def test_reference_tuples_clip_probe_vs_twin(ctx):
    """A copy table in the reference's own form -- (chr, reference_start + 1, reference_end, length, strand), Util.py:8022-8030: no clip
    words -- through hite_flank_region_align: (1) the estimated words, hite_clip_probe == orc_clip_probe record for record (both strands,
    records at contig ends, intervals shorter than two probes); (2) they are close to what the copy finder knows (its end extensions'
    clips); (3) the whole stage on the 5-tuples == the oracle chain, which estimates by the same rule"""
    import oracle_pipeline as OP
    import synth_small

    g = synth_small.make(29, n_fam=20)
    ctx.genome_pack(g["contigs"])
    ctx.release_copy_index()
    full = ctx.find_copies(g["cands"], clips=True)
    assert full == O.find_copies(g["contigs"], g["cands"], clips=True)
    # the reference's tuple: (chr, start, end, aligned length, strand) -- here with the contig as its index and the strand as 0 / 1
    ref5 = [[(t[0], t[1], t[2], t[3], t[2] - t[1] + 1) for t in cp] for cp in full]
    hand = [(0, 1, 30, 0, 30), (0, 5, 60, 1, 56), (len(g["contigs"]) - 1, max(1, len(g["contigs"][-1]) - 39), len(g["contigs"][-1]), 1, 40)]
    ref5[0] = ref5[0] + hand
    got = ctx.clip_probe(g["cands"], ref5)
    n_rec = n_near = n_nonzero = 0
    for cand, cps, words, cpf in zip(g["cands"], ref5, got, full):
        for k, (t, w) in enumerate(zip(cps, words)):
            pr = O.clip_probe(cand, OP._interval(g["contigs"][t[0]], t[1], t[2], t[3]))
            exp = ((pr >> 16) | ((pr & 0xffff) << 16)) if t[3] else pr
            assert w == exp, (t, w, exp)
            if k < len(cpf):
                n_rec += 1
                n_nonzero += cpf[k][5] != 0
                n_near += abs((w & 0xffff) - (cpf[k][5] & 0xffff)) <= 3 and abs((w >> 16) - (cpf[k][5] >> 16)) <= 3
    assert n_nonzero >= 20 and n_near >= 0.85 * n_rec, (n_rec, n_nonzero, n_near)
    ref5[0] = ref5[0][:-len(hand)]
    res, _ = ctx.flank_region_align("tir", g["cands"], ref5, plant=1)
    n_te = 0
    for cand, cp, r in zip(g["cands"], ref5, res):
        assert [r[0], r[1], r[2], r[3]] == OP.fine_stage_candidate("tir", cand, cp, g["contigs"], plant=1)
        n_te += r[0]
    res6, _ = ctx.flank_region_align("tir", g["cands"], full, plant=1)
    print("reference tuples: %d records, %d with a clip, estimate within 3 bases of the finder's at both ends for %d; TE calls %d (with the finder's words: %d) of %d"
          % (n_rec, n_nonzero, n_near, n_te, sum(r[0] for r in res6), len(res)))
    assert n_te >= 0.9 * sum(r[0] for r in res6)


def test_clip_probe_on_a_whole_candidate_table(ctx):
    """hite_copy_config(0): the records carry the whole candidate, so nothing was clipped -- and a table passed WITHOUT clip words
    (the finder's 5-tuples on the host, the finder's device table with no clip pointer) still goes through clip_probe_kernel on
    every call.  Pinned here: the probed words are orc_clip_probe's, record for record; the stage's calls on the probed table are
    the twin chain's, and equal those of the same table with an explicit zero-filled clip array, on the host and on the device.
    The probe does NOT answer 0|0 throughout: on this genome (the neighbouring test's) the twin estimates a clip for 44 of 345
    records (12.8 %; one base at one end for 42 of them), which here leaves all 16 calls as they are with zeros -- the twin chain
    says so before the device is asked.  It is not harmless everywhere: on synth_small.make(23, n_fam=24) the twin chain builds
    one of 12 consensi two bases shorter from the probed words (65 of 396 non-zero) than from zeros; there the calls are held
    to the twin's for each form, not to each other."""
    import oracle_pipeline as OP
    import synth_small
    import torch
    from hite_amd._lib import CALL_DTYPE

    def words_of_twin(g, tab):
        out = []
        for cand, cps in zip(g["cands"], tab):
            ws = []
            for t in cps:
                pr = O.clip_probe(cand, OP._interval(g["contigs"][t[0]], t[1], t[2], t[3]))
                ws.append(((pr >> 16) | ((pr & 0xffff) << 16)) if t[3] else pr)
            out.append(ws)
        return out

    dev = torch.device("cuda", 0)
    try:
        ctx.copy_config(False)
        O.find_copies_config(False)
        for seed, n_fam, harmless in ((29, 20, True), (23, 24, False)):
            g = synth_small.make(seed, n_fam=n_fam)
            ctx.genome_pack(g["contigs"])
            ctx.release_copy_index()
            whole = ctx.find_copies(g["cands"], clips=True)
            assert whole == O.find_copies(g["contigs"], g["cands"], clips=True)
            assert all(cp[5] == 0 for t in whole for cp in t) and sum(len(t) for t in whole) > 300
            ref5 = [[(t[0], t[1], t[2], t[3], t[2] - t[1] + 1) for t in cp] for cp in whole]
            zero6 = [[t[:5] + (0,) for t in cp] for cp in whole]
            exp_words = words_of_twin(g, ref5)
            assert ctx.clip_probe(g["cands"], ref5) == exp_words
            flat = [w for ws in exp_words for w in ws]
            n_nonzero = sum(w != 0 for w in flat)
            print("whole-candidate table, seed %d: the probe estimates a clip for %d of %d records" % (seed, n_nonzero, len(flat)))
            assert 0 < n_nonzero < 0.2 * len(flat)           # (the twin does not say 0|0 throughout: equality with the twin is the contract)
            exp5 = [OP.fine_stage_candidate("tir", cand, cp, g["contigs"], plant=1) for cand, cp in zip(g["cands"], ref5)]
            exp0 = [OP.fine_stage_candidate("tir", cand, cp, g["contigs"], plant=1) for cand, cp in zip(g["cands"], zero6)]
            assert (exp5 == exp0) == harmless, (seed, sum(a != b for a, b in zip(exp5, exp0)))
            res5, _ = ctx.flank_region_align("tir", g["cands"], ref5, plant=1)
            res0, _ = ctx.flank_region_align("tir", g["cands"], zero6, plant=1)
            assert [[r[0], r[1], r[2], r[3]] for r in res5] == exp5
            assert [[r[0], r[1], r[2], r[3]] for r in res0] == exp0
            if harmless:
                assert res5 == res0 and sum(r[0] for r in res5) >= 5
            # the device table: no clip pointer (probed) against a zero-filled clip array
            cb = [c.encode() for c in g["cands"]]
            off = np.zeros(len(cb) + 1, dtype=np.int64)
            np.cumsum([len(c) for c in cb], out=off[1:])
            d_cand = torch.from_numpy(np.frombuffer(b"".join(cb) + b"\0" * 64, dtype=np.uint8).copy()).to(dev)
            d_off = torch.from_numpy(off).to(dev)
            n, nbytes = len(cb), int(off[-1])
            cap = nbytes + 200 * n + 4096
            ctx.copy_index_build()
            outs = []
            for form in ("probed", "zeros"):
                d_calls = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
                d_cons = torch.zeros(cap + 64, dtype=torch.uint8, device=dev)
                nc, p_cf, p_ct, p_s1, p_e1, p_mn, _an = ctx.find_copies_dev(n, d_cand.data_ptr(), d_off.data_ptr(), nbytes)
                assert nc == len(flat)
                d_zero = torch.zeros(nc + 16, dtype=torch.int32, device=dev)
                torch.cuda.synchronize()
                ctx.flank_region_align_dev("tir", 1, n, d_cand.data_ptr(), d_off.data_ptr(), p_cf, nc, p_ct, p_s1, p_e1, p_mn, 50, d_calls.data_ptr(),
                                           d_cons.data_ptr(), cap, d_clip=d_zero.data_ptr() if form == "zeros" else 0)
                torch.cuda.synchronize()
                calls = ctx.download(d_calls.data_ptr(), n * 32, np.uint8).view(CALL_DTYPE)
                cons = ctx.download(d_cons.data_ptr(), cap, np.uint8)
                outs.append([[bool(c["is_te"]), cons[c["cons_off"]:c["cons_off"] + c["cons_len"]].tobytes().decode() if c["is_te"] else "", int(c["row_num"])]
                             for c in calls])
            assert outs[0] == [[e[0], e[2], e[3]] for e in exp5], seed
            assert outs[1] == [[e[0], e[2], e[3]] for e in exp0], seed
            if harmless:
                assert outs[0] == outs[1]
    finally:
        ctx.copy_config(None)
        O.find_copies_config(None)


def test_aligned_interval_mode_through_the_host_mirror(ctx, tmp_path):
    """util.get_full_length_copies_minimap2 -> util.flank_region_align_v5 (the reference's two functions, Util.py:7933 / 8032) in the
    reference-coordinate mode: the clip words travel as a 6th field of the copy tuples and the stage's calls are the direct call's"""
    import synth_small
    from hite_amd import util

    g = synth_small.make(23, n_fam=24)
    gref = tmp_path / "g.fa"
    gref.write_text("".join(">c%d\n%s\n" % (i, s) for i, s in enumerate(g["contigs"])))
    cand = tmp_path / "cand.fa"
    cand.write_text("".join(">q%d\n%s\n" % (i, s) for i, s in enumerate(g["cands"])))
    real, low = tmp_path / "real.fa", tmp_path / "low.fa"
    uctx = util.set_reference(str(gref))
    try:
        uctx.copy_config(True)      # (the default; explicit here)
        cps = util.get_full_length_copies_minimap2(str(cand), str(gref))
        assert sum(cp[5] != 0 for v in cps.values() for cp in v) > 20
        tab = uctx.find_copies(g["cands"], clips=True)
        res, _ = uctx.flank_region_align("tir", g["cands"], tab, plant=1)
        # (after the direct call: the low-copy rescue inside the stage packs other sequences into the context)
        t, l = util.flank_region_align_v5(str(cand), str(real), 50, str(gref), None, "tir", str(tmp_path), 1, 0, None, "", 1, 0, 0, str(low))
    finally:
        uctx.copy_config(None)
    direct = {"q%d" % i: r[2] for i, r in enumerate(res) if r[0]}
    both = dict(t, **l)
    assert len(direct) >= 6 and len(both) >= 3
    assert all(n in direct and s == direct[n] for n, s in both.items())     # (TG..CA consensi and unrescued low-copy ones are dropped on the way)


def test_seed_allvsall_vs_twin(ctx):
    """all-vs-all seeding (stage 3.1, the build's blastn stand-in): HIP == twin, record for record, incl. segment splits;
    the table drives FMEA to the same intervals as the oracle's FMEA on the twin's table"""
    import synth_small

    for seed, nf, seg in ((31, 10, 100_000), (7, 14, 37_000), (19, 6, 1_000_000)):
        g = synth_small.make(seed, n_fam=nf, n_chr=2, chr_len=260_000)
        ctx.genome_pack(g["contigs"])
        ctx.release_copy_index()
        got = ctx.seed_allvsall(seg_len=seg)
        exp = O.seed_allvsall(g["contigs"], seg_len=seg)
        sc, so = ctx.seed_segments(seg)
        assert np.array_equal(sc, exp["seg_chrom"]) and np.array_equal(so, exp["seg_off"])
        for k in ("qseg", "sseg", "qs", "qe", "ss", "se"):
            assert np.array_equal(got[k], exp[k]), (seed, k, len(got[k]), len(exp[k]))
        assert len(got["qseg"]) > 50 and got["stats"][3] == len(got["qseg"])
    # seeding -> FMEA on the GPU == oracle FMEA on the same table
    oc, os_, oe = ctx.fmea_chain(got["qseg"], got["sseg"], got["qs"], got["qe"], got["ss"], got["se"], sc, so, 2000, 30000)
    h = dict(got)
    h["seg_chrom"], h["seg_off"], h["chrom_names"] = sc, so, ["chr%d" % (i + 1) for i in range(2)]
    exp_names = O.fmea(h, 2000, 30000)
    assert ["chr%d:%d-%d" % (c + 1, a, b) for c, a, b in zip(oc, os_, oe)] == exp_names and len(exp_names) > 3
    # device-resident form (the HSP table never crosses PCIe): same intervals
    (oc2, os2, oe2), st2 = ctx.coarse_stage_dev(seg, sc, so, 2000, 30000)
    assert np.array_equal(oc, oc2) and np.array_equal(os_, os2) and np.array_equal(oe, oe2) and st2 == got["stats"]


def test_coarse_boundary_script_end_to_end(ctx, tmp_path):
    """stage 3.1 without external tools: chunk of 'chr$offset' segments -> all-vs-all seeding -> FMEA -> longest_repeats +
    flanked FASTA; the planted multi-copy families come out as candidate repeats"""
    import os
    import subprocess
    import sys as _sys

    import synth_small
    from hite_amd import util

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    g = synth_small.make(43, n_fam=10, n_chr=2, chr_len=300_000)
    ref = tmp_path / "genome.fa"
    ref.write_text("".join(">chr%d\n%s\n" % (i + 1, s) for i, s in enumerate(g["contigs"])))
    cut = tmp_path / "genome.cut0.fa"
    seg = 100_000
    with open(cut, "w") as f:
        for i, s in enumerate(g["contigs"]):
            for o in range(0, len(s), seg):
                f.write(">chr%d$%d\n%s\n" % (i + 1, o, s[o:o + seg]))
    out = tmp_path / "out"
    rc = subprocess.run([_sys.executable, root + "/hite_amd/scripts/coarse_boundary.py", "-g", str(cut), "-r", str(ref),
                         "--tmp_output_dir", str(out), "--ref_index", "0", "--fixed_extend_base_threshold", "1000",
                         "--max_repeat_len", "30000", "--thread", "1", "--flanking_len", "50", "--recover", "0"],
                        capture_output=True, text=True)
    assert rc.returncode == 0, rc.stderr[-2000:]
    names, seqs = util.read_fasta(str(out / "longest_repeats_0.fa"))
    fn, _fc = util.read_fasta(str(out / "longest_repeats_0.flanked.fa"))
    assert len(names) == len(fn) and len(names) > 5
    iv = []
    for n in names:
        c, pos = n.split(":")
        a, b = map(int, pos.split("-"))
        assert seqs[n] == g["contigs"][int(c[3:]) - 1][a:b] and 80 <= b - a < 30000
        iv.append((int(c[3:]) - 1, a, b))
    hit = tot = 0
    for fam, div in zip(g["truth"], g["divs"]):
        if len(fam) < 3 or div > 0.08:
            continue
        tot += 1
        c0, a0, b0, _m = fam[0]
        hit += any(c == c0 and min(b, b0) - max(a, a0) > 0.7 * (b0 - a0) for c, a, b in iv)
    assert tot >= 3 and hit >= tot - 1, (hit, tot)


def test_mask_genome_intactTE(ctx, tmp_path):
    """N-masking of the full-length copies of a TE library: file output and the resident genome agree"""
    import synth_small
    from hite_amd import util

    g = synth_small.make(11, n_fam=16)
    gp = tmp_path / "genome.cut1.fa"
    gp.write_text("".join(">chr%d$0\n%s\n" % (i + 1, s) for i, s in enumerate(g["contigs"])))
    lib = tmp_path / "prev_TE.fa"
    lib.write_text("".join(">TE_%d\n%s\n" % (i, s) for i, s in enumerate(g["cands"][:6])))
    out = util.mask_genome_intactTE(str(lib), str(gp))
    names, masked = util.read_fasta(out)
    assert names == ["chr%d$0" % (i + 1) for i in range(len(g["contigs"]))]
    # expectation from the twin's copy table: every copy the finder reports has >= 95 % of the library sequence aligned (its own
    # acceptance rule), which is the coverage rule of get_full_length_copies_from_blastn_v1 on the blast6 line written for it
    tab = O.find_copies(g["contigs"], g["cands"][:6])
    exp = [np.frombuffer(s.encode(), dtype=np.uint8).copy() for s in g["contigs"]]
    nmask = 0
    for cand, copies in zip(g["cands"][:6], tab):
        for (c, s1, e1, _m, _a) in copies:
            exp[c][s1 - 1:e1] = ord("N")
            nmask += 1
    assert nmask >= 6
    for n, e in zip(names, exp):
        assert masked[n] == e.tobytes().decode()
    # the resident genome carries the same mask (gather of a masked interval gives N)
    c, s1, e1, _m, _a = tab[0][0]
    wins, _ = util.get_ctx().flank_gather([c], [s1], [e1], [0], flank=0)
    assert set(wins[0].decode()) == {"N"}


def test_ltr_frame(ctx, tmp_path):
    """FiLTR flank-frame vote: golden vectors (reference outputs) and fresh random matrices vs the oracle, batched"""
    from hite_amd import util

    g = load_golden("ltr_frame")
    by = {}
    for c in g:
        by.setdefault((c["flank"], c["window"]), []).append(c)
    for (flank, win), cs in by.items():
        got_l = ctx.ltr_frame([c["left"] for c in cs], flank, win, "left")
        got_r = ctx.ltr_frame([c["right"] for c in cs], flank, win, "right")
        for c, a, b in zip(cs, got_l, got_r):
            assert list(a) == c["left_out"] and list(b) == c["right_out"]
    rng = np.random.default_rng(77)
    mats = []
    for _ in range(200):
        R, flank = int(rng.integers(2, 120)), 60
        cons = casegen.rand_seq(rng, flank)
        h = int(rng.integers(0, flank + 1))
        rows = []
        for _r in range(R):
            s = list(casegen.rand_seq(rng, flank))
            for k in range(h):
                if rng.random() > 0.1:
                    s[k] = cons[k]
            if rng.random() < 0.1:
                s = ["-"] * flank
            rows.append("".join(s))
        mats.append(rows)
    got = ctx.ltr_frame(mats, 60, 20, "right")
    assert [tuple(x) for x in got] == [O.ltr_frame(m, 60, 20, "right") for m in mats]
    got = ctx.ltr_frame([[r[::-1] for r in m] for m in mats], 60, 20, "left")
    assert [tuple(x) for x in got] == [O.ltr_frame([r[::-1] for r in m], 60, 20, "left") for m in mats]
    # file-level mirror
    c = g[5]
    mf = tmp_path / "x.matrix"
    mf.write_text("".join(a + "\t" + b + "\n" for a, b in zip(c["left"], c["right"])))
    assert list(util.judge_left_frame_LTR(str(mf), c["flank"], c["window"])) == c["left_out"]
    assert list(util.judge_right_frame_LTR(str(mf), c["flank"], c["window"])) == c["right_out"]


def test_seed_allvsall_edge_cases(ctx):
    """all-vs-all seeding on degenerate genomes: no repeats, contigs shorter than a k-mer, N blocks, a repeat across a
    segment border, an inverted repeat, a tandem array -- always equal to the twin"""
    rng = np.random.default_rng(99)
    unit = casegen.rand_seq(rng, 900)
    fam = casegen.rand_seq(rng, 1500)
    g1 = [casegen.rand_seq(rng, 30_000)]                                                   # unique sequence
    g2 = ["ACGT", casegen.rand_seq(rng, 14), casegen.rand_seq(rng, 5000)]                    # tiny contigs
    base = casegen.rand_seq(rng, 60_000)
    g3 = [base[:10_000] + fam + base[10_000:29_400] + fam[:700] + "N" * 50 + fam[750:] + base[29_400:45_000] +
          casegen.revcomp(fam) + base[45_000:]]                                             # direct, N-broken and inverted copies
    g4 = [casegen.rand_seq(rng, 3000) + unit * 6 + casegen.rand_seq(rng, 3000), "N" * 2000 + casegen.rand_seq(rng, 4000)]  # tandem array
    # hashes that occur about SEED_MAXOCC = 1000 times (a run of the index that long is not seeded from: the kernel finds a run's ends
    # with bit searches inside a halo of 1024 entries): arrays of 998 .. 1003 and 1100 copies of a 41-base unit, behind / before other runs
    u41, v43 = casegen.rand_seq(rng, 41), casegen.rand_seq(rng, 43)
    g5 = [[casegen.rand_seq(rng, 1500) + u41 * n + casegen.rand_seq(rng, 700)] for n in (998, 1000, 1001, 1003)]
    g5.append([u41 * 999 + casegen.rand_seq(rng, 100), v43 * 1002, casegen.rand_seq(rng, 300) + v43[::-1] * 1100])
    for contigs, seg in ((g1, 10_000), (g2, 1000), (g3, 20_000), (g3, 1_000_000), (g4, 2_500)) + tuple((g, 1_000_000) for g in g5):
        ctx.genome_pack(contigs)
        ctx.release_copy_index()
        got = ctx.seed_allvsall(seg_len=seg)
        exp = O.seed_allvsall(contigs, seg_len=seg)
        for k in ("qseg", "sseg", "qs", "qe", "ss", "se"):
            assert np.array_equal(got[k], exp[k]), (len(contigs), seg, k, len(got[k]), len(exp[k]))
    assert len(got["qseg"]) > 0
    ctx.genome_pack(g3)
    ctx.release_copy_index()
    h = ctx.seed_allvsall(seg_len=1_000_000)
    assert (h["ss"] > h["se"]).any() and (h["ss"] < h["se"]).any()   # both strands reported


def test_nonltr_prep(ctx, tmp_path):
    """non-LTR candidate preparation (search_polyA_TSD): golden vectors (reference outputs) + random tails vs the oracle"""
    from hite_amd import util

    g = load_golden("nonltr_prep")
    got = util.search_polyA_TSD_batch([c["seq"] for c in g], 50, 25)
    for c, r in zip(g, got):
        assert list(r) == [c["found"], c["tsd"], c["non_ltr"]], (c["seq"][:50], r[:2])
    rng = np.random.default_rng(8)
    seqs = []
    for _ in range(400):
        L = int(rng.integers(30, 1200))
        s = list(casegen.rand_seq(rng, L + 100))
        for _k in range(int(rng.integers(0, 4))):
            p = int(rng.integers(0, len(s) - 20))
            unit = ["A", "T", "AC", "TTG", "GATA", "AAAAG"][int(rng.integers(0, 6))]
            rep = (unit * 12)[:int(rng.integers(6, 24))]
            s[p:p + len(rep)] = list(rep)
        if rng.random() < 0.5:
            t = casegen.rand_seq(rng, int(rng.integers(8, 21)))
            a, b = int(rng.integers(20, 60)), len(s) - int(rng.integers(30, 70))
            s[a:a + len(t)] = list(t)
            s[b:b + len(t)] = list(t if rng.random() < 0.6 else casegen.mutate(rng, t, 0.07))
        seqs.append("".join(s)[:L + 100])
    for _ in range(150):   # constructed elements: TSD + body + polyA / tandem tail + TSD (or the reverse-strand form)
        body = casegen.rand_seq(rng, int(rng.integers(90, 900)))
        t = casegen.rand_seq(rng, int(rng.integers(8, 21)))
        t2 = t if rng.random() < 0.6 else casegen.mutate(rng, t, 0.06)
        tail = "A" * int(rng.integers(6, 20)) if rng.random() < 0.7 else "CA" * int(rng.integers(4, 9))
        el = body + tail
        if rng.random() < 0.4:
            el = casegen.revcomp(el)
        seqs.append((casegen.rand_seq(rng, 50) + t)[-50:] + el + (t2 + casegen.rand_seq(rng, 50))[:50])
    got = util.search_polyA_TSD_batch(seqs, 50, 25)
    assert [tuple(x) for x in got] == [O.search_polyA_TSD(s, 50, 25) for s in seqs]
    assert sum(x[0] for x in got) > 20
    # file-level mirror: length classes and names
    fa = tmp_path / "lr.flanked.fa"
    fa.write_text("".join(">r%d\n%s\n" % (i, c["seq"]) for i, c in enumerate(g)))
    sine, line = util.get_candidate_non_LTR(str(fa), 50)
    for name, seq in list(sine.items()) + list(line.items()):
        i = int(name.split("\t")[0][1:])
        assert g[i]["found"] and name.endswith("TSD:" + g[i]["tsd"]) and seq == g[i]["non_ltr"]
    assert len(sine) + len(line) > 10


def _random_hsp_table(rng, nq, ns, n_copies, dup=0.05):
    """blast6-like rows (q, s, qs, qe, ss, se, identity) of TE queries hitting chromosomes, fragmented and shuffled"""
    qlen = [int(rng.integers(150, 4000)) for _ in range(nq)]
    slen = [int(rng.integers(50_000, 3_000_000)) for _ in range(ns)]
    rows = []
    for _ in range(n_copies):
        q, s = int(rng.integers(0, nq)), int(rng.integers(0, ns))
        rev = rng.random() < 0.5
        span = max(40, int(qlen[q] * float(rng.choice([1.0, 1.0, 0.96, 0.7, 0.3]))))
        span = min(span, qlen[q])
        q0 = int(rng.integers(1, qlen[q] - span + 2))
        pos = int(rng.integers(1000, slen[s] - 3 * qlen[q] - 1000)) if rng.random() < 0.9 else 5000 + 37 * q   # piled-up copies
        cuts = sorted(set([0, span] + [int(x) for x in rng.integers(10, max(11, span - 10), size=int(rng.integers(0, 4)))]))
        shift = 0
        for i in range(len(cuts) - 1):
            a, b = cuts[i], cuts[i + 1]
            if i:
                shift += int(rng.choice([0, 0, 2, -2, 150, 199, 200, 201, 400]))
            fs, fe = q0 + a + (int(rng.choice([0, 0, 4, 180, 199, 200])) if i else 0), q0 + b - 1
            if fe < fs:
                continue
            ss_, se_ = (pos + a + shift, pos + b - 1 + shift) if not rev else (pos + span - a + shift, pos + span - b + 1 + shift)
            idt = float(rng.choice([100.0, 99.2, 87.5]))
            rows.append((q, s, fs, fe, ss_, se_, idt))
            if rng.random() < dup:
                rows.append((q, s, fs, fe, ss_, se_, idt if rng.random() < 0.5 else 80.0))
    rows = [rows[i] for i in rng.permutation(len(rows))]
    return rows, qlen, slen


def test_query_copies(ctx, tmp_path):
    """get_query_copies (blastn-route copy clustering): reference goldens through the util mirror, random tables vs the oracle"""
    from hite_amd import util
    for ci, c in enumerate(load_golden("query_copies")):
        recs = {}
        for (q, s, a, b, cc, d, idt) in c["rows"]:
            recs.setdefault("TE_%d" % q, {}).setdefault("chr%d" % s, []).append((a, b, cc, d, idt))
        qc = {"TE_%d" % q: "A" * L for q, L in enumerate(c["qlen"])}
        spath = None
        if c["scov"] > 0:
            spath = str(tmp_path / ("subj_%d.fa" % ci))
            with open(spath, "w") as fh:
                for s, L in enumerate(c["slen"]):
                    fh.write(">chr%d\n%s\n" % (s, "A" * L))
        got = util.get_query_copies(list(recs.items()), qc, spath, c["qcov"], c["scov"])
        exp = {k: [tuple(x) for x in v] for k, v in c["out"].items()}
        assert got == exp, ci
    rng = np.random.default_rng(6828)
    for (nq, ns, ncp, kw) in [(1, 1, 1, {}), (3, 2, 40, {}), (200, 5, 6000, {}), (2000, 20, 60000, {"qcov": 0.8}),
                              (50, 3, 30000, {"qcov": 0.5, "max_copy": 30}), (300, 4, 8000, {"scov": 0.0005, "qthr": 150, "sthr": 250})]:
        rows, qlen, slen = _random_hsp_table(rng, nq, ns, ncp)
        cols = list(zip(*rows))
        exp = O.query_copies(rows, qlen, slen, kw.get("qcov", 0.95), kw.get("scov", 0.0), kw.get("qthr", 200), kw.get("sthr", 200),
                             kw.get("max_copy", 100))
        got = ctx.query_copies(cols[0], cols[1], cols[2], cols[3], cols[4], cols[5], cols[6], qlen, slen, **kw)
        assert got == exp, (nq, ns, ncp)
        assert ncp < 100 or sum(len(x) for x in got) > 0
    # no identity column, empty table, bad input
    rows, qlen, slen = _random_hsp_table(rng, 20, 2, 500, dup=0.0)
    cols = list(zip(*rows))
    assert ctx.query_copies(cols[0], cols[1], cols[2], cols[3], cols[4], cols[5], None, qlen, slen) == O.query_copies(rows, qlen, slen, 0.95)
    assert ctx.query_copies([], [], [], [], [], [], [], [100, 200], [1000]) == [[], []]
    with pytest.raises(RuntimeError):
        ctx.query_copies([0], [0], [10], [50], [-1, ], [50], [99.0], [100], [1000])    # negative coordinate
    with pytest.raises(RuntimeError):
        ctx.query_copies([3], [0], [1], [50], [1, ], [50], [99.0], [100], [1000])      # query id out of range


def test_get_copies_v1_file(ctx, tmp_path):
    """get_copies_v1: blast6 file + query fasta -> copies; self hits skipped; equals the oracle on the parsed table"""
    from hite_amd import util

    rng = np.random.default_rng(7032)
    rows, qlen, slen = _random_hsp_table(rng, 30, 3, 900)
    bl = tmp_path / "hits.out"
    with open(bl, "w") as fh:
        fh.write("TE_0\tTE_0\t100.0\t50\t0\t0\t1\t50\t1\t50\t0.0\t90\n")         # self hit
        for (q, s, a, b, c, d, idt) in rows:
            fh.write("TE_%d\tchr%d\t%.3f\t%d\t0\t0\t%d\t%d\t%d\t%d\t1e-50\t500\n" % (q, s, idt, b - a + 1, a, b, c, d))
    qf = tmp_path / "q.fa"
    with open(qf, "w") as fh:
        for q, L in enumerate(qlen):
            fh.write(">TE_%d\n%s\n" % (q, "ACGT" * (L // 4) + "A" * (L % 4)))
    got = util.get_copies_v1(str(bl), str(qf), "", query_coverage=0.9)
    order = {}
    dense = []
    for r in rows:
        dense.append((order.setdefault(r[0], len(order)),) + tuple(r[1:6]) + (float("%.3f" % r[6]),))
    ql = [0] * len(order)
    for orig, q in order.items():
        ql[q] = qlen[orig]
    exp = O.query_copies(dense, ql, slen, 0.9)
    assert set(got) == {"TE_%d" % o for o in order}
    for orig, q in order.items():
        assert got["TE_%d" % orig] == [("chr%d" % c[0],) + c[1:] for c in exp[q]]


def _random_lib_table(rng, nseq, nhits):
    lens = [int(rng.integers(120, 6000)) for _ in range(nseq)]
    rows = []
    for _ in range(nhits):
        q, s = int(rng.integers(0, nseq)), int(rng.integers(0, nseq))
        rev = rng.random() < 0.4
        span = max(25, int(min(lens[q], lens[s]) * float(rng.choice([1.0, 0.97, 0.9, 0.5, 0.1]))))
        span = min(span, lens[q], lens[s])
        q0, s0 = int(rng.integers(1, lens[q] - span + 2)), int(rng.integers(1, lens[s] - span + 2))
        cuts = sorted(set([0, span] + [int(x) for x in rng.integers(5, max(6, span - 5), size=int(rng.integers(0, 5)))]))
        for i in range(len(cuts) - 1):
            a, b = cuts[i], cuts[i + 1]
            jq = int(rng.choice([0, 0, 3, 20, 60, 200])) if i else 0
            js = int(rng.choice([0, 0, -2, 4, 30, 90, 300])) if i else 0
            fs, fe = q0 + a + jq, q0 + b - 1
            ss_, se_ = (s0 + a + js, s0 + b - 1) if not rev else (s0 + span - a - 1 - js, s0 + span - b)
            if fe < fs or ss_ < 1 or se_ < 1:
                continue
            rows.append((q, s, fs, fe, ss_, se_))
            if rng.random() < 0.05:
                rows.append((q, s, fs, fe, ss_, se_))
        if rng.random() < 0.2:
            rows.append((q, q, 1, lens[q], 1, lens[q]))
    return [rows[i] for i in rng.permutation(len(rows))], lens


def test_lib_dedup(ctx, tmp_path):
    """panHiTE library de-duplication pieces (f-3): chain records / clusters / consensus vs reference goldens and the oracle"""
    from hite_amd import util

    g = load_golden("lib_dedup")
    for ci, c in enumerate(g["chain"]):
        cols = list(zip(*c["rows"])) if c["rows"] else [[]] * 6
        recs = ctx.lib_chain(cols[0], cols[1], cols[2], cols[3], cols[4], cols[5], c["lens"], c["thr"], c["chunk_size"])
        assert recs == c["recs"], ci
        assert [sorted(x) for x in ctx.lib_cluster(recs, c["lens"], c["thr"])] == c["clusters"]
    # file-level mirrors on one golden case
    c = g["chain"][3]
    names = ["seq_%d" % i for i in range(len(c["lens"]))]
    fa, bl = tmp_path / "lib.fa", tmp_path / "lib.out"
    with open(fa, "w") as fh:
        for nme, L in zip(names, c["lens"]):
            fh.write(">%s\n%s\n" % (nme, "A" * L))
    with open(bl, "w") as fh:
        for (q, s, a, b, cc, d) in c["rows"]:
            fh.write("%s\t%s\t95.0\t%d\t0\t0\t%d\t%d\t%d\t%d\t1e-20\t200\n" % (names[q], names[s], b - a + 1, a, b, cc, d))
    chunks = util.lib_longest_repeats(str(bl), str(fa), c["thr"], chunk_size=c["chunk_size"])
    flat = [[ch, int(r[0][4:]), r[1], r[2], int(r[3][4:]), r[4], r[5]] for ch, d in enumerate(chunks) for lst in d.values() for r in lst]
    assert flat == c["recs"]
    cl = util.cluster_sequences_from_chunks(chunks, util.read_fasta(str(fa))[1], c["thr"])
    assert [sorted(int(x[4:]) for x in k) for k in cl] == c["clusters"]
    # random tables vs the oracle, chunked and not
    rng = np.random.default_rng(12202)
    for (nseq, nhits, cs) in [(1, 3, 0), (40, 800, 0), (300, 20000, 0), (300, 20000, 997), (2000, 60000, 5000)]:
        rows, lens = _random_lib_table(rng, nseq, nhits)
        thr = float(rng.choice([0.95, 0.8]))
        cols = list(zip(*rows))
        recs = ctx.lib_chain(cols[0], cols[1], cols[2], cols[3], cols[4], cols[5], lens, thr, cs)
        assert recs == O.lib_chain(rows, lens, thr, cs), (nseq, nhits, cs)
        assert ctx.lib_cluster(recs, lens, thr) == O.lib_cluster(recs, lens, thr)
    assert ctx.lib_chain([], [], [], [], [], [], [100], 0.95) == []
    with pytest.raises(RuntimeError):
        ctx.lib_chain([0], [5], [1], [10], [1], [10], [100], 0.95)       # subject id out of range
    # consensus: goldens through the file mirror, random batch vs the oracle
    for ci, c in enumerate(g["cons"]):
        af = tmp_path / ("c%d.maf.fa" % ci)
        with open(af, "w") as fh:
            for r, row in enumerate(c["rows"]):
                fh.write(">r%d\n%s\n" % (r, row))
        assert util.cons_from_mafft_v1(str(af)) == c["cons"], ci
    als = []
    for _ in range(60):
        R, L = int(rng.integers(1, 40)), int(rng.integers(1, 1500))
        base = casegen.rand_seq(rng, L)
        al = []
        for _r in range(R):
            row = np.frombuffer(base.encode(), dtype=np.uint8).copy()
            m = rng.random(L)
            row[m < 0.3] = ord("-")
            sub = (m >= 0.3) & (m < 0.4)
            row[sub] = np.frombuffer(b"ACGTN", dtype=np.uint8)[rng.integers(0, 5, size=int(sub.sum()))]
            al.append(row.tobytes().decode())
        als.append(al)
    got = ctx.msa_consensus(als)
    for al, gc in zip(als, got):
        assert gc == O.cons_majority(al)
    assert ctx.msa_consensus([]) == []


def test_ltr_both_ends(ctx, tmp_path):
    """FiLTR get_both_ends_frame: reference goldens through the file mirror (batch call for the rest) + frames feed the vote"""
    from hite_amd import util

    g = load_golden("ltr_both_ends")
    als = [[r.upper() for r in c["rows"]] for c in g]
    flanks = sorted({c["flank"] for c in g})
    nfound = 0
    for F in flanks:
        idx = [i for i, c in enumerate(g) if c["flank"] == F]
        got = ctx.ltr_both_ends([als[i] for i in idx], [g[i]["cur"] for i in idx], F)
        for i, res in zip(idx, got):
            c = g[i]
            exp = O.ltr_both_ends(als[i], c["cur"], F)
            if c["frames"] is None:
                assert res is None and exp is None
                continue
            assert res is not None
            assert [list(x) for x in res[0]] == c["frames"] and res[1] == c["full"], i
            assert (res[2], res[3]) == (exp[2], exp[3])
            nfound += 1
    assert nfound > 40
    # file-level mirror and hand-over to the frame vote
    c = next(c for c in g if c["frames"] is not None and len(c["rows"]) >= 4)
    af = tmp_path / "q.maf.fa"
    af.write_text("".join(">copy%d\n%s\n" % (r, row) for r, row in enumerate(c["rows"])))
    (tmp_path / "o").mkdir(); (tmp_path / "f").mkdir()
    m1, m2 = util.get_both_ends_frame("q", c["cur"], str(af), str(tmp_path / "o"), str(tmp_path / "f"), c["flank"], 0)
    assert [ln.rstrip("\n").split("\t") for ln in open(m1)] == c["frames"]
    assert [ln.rstrip("\n") for ln in open(m2)] == c["full"]
    lt = util.judge_left_frame_LTR(m1, c["flank"])
    assert isinstance(lt[0], (bool, np.bool_, int))


def test_wide_radix_sort_on_small_inputs(tmp_path):
    """the 10-bit LDS-staged scatter (normally used from 4 M elements on) forced onto the small parity cases: FMEA, copy
    clustering, library chaining and the copy finder must give the same answers (ragged last tiles, empty digits)"""
    import os
    import subprocess
    import sys as _sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HITE_SORT_WIDE_MIN="2")
    rc = subprocess.run([_sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_parity.py"), "-x", "-q", "-m", "gpu", "-k",
                         "fmea or query_copies or lib_dedup or find_copies or seed_allvsall"], env=env, capture_output=True, text=True, cwd=root)
    assert rc.returncode == 0, rc.stdout[-3000:] + rc.stderr[-2000:]
    assert " passed" in rc.stdout
    # the copy finder's hits travel as packed 8-byte records when their fields fit 64 bits (always, at test sizes): the
    # 12-byte key + value form, with both radix-sort forms, must give the same tables
    for extra in ({"HITE_HITS_WIDE": "1"}, {"HITE_HITS_WIDE": "1", "HITE_SORT_WIDE_MIN": "2"}):
        rc = subprocess.run([_sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_parity.py"), "-x", "-q", "-m", "gpu", "-k",
                             "find_copies or hot_path or flank_region_align"], env=dict(os.environ, **extra), capture_output=True, text=True, cwd=root)
        assert rc.returncode == 0, rc.stdout[-3000:] + rc.stderr[-2000:]
        assert " passed" in rc.stdout


def test_seed_anchor_record_forms(tmp_path):
    """stage 3.1's anchors travel as packed 8-byte records (strand | diagonal | query position) when the genome has at most 2^30
    bases -- always, at test sizes; the 12-byte key + value form of larger genomes (HITE_SEED_PACK=0), with both radix-sort forms,
    must give the same HSP tables, shares and intervals"""
    import os
    import subprocess
    import sys as _sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # HITE_SEED_PLACE=1: the seeds' records reach position order through one radix pass + a scatter inside L2-sized windows (the form of
    # genomes with >= 4 M minimizers) also at test sizes, with both radix-sort forms and with the counts scattered beside the records
    for extra in ({"HITE_SEED_PACK": "0"}, {"HITE_SEED_PACK": "0", "HITE_SORT_WIDE_MIN": "2"}, {"HITE_SEED_PLACE": "1"},
                  {"HITE_SEED_PLACE": "1", "HITE_SORT_WIDE_MIN": "2", "HITE_SEED_PLACE_CNT": "1", "HITE_SEED_PLACE_LDS": "0"}):
        rc = subprocess.run([_sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_parity.py"), "-x", "-q", "-m", "gpu", "-k",
                             "seed_allvsall or seed_shard or coarse_boundary"], env=dict(os.environ, **extra), capture_output=True, text=True, cwd=root)
        assert rc.returncode == 0, rc.stdout[-3000:] + rc.stderr[-2000:]
        assert " passed" in rc.stdout


def test_fmea_stress_hash(ctx):
    """30 k-line HSP table: the GPU's ordered interval names hash to the reference's sha256 (fixture holds parameters + hash)"""
    import hashlib

    g = load_golden("fmea_stress")
    rows = casegen.make_hsp_table(**{k: (tuple(v) if isinstance(v, list) else v) for k, v in g["params"].items()})
    got, _h = _fmea_gpu(ctx, rows, g["skip_gap"], g["max_len"])
    assert len(rows) == g["lines"] and len(got) == g["intervals"]
    assert hashlib.sha256("\n".join(got).encode()).hexdigest() == g["sha256"]


def test_coarse_boundary_honours_prev_TE(ctx, tmp_path):
    """argv as main.py builds it (main.py:520-532), --prev_TE with a non-empty library: the chunk is N-masked with the
    full-length copies of those TEs before seeding (mask_genome_intactTE, Util.py:6389), so the families already in prev_TE
    do not come out again, the others still do"""
    import os
    import subprocess
    import sys as _sys

    import synth_small
    from hite_amd import util

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    g = synth_small.make(43, n_fam=10, n_chr=2, chr_len=300_000)
    ref = tmp_path / "genome.fa"
    ref.write_text("".join(">chr%d\n%s\n" % (i + 1, s) for i, s in enumerate(g["contigs"])))
    cut = tmp_path / "genome.cut0.fa"
    with open(cut, "w") as f:
        for i, s in enumerate(g["contigs"]):
            for o in range(0, len(s), 100_000):
                f.write(">chr%d$%d\n%s\n" % (i + 1, o, s[o:o + 100_000]))
    multi = [k for k, (fam, div) in enumerate(zip(g["truth"], g["divs"])) if len(fam) >= 3 and div <= 0.08]
    assert len(multi) >= 4
    known = multi[:len(multi) // 2]
    prev = tmp_path / "prev_TE.fa"
    prev.write_text("".join(">known_%d\n%s\n" % (k, g["cands"][k]) for k in known))

    def run(out, prev_path):
        argv = [_sys.executable, root + "/hite_amd/scripts/coarse_boundary.py", "-g", str(cut), "--tmp_output_dir", str(out),
                "--prev_TE", str(prev_path), "--fixed_extend_base_threshold", "1000", "--max_repeat_len", "30000", "--thread", "2",
                "--flanking_len", "50", "--tandem_region_cutoff", "0.5", "--ref_index", "0", "-r", str(ref), "--recover", "0",
                "--debug", "0", "-w", str(tmp_path)]
        rc = subprocess.run(argv, capture_output=True, text=True)
        assert rc.returncode == 0, rc.stderr[-2000:]
        names, _ = util.read_fasta(str(out / "longest_repeats_0.fa"))
        iv = []
        for n in names:
            c, pos = n.split(":")
            a, b = map(int, pos.split("-"))
            iv.append((int(c[3:]) - 1, a, b))
        return iv

    def recovered(iv, k):
        c0, a0, b0, _m = g["truth"][k][0]
        return any(c == c0 and min(b, b0) - max(a, a0) > 0.7 * (b0 - a0) for c, a, b in iv)

    empty = tmp_path / "none.fa"
    empty.write_text("")
    base = run(tmp_path / "out_a", empty)
    masked = run(tmp_path / "out_b", prev)
    assert sum(recovered(base, k) for k in multi) >= len(multi) - 1
    assert sum(recovered(masked, k) for k in known) == 0                       # already in prev_TE: masked, not re-discovered
    assert sum(recovered(masked, k) for k in multi if k not in known) >= len(multi) - len(known) - 1


def test_reference_signatures_and_prev_TE_lock(ctx, tmp_path):
    """flank_region_align_v5 called with exactly the reference's positional arguments (Util.py:8032) uses the built-in copy
    finder; determine_repeat_boundary_v5 takes the reference's ten arguments (Util.py:4637); the stage tail renames through
    rename_fasta / lib_add_prefix and appends to prev_TE through update_prev_TE"""
    import inspect
    import os
    import sys as _sys

    import synth_small
    from hite_amd import util

    assert list(inspect.signature(util.determine_repeat_boundary_v5).parameters)[:10] == [
        "repeats_path", "longest_repeats_path", "prev_TE", "fixed_extend_base_threshold", "max_single_repeat_len", "tmp_output_dir",
        "threads", "ref_index", "reference", "debug"]
    assert list(inspect.signature(util.flank_region_align_v5).parameters)[:16] == [
        "candidate_sequence_path", "real_TEs", "flanking_len", "reference", "split_ref_dir", "TE_type", "tmp_output_dir", "threads",
        "ref_index", "log", "subset_script_path", "plant", "debug", "iter_num", "all_low_copy", "result_type"]
    g = synth_small.make(5, n_fam=10)
    gref = tmp_path / "genome.fa"
    gref.write_text("".join(">c%d\n%s\n" % (i, s) for i, s in enumerate(g["contigs"])))
    cand = tmp_path / "cand.fa"
    cand.write_text("".join(">q%d\n%s\n" % (i, s) for i, s in enumerate(g["cands"])))
    real, low = tmp_path / "real.fa", tmp_path / "low.fa"
    t, l = util.flank_region_align_v5(str(cand), str(real), 50, str(gref), None, "tir", str(tmp_path), 1, 0, None, "", 1, 0, 0, str(low))
    assert len(t) + len(l) >= 3 and set(util.read_fasta(str(real))[0]) == set(t)
    # the copy finder follows the genome: a second reference in the same process gives that genome's copies
    g2 = synth_small.make(6, n_fam=6)
    gref2 = tmp_path / "genome2.fa"
    gref2.write_text("".join(">d%d\n%s\n" % (i, s) for i, s in enumerate(g2["contigs"])))
    cand2 = tmp_path / "cand2.fa"
    cand2.write_text("".join(">p%d\n%s\n" % (i, s) for i, s in enumerate(g2["cands"])))
    cp2 = util.get_full_length_copies_minimap2(str(cand2), str(gref2))
    exp2 = O.find_copies(g2["contigs"], g2["cands"])
    for i, e in enumerate(exp2):
        got = cp2.get("p%d" % i, [])
        assert [(int(c[0][1:]), c[1], c[2], c[4] == "-") for c in got] == [(x[0], x[1], x[2], bool(x[3])) for x in e]
    cp1 = util.get_full_length_copies_minimap2(str(cand), str(gref))
    exp1 = O.find_copies(g["contigs"], g["cands"])
    assert sum(len(v) for v in cp1.values()) == sum(len(e) for e in exp1)
    # stage tail
    _sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hite_amd", "scripts"))
    import _stage

    prev = tmp_path / "prev_TE.fa"
    prev.write_text(">old_0\nACGTACGTAC\n")
    res = tmp_path / "res.fa"
    res.write_text(">a#DNA/hAT\n" + "ACGT" * 30 + "\n>b\n" + "AC" * 20 + "\n>c\n" + "TTGA" * 25 + "\n")
    kept = _stage.finish(str(res), str(tmp_path / "confident_tir_0.fa"), "TIR", "0", str(gref), 80, str(prev))
    assert list(kept) == ["genome-TIR_0_0#DNA/hAT", "genome-TIR_0_1"]
    pn, _pc = util.read_fasta(str(prev))
    assert pn == ["old_0", "genome-TIR_0_0#DNA/hAT", "genome-TIR_0_1"] and os.path.exists(str(prev) + ".lock")


def test_pan_remove_redundancy_script(ctx, tmp_path):
    """config C5 in miniature: the TE libraries of several genomes, concatenated, come out as one non-redundant library:
    one consensus per family (copies 1-4 % apart collapse), unrelated sequences pass unchanged, LTR internal sequences
    ('-int#') are handled apart with their own coverage threshold"""
    import os
    import subprocess
    import sys as _sys

    from hite_amd import util

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rng = np.random.default_rng(515)
    recs, fams = [], []
    for f in range(6):
        cons = casegen.rand_seq(rng, int(rng.integers(400, 1500)))
        fams.append(cons)
        internal = f >= 4
        for g in range(int(rng.integers(3, 7))):     # one copy per "genome"
            s = casegen.mutate(rng, cons, float(rng.uniform(0.01, 0.04)))
            recs.append(("G%d-fam%d%s#%s" % (g, f, "-int" if internal else "", "LTR/Gypsy" if internal else "DNA/hAT"), s))
    for k in range(5):
        recs.append(("single%d#Unknown" % k, casegen.rand_seq(rng, int(rng.integers(300, 900)))))
    order = rng.permutation(len(recs))
    merged = tmp_path / "merged.fa"
    merged.write_text("".join(">%s\n%s\n" % recs[i] for i in order))
    out = tmp_path / "out"
    rc = subprocess.run([_sys.executable, root + "/hite_amd/scripts/pan_remove_redundancy.py", "--merge_te_file", str(merged), "--threads", "2",
                         "--output_dir", str(out), "-w", str(tmp_path)], capture_output=True, text=True)
    assert rc.returncode == 0, rc.stderr[-2000:]
    names, seqs = util.read_fasta(str(out / "panTE.fa"))
    assert sum(n.startswith("single") for n in names) == 5
    for f, cons in enumerate(fams):
        mine = [n for n in names if "-fam%d" % f in n]
        assert len(mine) == 1, (f, mine)          # the family collapsed into one record ...
        got = seqs[mine[0]]
        assert abs(len(got) - len(cons)) <= 0.02 * len(cons)
        d = O.nw_distance(got, cons)
        assert d <= 0.03 * len(cons) * 3, (f, d, len(cons))   # ... whose consensus is closer to the family than its members
    assert len(names) == 11


def test_generate_cons_v1_golden_on_gpu(ctx, tmp_path):
    """util.generate_cons_v1 (alignments and consensus on the GPU) against the reference's own generate_cons_v1 run with a
    fabricated Ninja file (tests/golden/cons_v1.json.gz), and the build's Ninja stand-in on the same clusters"""
    from hite_amd import util

    util._CTX = ctx
    cases = load_golden("cons_v1")
    for ci, c in enumerate(cases):
        fa = tmp_path / ("cl%d.fa" % ci)
        fa.write_text("".join(">%s\n%s\n" % (n, s) for n, s in zip(c["names"], c["seqs"])))
        ninja = {int(k): v for k, v in c["ninja"].items()}
        got = util.generate_cons_v1(0, str(fa), str(tmp_path), 1, ninja_clusters=ninja)
        assert got == c["expected"], ci
        # the stand-in (leader clustering at 20 % on the cluster's alignment) finds the planted families: the names tell them
        own = util.generate_cons_v1(0, str(fa), str(tmp_path), 1)
        fams = {n.split("_")[0].split("-")[1] for n in c["names"]}
        assert {n.split("_")[0].split("-")[1] for n in own} == fams and len(own) <= len(c["names"])
    assert util.read_Ninja_clusters.__doc__


def test_deredundant_limits(ctx, tmp_path, monkeypatch):
    """libraries beyond one all-vs-all call are searched in blocks (same clusters as in one call), members longer
    than the aligner's windows pass unclustered instead of failing the whole library, lower-case input is compared
    case-insensitively, members the aligner drops pass unchanged"""
    from hite_amd import util

    util._CTX = ctx
    rng = np.random.default_rng(99)
    recs = []
    fams = []
    for f in range(5):
        cons = casegen.rand_seq(rng, int(rng.integers(500, 1200)))
        fams.append(cons)
        for g in range(4):
            sq = casegen.mutate(rng, cons, 0.02)
            recs.append(("G%d-fam%d#DNA/hAT" % (g, f), sq.lower() if (f + g) % 3 == 0 else sq))
    big = casegen.rand_seq(rng, 40_000)                              # an LTR internal sequence beyond 32 767 bases, twice
    recs.append(("G0-long-int#LTR/Gypsy", big))
    recs.append(("G1-long-int#LTR/Gypsy", casegen.mutate(rng, big, 0.01)))
    recs.append(("single#Unknown", casegen.rand_seq(rng, 700)))
    lib = tmp_path / "lib.fa"
    lib.write_text("".join(">%s\n%s\n" % r for r in recs))
    out1 = util.deredundant_for_LTR_v5(str(lib), str(tmp_path), 1, "x", 0.95, 0)
    n1, s1 = util.read_fasta(out1)
    assert sum("-long-int" in n for n in n1) == 2 and "single#Unknown" in n1            # passed unchanged
    assert s1["G0-long-int#LTR/Gypsy"] == big
    for f in range(5):
        mine = [n for n in n1 if "-fam%d#" % f in n]
        assert len(mine) == 1, (f, mine)
        assert O.nw_distance(s1[mine[0]].upper(), fams[f]) <= 0.03 * len(fams[f]) * 3
    # the same library in blocks of 6 sequences (pairs of blocks packed together)
    monkeypatch.setattr(util, "SEED_MAX_SEGMENTS", 12)
    lib2 = tmp_path / "lib2.fa"
    lib2.write_text(lib.read_text())
    out2 = util.deredundant_for_LTR_v5(str(lib2), str(tmp_path), 1, "y", 0.95, 0)
    n2, s2 = util.read_fasta(out2)
    assert sorted(n2) == sorted(n1) and all(s2[n] == s1[n] for n in n1)


@pytest.mark.parametrize("te_type,script,outname,label", [
    ("helitron", "judge_Helitron_transposons.py", "confident_helitron_0.fa", "Helitron_0_"),
    ("non_ltr", "judge_Non_LTR_transposons.py", "confident_non_ltr_0.fa", "Non_LTR_0_")])
def test_typed_stage_scripts_find_the_planted_families(ctx, tmp_path, te_type, script, outname, label):
    """the Helitron / non-LTR drop-in scripts on families shaped for them (judge_Helitron_transposons.py:86-125,
    judge_Non_LTR_transposons.py:48-92): every sequence of the output FASTA is one planted element (within 3 % of one genomic
    copy, strand free), at least four families come out, none twice, names follow rename_fasta + lib_add_prefix"""
    import os
    import subprocess
    import sys as _sys

    import synth_small
    from hite_amd import util

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    g = synth_small.make(12, n_fam=16, te_type=te_type)
    ref = tmp_path / "genome.fa"
    ref.write_text("".join(">chr%d\n%s\n" % (i + 1, s) for i, s in enumerate(g["contigs"])))
    flanked = tmp_path / "cand.flanked.fa"
    recs = []
    for cand, cps in zip(g["cands"], g["copies"]):
        c, a, b, _m = cps[0]
        recs.append(">chr%d:%d-%d\n%s\n" % (c + 1, a - 50, b + 50, g["contigs"][c][a - 1 - 50:b + 50]))
    flanked.write_text("".join(recs))
    candf = tmp_path / "cand.fa"
    candf.write_text("".join(">c%d\n%s\n" % (i, s) for i, s in enumerate(g["cands"])))
    out = tmp_path / "out"
    rc = subprocess.run([_sys.executable, root + "/hite_amd/scripts/" + script, "--seqs", str(flanked), "-t", "1", "--tmp_output_dir", str(out),
                         "--ref_index", "0", "--flanking_len", "50", "--recover", "0", "-r", str(ref), "--min_TE_len", "80",
                         "--candidates", str(candf)], capture_output=True, text=True)
    assert rc.returncode == 0, rc.stderr[-2000:]
    names, seqs = util.read_fasta(str(out / outname))
    assert len(names) >= 4 and all(n.startswith("genome-" + label) for n in names), names
    hit_fams = []
    for n in names:
        sq = seqs[n]
        best = None
        for f, fam in enumerate(g["truth"]):
            c, a, b, mn = fam[0]
            el = g["contigs"][c][a - 1:b]
            if abs(len(el) - len(sq)) > 0.1 * len(el):
                continue
            d = min(O.nw_distance(sq, el), O.nw_distance(util.getReverseSequence(sq), el))
            if best is None or d < best[0]:
                best = (d, f, len(el))
        assert best is not None and best[0] <= 0.03 * 3 * best[2], (n, len(sq), best)
        hit_fams.append(best[1])
    assert len(set(hit_fams)) == len(hit_fams) and len(hit_fams) >= 4


def test_remove_redundant_sequences(ctx, tmp_path):
    """the stand-in for `cd-hit-est -aS 0.95 -aL 0.95` (used when cd-hit-est is not installed): near-identical sequences of about
    the same length collapse to the longest, a fragment of 70 % stays (-aL), unrelated sequences stay, the output is ordered
    longest first"""
    from hite_amd import util

    util._CTX = ctx
    rng = np.random.default_rng(808)
    recs = []
    fams = [casegen.rand_seq(rng, L) for L in (900, 1400, 600)]
    for f, cons in enumerate(fams):
        for k in range(3):
            sq = casegen.mutate(rng, cons, 0.02)
            recs.append(("f%d_%d" % (f, k), sq[: len(sq) - 3 * k]))       # lengths differ a little: the first is the longest
    recs.append(("frag_of_f1", fams[1][:980]))
    recs.append(("other_a", casegen.rand_seq(rng, 800)))
    recs.append(("other_b", casegen.rand_seq(rng, 300)))
    order = rng.permutation(len(recs))
    inp, outp = tmp_path / "in.fa", tmp_path / "out.fa"
    inp.write_text("".join(">%s\n%s\n" % recs[i] for i in order))
    util.remove_redundant_sequences(str(inp), str(outp))
    names, seqs = util.read_fasta(str(outp))
    assert sorted(names) == sorted(["f0_0", "f1_0", "f2_0", "frag_of_f1", "other_a", "other_b"])
    lens = [len(seqs[n]) for n in names]
    assert lens == sorted(lens, reverse=True)


def test_row_selection_ties_follow_the_window_names(ctx):
    """more than 100 copies with windows over 1000 bp: their first500+last500 forms are all 1000 long, so ready_for_MSA.sh's
    choice of 100 is decided by the NAME order alone (pinned by tests/golden/ready_for_msa.json.gz); contig names whose byte
    order differs from their packing order"""
    import oracle_pipeline as OP
    import synth_small

    names = ["chr10", "chr2", "chr1_random"]            # byte order of "<name>:": chr10 < chr1_random < chr2  -> ranks 0, 2, 1
    n_checked = n_big = 0
    for seed in (31, 32, 33):
        g = synth_small.make(seed, n_fam=10, te_type="tir")
        ctx.genome_pack(g["contigs"])
        ctx.set_contig_order(names)
        got, _stats = ctx.flank_region_align("tir", g["cands"], g["copies"], plant=1)
        for cand, copies, res in zip(g["cands"], g["copies"], got):
            exp = OP.fine_stage_candidate("tir", cand, copies, g["contigs"], plant=1, contig_names=names)
            assert [res[0], res[1], res[2], res[3]] == exp, (seed, res, exp)
            n_checked += 1
            n_big += len(copies) > 100
    ctx.set_contig_order(None)
    assert n_checked >= 15 and n_big >= 3


def test_chain_variants_golden_on_gpu(ctx, tmp_path):
    """FMEA (Util.py:10452), get_full_length_copies_from_blastn_v1 (:5907), generate_full_length_out_v1 (:6288) and
    multiple_alignment_blast_and_get_copies_v1 (:7179) with the chaining on the GPU (hite_chain_all / hite_query_copies)
    against what the reference computed (tests/golden/chain_variants.json.gz), then hite_chain_all against its twin on random
    tables large enough for every kernel path (many queries and subjects, both strands, duplicates, per-query gaps)"""
    import chain_variant_cases
    from hite_amd import util

    n_chains, n_copies = chain_variant_cases.check_all(util, ctx, str(tmp_path))
    assert n_chains > 100 and n_copies > 50
    rng = np.random.default_rng(6288)
    for trial in range(6):
        nq, ns = int(rng.integers(1, 40)), int(rng.integers(1, 12))
        n = int(rng.integers(50, 6000))
        qid = rng.integers(0, nq, n).astype(np.int32)
        sid = rng.integers(0, ns, n).astype(np.int32)
        qs = rng.integers(1, 3000, n).astype(np.int64)
        qe = qs + rng.integers(1, 400, n)
        ss = rng.integers(1, 40000 if trial % 2 else 4000, n).astype(np.int64)
        ln = rng.integers(1, 400, n)
        rev = rng.random(n) < 0.45
        se = np.where(rev, ss - ln, ss + ln)
        keep = se >= 1
        qid, sid, qs, qe, ss, se = (x[keep] for x in (qid, sid, qs, qe, ss, se))
        # duplicates
        dup = rng.integers(0, len(qid), len(qid) // 10)
        qid, sid, qs, qe, ss, se = (np.concatenate([x, x[dup]]) for x in (qid, sid, qs, qe, ss, se))
        gaps = rng.integers(0, 3000, nq).astype(np.int64) if trial % 3 else np.full(nq, 200, dtype=np.int64)
        got = ctx.chain_all(qid, sid, qs, qe, ss, se, nq, ns, gaps)
        exp = O.chain_all(qid, sid, qs, qe, ss, se, nq, ns, gaps)
        assert got == exp, trial
        assert sum(len(x) for x in got) > 10
    assert ctx.chain_all([], [], [], [], [], [], 3, 2, [5, 5, 5]) == [[], [], []]


def test_seed_shard_partitions_the_hsp_table(ctx):
    """hite_seed_shard (hite_amd/dist.py coarse_stage_sharded): the shares of three ranks, computed one after the
    other on the one GPU, are each the twin's share, and together -- concatenated in rank order, stably sorted by (query
    segment, subject segment) -- the unsharded HSP table record for record; the sharded stage as one rank runs it gives the
    intervals of the stage computed directly"""
    import synth_small
    from hite_amd import dist as hd
    from oracle_ctx import OracleCtx

    g = synth_small.make(31, n_fam=14, n_chr=3, chr_len=150_000)
    ctx.genome_pack(g["contigs"])
    ctx.release_copy_index()
    keys = ("qseg", "sseg", "qs", "qe", "ss", "se")
    whole = ctx.seed_allvsall(seg_len=50_000)
    tw = OracleCtx()
    tw.genome_pack(g["contigs"])
    parts = []
    try:
        for r in range(3):
            ctx.seed_shard(r, 3)
            tw.seed_shard(r, 3)
            part = ctx.seed_allvsall(seg_len=50_000)
            twin = tw.seed_allvsall(seg_len=50_000)
            for k in keys:
                assert np.array_equal(part[k], twin[k]), (r, k)
            assert len(part["qseg"]) > 0
            parts.append(np.stack([np.asarray(part[k], dtype=np.int64) for k in keys], axis=1))
    finally:
        ctx.seed_shard(0, 0)
    rows = np.concatenate(parts)
    rows = rows[np.argsort(rows[:, 0] * 100000 + rows[:, 1], kind="stable")]
    for i, k in enumerate(keys):
        assert np.array_equal(rows[:, i], np.asarray(whole[k], dtype=np.int64)), k
    oc, os_, oe = hd.coarse_stage_sharded(ctx, 50_000, 2000, 30000, base_threshold=100_000)
    tc, ts, te = hd.coarse_stage_sharded(tw, 50_000, 2000, 30000, base_threshold=100_000)
    assert (oc.tolist(), os_.tolist(), oe.tolist()) == (tc.tolist(), ts.tolist(), te.tolist()) and len(oc) >= 20
    # a search whose anchors exceed what one call sorts (config C5's merge of eight libraries: 5 x 10^9) runs in shares by itself
    # (Context.seed_allvsall): the same table, record for record
    anchors = whole["stats"][1]
    auto = ctx.seed_allvsall(seg_len=50_000, max_anchors=anchors // 5)
    assert auto.get("shares", 1) >= 4 and auto["stats"][1] == anchors
    for k in keys:
        assert np.array_equal(auto[k], whole[k]), k


def test_sharded_context_keeps_its_shard_through_the_auto_split(ctx):
    """a context that is rank r of 3 (what hite_amd.dist.coarse_stage_sharded sets before it seeds) and whose share has more anchors
    than one call sorts: Context.seed_allvsall splits THAT share (sub-share s of S = rank r S + s of world 3 S) -- the table is the
    rank's share and the twin's, record for record, the anchors are the share's, the context is rank r of 3 afterwards, and the
    three tables together are the unsharded one.  (Before, the split returned the whole table and left the context unsharded.)"""
    import synth_small
    from oracle_ctx import OracleCtx

    g = synth_small.make(31, n_fam=14, n_chr=3, chr_len=150_000)
    ctx.genome_pack(g["contigs"])
    ctx.release_copy_index()
    keys = ("qseg", "sseg", "qs", "qe", "ss", "se")
    whole = ctx.seed_allvsall(seg_len=50_000)
    tw = OracleCtx()
    tw.genome_pack(g["contigs"])
    parts = []
    try:
        for r in range(3):
            ctx.seed_shard(r, 3)
            tw.seed_shard(r, 3)
            share = ctx.seed_allvsall(seg_len=50_000)
            twin = tw.seed_allvsall(seg_len=50_000)
            auto = ctx.seed_allvsall(seg_len=50_000, max_anchors=share["stats"][1] // 3)
            assert auto.get("shares", 1) >= 2 and auto["stats"][1] == share["stats"][1], (r, auto.get("shares"), auto["stats"], share["stats"])
            for k in keys:
                assert np.array_equal(auto[k], share[k]), (r, k, len(auto[k]), len(share[k]))
                assert np.array_equal(auto[k], twin[k]), (r, k)
            assert 0 < len(auto["qseg"]) < len(whole["qseg"])
            again = ctx.seed_allvsall(seg_len=50_000)          # the shard survived the split
            for k in keys:
                assert np.array_equal(again[k], share[k]), (r, k, len(again[k]), len(share[k]))
            parts.append(np.stack([np.asarray(auto[k], dtype=np.int64) for k in keys], axis=1))
    finally:
        ctx.seed_shard(0, 0)
    rows = np.concatenate(parts)
    rows = rows[np.argsort(rows[:, 0] * 100000 + rows[:, 1], kind="stable")]
    for i, k in enumerate(keys):
        assert np.array_equal(rows[:, i], np.asarray(whole[k], dtype=np.int64)), k
    again = ctx.seed_allvsall(seg_len=50_000)
    assert all(np.array_equal(again[k], whole[k]) for k in keys)


def test_coarse_stage_sharded_over_rccl_world1(ctx):
    """the collectives of the sharded coarse stage on their RCCL code path (all_gather_into_tensor, all_to_all_single with split
    sizes, the padded variable-length all-gather): one rank, backend "nccl" -- the result must be the stage without a process
    group.  (Two ranks are checked with gloo and the CPU twins in tests/test_dist_gloo.py; a multi-GPU node was never available.)"""
    import socket

    import synth_small
    import torch
    import torch.distributed as dist
    from hite_amd import dist as hd

    g = synth_small.make(31, n_fam=14, n_chr=3, chr_len=150_000)
    ctx.genome_pack(g["contigs"])
    ctx.release_copy_index()
    plain = hd.coarse_stage_sharded(ctx, 50_000, 2000, 30000, base_threshold=100_000)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        # world 1 takes the single-rank shortcut inside coarse_stage_sharded: call the exchange helpers directly as well
        rows = np.arange(60, dtype=np.int64).reshape(10, 6)
        got = hd._exchange_rows(rows, np.zeros(10, dtype=np.int64), None, torch.device("cuda", 0))
        assert np.array_equal(got, rows)
        allv, sizes = hd.allgather_varlen(torch.arange(7, dtype=torch.int64, device="cuda"), None)
        assert allv.cpu().tolist() == list(range(7)) and sizes.tolist() == [7]
        shard = hd.coarse_stage_sharded(ctx, 50_000, 2000, 30000, device=torch.device("cuda", 0), base_threshold=100_000)
    finally:
        dist.destroy_process_group()
    assert [x.tolist() for x in shard] == [x.tolist() for x in plain] and len(plain[0]) >= 20


def test_coarse_stage_sharded_two_ranks_on_one_gpu(ctx, tmp_path):
    """stage 3.1 sharded over TWO ranks with the real device stages on each (hite_seed_shard's share of the anchors, the all-to-all
    of HSP records to the owners of the query files, hite_fmea_chain per owned file, the all-gather of the interval lists): the
    ranks share this GPU and exchange over gloo (tests/_coarse_two_ranks.py under torch.distributed.run) -- the merged intervals
    must be the unsharded stage's.  (RCCL between two GPUs stays unmeasured: no node.)"""
    import json
    import subprocess
    import sys
    import synth_small
    from hite_amd import dist as hd

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    g = synth_small.make(31, n_fam=14, n_chr=3, chr_len=150_000)
    ctx.genome_pack(g["contigs"])
    ctx.release_copy_index()
    plain = hd.coarse_stage_sharded(ctx, 50_000, 2000, 30000, base_threshold=100_000)
    out = tmp_path / "sharded.json"
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import socket

    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(root, "tests", "_coarse_two_ranks.py"), str(out)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    shard = json.load(open(out))
    assert shard == [np.asarray(x).tolist() for x in plain] and len(plain[0]) >= 20


def test_itr_search_tool_golden_and_twin(ctx):
    """hite_itr_search (the in-tree stage where the reference runs tools/itrsearch -i 0.7 -l 7, Util.py:216-224) against the tool's
    own output (3 300 records), then field for field against the twin on fresh records: 20 000 first-40 + last-40 records (LDS path),
    600 whole sequences up to 2 kb (scratch path, 8 strips), other thresholds and scores, empty and one-base records"""
    import itr_cases

    itr_cases.check_tool_records(lambda seqs, e: ctx.itr_search(seqs, end_len=e))
    fresh = casegen.make_itr_cases(6101, 20000)
    assert np.array_equal(ctx.itr_search(fresh, end_len=40), O.itr_search(fresh, 40))
    assert np.array_equal(ctx.itr_search(fresh[:3000], end_len=0), O.itr_search(fresh[:3000], 0))
    whole = casegen.make_itr_cases(6102, 600, long_=True)
    a, b = ctx.itr_search(whole, end_len=0), O.itr_search(whole, 0)
    assert np.array_equal(a, b) and int(a[:, 5].sum()) > 300 and int(a[:, 1].max()) > 450
    mixed = whole[:50] + fresh[:50] + ["", "A", "AT", "ACGT", "N" * 90, "ACGTN" * 30]
    for kw in (dict(min_identity=0.8, min_len=10), dict(min_identity=0.75, min_len=5, match=5, mismatch=4, gap_open=8, gap_extend=2),
               dict(min_identity=0.0, min_len=0, match=1, mismatch=3, gap_open=5, gap_extend=2)):
        for e in (0, 40, 7, 200):
            assert np.array_equal(ctx.itr_search(mixed, end_len=e, **kw),
                                  O.itr_search(mixed, e, kw["min_identity"], kw["min_len"], kw.get("match", 10), kw.get("mismatch", 16),
                                               kw.get("gap_open", 32), kw.get("gap_extend", 32)))


def test_itr_filter_host_mirrors_golden_on_gpu(ctx):
    """search_confident_tir_batch_v1 (Util.py:6533-6628) and remove_no_tirs (Util.py:13897-13920) through the HIP library against the
    reference's own runs with the tool: variants without a terminal inverted repeat are dropped, never passed through"""
    import itr_cases
    from hite_amd import util

    n_q, n_drop = itr_cases.check_batches(util, ctx)
    assert n_drop > n_q
    itr_cases.check_rescue(util, ctx)


def test_flanking_seq_dev_windows_vs_oracle(ctx):
    """generate_final_result + flanking_seq on the device (Context.flanking_seq_dev: what the end-to-end coarse step of bench.py
    runs): every window == the oracle's clamping rule (Util.py:4614-4634) applied to the contig, for intervals at contig starts and
    ends, shorter than two flanks, and in the middle"""
    names, seqs = casegen.make_genome(911, n_chr=3, chr_len=(4000, 30000), other_frac=0.0)
    ctx.genome_pack(seqs)
    rng = np.random.default_rng(912)
    c, a, b = [], [], []
    for k in range(400):
        ci = int(rng.integers(0, 3)); L = len(seqs[ci])
        ln = int(rng.choice([80, 150, 1200, 3000]))
        s0 = int(rng.choice([0, 3, 49, 50, 51, max(0, L - ln - 30), max(0, L - ln), int(rng.integers(0, max(1, L - ln)))]))
        c.append(ci); a.append(s0); b.append(min(L, s0 + ln))
    total = ctx.flanking_seq_dev(c, a, b, 50)
    out, off, ln = ctx.flank_windows
    fold = lambda s: "".join(ch if ch in "ACGT" else "N" for ch in s)  # noqa: E731
    got_total = 0
    for k in range(len(c)):
        lo, hi, _ns, _ne = O.flanking_seq(a[k], b[k], len(seqs[c[k]]), 50)        # the slice [lo, hi) of the contig
        exp = fold(seqs[c[k]][lo:hi])
        if int(ln[k]) == 0:            # (the gather's 100-base rule; flanking_seq itself has no minimum)
            assert len(exp) < 100
            continue
        assert out[int(off[k]):int(off[k]) + int(ln[k])].tobytes().decode() == exp, k
        got_total += int(ln[k])
    assert got_total == total and total > 100_000


def test_low_copy_rescue_golden_on_gpu(ctx, tmp_path, monkeypatch):
    """the low-copy recall (Util.py:8196-8287) with the HIP terminal-inverted-repeat stage: real_TEs, all_low_copy and the domain
    table of the reference's own run (TRF + itrsearch + get_domain_info over a fabricated blastx table)"""
    import itr_cases
    from hite_amd import util

    itr_cases.check_low_copy_rescue(util, ctx, tmp_path, monkeypatch)


def test_allgather_records_on_a_callers_rccl_communicator(ctx):
    """hite_allgather_records: ONE ncclAllGather on the communicator the caller owns.  Here the caller is this test: a
    world-1 communicator made with RCCL's own C API (the RCCL torch carries, reached through ctypes), 50 000 call records"""
    import ctypes as C

    import torch

    libdir = os.path.join(os.path.dirname(torch.__file__), "lib")
    path = os.path.join(libdir, "librccl.so")
    if not os.path.exists(path):
        pytest.skip("no librccl.so beside torch")
    rccl = C.CDLL(path, mode=C.RTLD_GLOBAL)

    class UniqueId(C.Structure):
        _fields_ = [("internal", C.c_char * 128)]

    uid = UniqueId()
    assert rccl.ncclGetUniqueId(C.byref(uid)) == 0
    comm = C.c_void_p()
    rccl.ncclCommInitRank.argtypes = [C.POINTER(C.c_void_p), C.c_int, UniqueId, C.c_int]
    torch.cuda.set_device(0)
    assert rccl.ncclCommInitRank(C.byref(comm), 1, uid, 0) == 0
    try:
        n = 50_000 * 32
        send = torch.randint(0, 255, (n,), dtype=torch.uint8, device="cuda:0")
        recv = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        ctx.allgather_records(comm.value, send.data_ptr(), recv.data_ptr(), n)
        torch.cuda.synchronize()
        assert torch.equal(send, recv)
    finally:
        rccl.ncclCommDestroy.argtypes = [C.c_void_p]
        rccl.ncclCommDestroy(comm)
