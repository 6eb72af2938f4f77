"""GPU: the high-copy LTR vote of FiLTR's hybrid CNN (include/hite_gpu.h, hite_ltr_deep) against its twin (tests/ltrdeep_twin.py) and
against what the reference recorded (tests/golden/ltr_deep.json.gz): the integer features byte for byte, the logits within the
fixture's tolerance T (32 x the largest |reference fp32 - twin binary64| measured on the CPU; never widened here), the decisions
exactly; a second model of seeded random parameters on matrices whose only bases sit at the corners and at the tile edges of the
kernels; the same bits at every batch size and place in a batch; and the stage around it on a miniature genome."""
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import framecluster_twin as FT
import ltrdeep_twin as T
import oracle_lib as O
from conftest import load_golden
from hite_amd import synth, util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_constants():
    txt = open(os.path.join(ROOT, "include", "hite_gpu.h")).read()
    return {k: int(v) for k, v in re.findall(r"#define\s+HITE_LTRDEEP_(\w+)\s+(\d+)", txt)}


@pytest.fixture(scope="module")
def ctx():
    import hite_amd

    c = hite_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fix(ctx):
    """the fixture, its model on the device, and the twin's answers on every fixture matrix (computed once)"""
    doc = load_golden("ltr_deep")
    params = np.load(os.path.join(ROOT, "tests", "golden", "ltr_deep_model.npy"))
    mats = [c["matrix"] for c in doc["cases"]]
    logits, pooled, status = T.ltr_deep(params, mats, pooled=True)
    assert not status.any()
    return dict(doc=doc, params=params, mats=mats, logits=logits, pooled=pooled, model=ctx.ltr_model(params), T=doc["tolerance"]["T"])


def test_constants_of_the_header():
    k = header_constants()
    assert (k["PARAMS"], k["ROWS"], k["COLS"], k["KMER"]) == (T.PARAMS, T.ROWS, T.COLS, T.KMER) == (40026, 100, 200, 3872)
    assert 1 <= k["TILE_H"] < T.ROWS and 1 <= k["TILE_W"] < T.COLS and 1 <= k["KMER_TILE"] < T.KMER      # several tiles on every axis
    assert k["BATCH_DEFAULT"] >= 9


def test_features_equal_twin_and_reference(ctx, fix):
    img, kmer, status = ctx.ltr_deep_features(fix["mats"])
    t_img, t_kmer, t_status = T.ltr_deep_features(fix["mats"])
    assert not status.any() and not t_status.any()
    assert img.dtype == np.uint8 and kmer.dtype == np.int32 and img.tobytes() == t_img.tobytes() and kmer.tobytes() == t_kmer.tobytes()
    for k, c in enumerate(fix["doc"]["cases"]):
        assert hashlib.sha256(img[k].astype(np.int64).tobytes()).hexdigest() == c["img_sha256"], c["name"]
        assert hashlib.sha256(kmer[k].astype(np.int64).tobytes()).hexdigest() == c["kmer_sha256"], c["name"]
    # as a dict, as ltr_flank_decide hands the matrices over
    d_img, _k, _s = ctx.ltr_deep_features({c["name"]: [tuple(r) for r in c["matrix"]] for c in fix["doc"]["cases"][:3]})
    assert d_img.tobytes() == img[:3].tobytes()


def test_not_scored_matrices_and_empty_call(ctx, fix):
    good = fix["mats"][1]
    row = "".join(good[0])
    mats = [good, [row] * 101, fix["mats"][0], [row] * 4, good, [r[:199] for r in ["".join(x) for x in good]], fix["mats"][7], []]
    logits, pooled, status = ctx.ltr_deep(fix["model"], mats, pooled=True)
    assert status.tolist() == [0, 1, 0, 1, 0, 1, 0, 1]
    alone, alone_pooled, _s = ctx.ltr_deep(fix["model"], [good, fix["mats"][0], fix["mats"][7]], pooled=True)
    assert logits[[0, 2, 6]].tobytes() == alone.tobytes() and logits[4].tobytes() == alone[0].tobytes()          # the neighbours are unaffected
    assert pooled[[0, 2, 6]].tobytes() == alone_pooled.tobytes()
    assert not logits[[1, 3, 5, 7]].any() and not pooled[[1, 3, 5, 7]].any()
    img, kmer, f_status = ctx.ltr_deep_features(mats)
    assert f_status.tolist() == status.tolist() and not img[[1, 3, 5, 7]].any() and not kmer[[1, 3, 5, 7]].any()
    assert img[4].tobytes() == T.ltr_deep_features([good])[0][0].tobytes()
    logits, status = ctx.ltr_deep(fix["model"], [])
    assert logits.shape == (0, 2) and status.shape == (0,)
    assert [a.shape[0] for a in ctx.ltr_deep_features([])] == [0, 0, 0]
    logits, status = ctx.ltr_deep(fix["model"], [[row] * 4])          # a call without a scored matrix
    assert status.tolist() == [1] and not logits.any()


def test_refused_arguments(ctx, fix):
    import hite_amd

    with pytest.raises(hite_amd.HiteError):
        ctx.ltr_model(fix["params"][:-1])
    bad = fix["params"].copy()
    bad[100] = np.nan
    with pytest.raises(hite_amd.HiteError):
        ctx.ltr_model(bad)
    assert ctx.ltr_deep(fix["model"], fix["mats"][:1])[1].tolist() == [0]          # the context stays usable


def test_logits_and_decisions(ctx, fix):
    doc = fix["doc"]
    logits, pooled, status = ctx.ltr_deep(fix["model"], fix["mats"], pooled=True)
    assert not status.any() and logits.dtype == np.float32
    err, err_pool = np.abs(logits.astype(np.float64) - fix["logits"]).max(), np.abs(pooled.astype(np.float64) - fix["pooled"]).max()
    ref = np.array([c["logits"] for c in doc["cases"]])
    print("largest |device - twin|: logits %.3g, pooled %.3g; |device - reference| logits %.3g; T = %.3g" %
          (err, err_pool, np.abs(logits.astype(np.float64) - ref).max(), fix["T"]))
    assert err <= fix["T"] and err_pool <= fix["T"]
    names = [c["name"] for c in doc["cases"]]
    votes = util.ltr_deep_votes(dict(zip(names, fix["mats"])), fix["model"], doc["threshold"], ctx=ctx)
    assert votes == {c["name"]: c["decision"] for c in doc["cases"]}
    assert votes == util.ltr_deep_votes(dict(zip(names, fix["mats"])), fix["params"], doc["threshold"], ctx=ctx)      # the flat array as the model


def random_params(seed):
    """seeded parameters in which every weight matters: weights of variance 1.5 / fan-in, batch norms with gamma of either sign"""
    rng = np.random.default_rng(seed)
    parts = []
    for key, shape in T.SPEC:
        n = int(np.prod(shape))
        if key.endswith("running_var"):
            v = rng.uniform(0.5, 1.5, n)
        elif key.endswith("running_mean") or key.endswith("bias"):
            v = rng.normal(0.0, 0.2, n)
        elif len(shape) == 1:          # gamma
            v = rng.uniform(0.6, 1.4, n) * rng.choice([-1.0, 1.0], n)
        else:
            v = rng.normal(0.0, np.sqrt(1.5 / (n // shape[0])), n)
        parts.append(v.astype(np.float32))
    return np.concatenate(parts)


def edge_matrices():
    """matrices of 100 rows that are all gaps but for single bases: the four corners; the rows and columns just inside and outside
    every tile edge of the image kernels; then rows that hold one k-mer word each, for the slots 0, 1, 3870, 3871 and the slots on
    either side of every tile edge of the k-mer axis"""
    k = header_constants()
    th, tw, kt = k["TILE_H"], k["TILE_W"], k["KMER_TILE"]
    blank = lambda: [["-"] * T.COLS for _ in range(T.ROWS)]  # noqa: E731
    join = lambda m: ["".join(r) for r in m]  # noqa: E731
    corners = blank()
    for r, c, ch in ((0, 0, "A"), (0, 199, "C"), (99, 0, "G"), (99, 199, "T")):
        corners[r][c] = ch
    rows_e = sorted({r for e in range(th, T.ROWS, th) for r in (e - 1, e)})
    cols_e = sorted({c for e in range(tw, T.COLS, tw) for c in (e - 1, e)})
    edges, diag = blank(), blank()
    for i, r in enumerate(rows_e):
        for j, c in enumerate(cols_e):
            edges[r][c] = "ACGT"[(i + j) % 4]
    for i, (r, c) in enumerate(zip(rows_e, cols_e + cols_e)):
        diag[r][c] = "ACGT"[i % 4]
    slots = [0, 1, T.KMER - 2, T.KMER - 1] + sorted({s for e in range(kt, T.KMER, kt) for s in (e - 1, e)})
    words = blank()
    for r, s in enumerate(slots):
        for kk, first in ((3, 0), (4, 124), (5, 748)):
            if first <= s < first + 5 ** kk - 1:
                word = "".join("AGCT-"[(s - first) // 5 ** (kk - 1 - j) % 5] for j in range(kk))
        words[r][10 + 100 * (r % 2):10 + 100 * (r % 2) + len(word)] = list(word)
    return [join(corners), join(edges), join(diag), join(words)], slots


def test_random_model_at_corners_and_tile_edges(ctx, fix):
    mats, slots = edge_matrices()
    _img, kmer, status = ctx.ltr_deep_features(mats)
    assert not status.any() and all(kmer[3, r % 2, s] >= 1 for r, s in enumerate(slots))          # every wanted slot is met
    params = random_params(99)
    assert (T.unpack(params)["model.1.bn2.weight"] < 0).any()
    model = ctx.ltr_model(params)
    logits, pooled, status = ctx.ltr_deep(model, mats, pooled=True)
    model.release()
    t_logits, t_pooled, _s = T.ltr_deep(params, mats, pooled=True)
    err, err_pool = np.abs(logits - t_logits).max(), np.abs(pooled - t_pooled).max()
    print("random model: largest |device - twin| logits %.3g, pooled %.3g (|logit| up to %.3g, pooled up to %.3g); T = %.3g" %
          (err, err_pool, np.abs(t_logits).max(), np.abs(t_pooled).max(), fix["T"]))
    assert len({tuple(np.round(l, 3)) for l in t_logits}) == len(mats)          # the four matrices are told apart
    assert err <= fix["T"] and err_pool <= fix["T"]


def test_same_bits_at_every_batch_size_and_place(fix, tmp_path):
    """HITE_LTRDEEP_BATCH is read when a context is created: a child process per batch size"""
    res = {}
    for batch in ("1", "4", None):
        out = tmp_path / ("batch_%s.npz" % batch)
        env = {k: v for k, v in os.environ.items() if k != "HITE_LTRDEEP_BATCH"}
        if batch:
            env["HITE_LTRDEEP_BATCH"] = batch
        subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_ltrdeep_child.py"), str(out)], check=True, env=env, timeout=300)
        res[batch] = np.load(out)
    first = res[None]["logits"][0].tobytes(), res[None]["pooled"][0].tobytes()
    for batch, r in res.items():
        assert r["logits"].shape == (3, 9, 2)
        for k in range(3):
            assert (r["logits"][k].tobytes(), r["pooled"][k].tobytes()) == first, (batch, k)
    assert np.abs(res["1"]["logits"][0] - fix["logits"][:9]).max() <= fix["T"]


PLAN = [("ltr", 3), ("ltr", 12), ("ltr", 4), ("ltr", 7), ("inner", 8), ("inner", 3), ("left", 8), ("right", 8), ("left", 20), ("ltr", 1)]
FLANK = 100


def frame_vote(matrices, flank, window, side):
    return [O.ltr_frame(list(rows), flank, window, side) for rows in matrices]


def test_stage_on_a_miniature_genome(fix, tmp_path):
    """the genome and plan of tests/test_gpu_ltr_filter.py: the flank filter with the model on the device == the same call through
    the twin; hybrid_ltr_deep on the `.matrix` directory of the high-copy candidates == ltr_deep_votes"""
    g = synth.make_ltr_flank_genome(PLAN, seed=5)
    ref = str(tmp_path / "genome.fa")
    util.store_fasta({"chr_%d" % k: c for k, c in enumerate(g["contigs"])}, ref)
    uctx = util.set_reference(ref)
    seconds = {}
    table, high = util.ltr_flank_filter(g["terminals"], ref, FLANK, ctx=uctx, model=fix["params"], seconds=seconds)
    assert "deep" in seconds and len(high) >= 2
    assert (table, high) == util.ltr_flank_filter(g["terminals"], ref, FLANK, ctx=uctx, model=fix["params"], deep=T.ltr_deep)
    assert (table, high) == util.ltr_flank_filter(g["terminals"], ref, FLANK, ctx=uctx, cluster=FT.frame_cluster, frame_vote=frame_vote,
                                                  model=fix["params"], deep=T.ltr_deep)
    plain, _high = util.ltr_flank_filter(g["terminals"], ref, FLANK, ctx=uctx)
    votes = util.ltr_deep_votes(high, fix["params"], ctx=uctx)
    assert sorted(votes) == sorted(high)
    for n, v in plain.items():
        assert table[n] == ((False, "high", "deep") if n in high and v[0] and not votes[n] else v), n
    d = tmp_path / "high"
    os.makedirs(d)
    for n, rows in high.items():
        util._write_matrix(str(d / (n + ".matrix")), rows)
    got = util.hybrid_ltr_deep(str(d), os.path.join(ROOT, "tests", "golden", "ltr_deep_model.npy"), str(tmp_path / "deep"), ctx=uctx)
    assert got == votes
    assert open(tmp_path / "deep" / "is_LTR_deep.txt").read() == "".join("%s\t%d\n" % (n, votes[n]) for n in sorted(votes))
