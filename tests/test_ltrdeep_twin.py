"""CPU: the twin of the high-copy LTR vote (tests/ltrdeep_twin.py) against what the reference's own feature extractor, model and merge
recorded in tests/golden/ltr_deep.json.gz (tools/gen_ltr_deep_fixture.py), a second opinion on its layers from torch in float64,
and the host functions around the model's parameters."""
import hashlib
import os

import numpy as np
import pytest

import ltrdeep_twin as T
from conftest import load_golden
from hite_amd import util

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def fix():
    doc = load_golden("ltr_deep")
    params = np.load(os.path.join(HERE, "golden", "ltr_deep_model.npy"))
    mats = [c["matrix"] for c in doc["cases"]]
    logits, pooled, status = T.ltr_deep(params, mats, pooled=True)          # computed once for the tests below
    return dict(doc=doc, params=params, mats=mats, logits=logits, pooled=pooled, status=status)


def test_fixture_covers_what_it_promises(fix):
    cases = fix["doc"]["cases"]
    assert {len(c["matrix"]) for c in cases} >= {6, 7, 63, 64, 65, 99, 100}
    assert {c["decision"] for c in cases} == {0, 1}
    assert all(abs(c["logits"][1] - c["logits"][0]) >= fix["doc"]["min_gap"] for c in cases)
    tol = fix["doc"]["tolerance"]
    assert tol["T"] == 32 * tol["measured"] and 0 < tol["measured"] < 1e-5
    pairs, all_gap_col, n_only, lower, gap_half = set(), False, False, False, False
    for m in fix["mats"]:
        rows = ["".join(r) for r in m]
        for c in range(T.COLS):
            col = [r[c] for r in rows]
            total = sum(ch in "ACGT" for ch in col)
            pairs |= {(col.count(b), total) for b in "ACGT"}
            all_gap_col |= all(ch == "-" for ch in col)
            n_only |= total == 0 and "N" in col
            lower |= any(ch in "acgt" for ch in col)
        gap_half |= all(set(r[100:]) == {"-"} for r in rows)
    assert pairs >= set(T.SPECIAL_SUPPORT) and all_gap_col and n_only and lower and gap_half


def test_features_equal_the_reference(fix):
    for c in fix["doc"]["cases"]:
        img, kmer = T.features(c["matrix"])
        for key, row in c["img_rows"].items():          # the raw rows first: they say where a digest differs
            p, r = (int(x) for x in key.split(","))
            assert img[p, r].tolist() == row, (c["name"], key)
        assert kmer[:, :130].tolist() == c["kmer_head"] and kmer.sum(axis=1).tolist() == c["kmer_sum"], c["name"]
        assert hashlib.sha256(np.ascontiguousarray(img, dtype=np.int64).tobytes()).hexdigest() == c["img_sha256"], c["name"]
        assert hashlib.sha256(np.ascontiguousarray(kmer, dtype=np.int64).tobytes()).hexdigest() == c["kmer_sha256"], c["name"]


def test_logits_and_decisions_equal_the_reference(fix):
    doc = fix["doc"]
    assert not fix["status"].any()
    ref = np.array([c["logits"] for c in doc["cases"]])
    err = np.abs(fix["logits"] - ref).max()
    print("largest |reference fp32 logit - twin binary64 logit| = %.3g (recorded %.3g, T %.3g)" % (err, doc["tolerance"]["measured"], doc["tolerance"]["T"]))
    assert err <= doc["tolerance"]["T"]
    votes = util.ltr_deep_votes({c["name"]: c["matrix"] for c in doc["cases"]}, fix["params"], doc["threshold"], deep=T.ltr_deep)
    assert votes == {c["name"]: c["decision"] for c in doc["cases"]}


def test_layers_equal_torch_float64(fix):
    """F.conv2d / F.batch_norm in float64 with the fixture's parameters on two matrices: every activation of the twin within 1e-9"""
    import torch
    F = torch.nn.functional
    P = T.unpack(fix["params"])
    tp = {k: torch.from_numpy(v) for k, v in P.items()}
    bn = lambda x, key: F.batch_norm(x, tp[key + ".running_mean"], tp[key + ".running_var"], tp[key + ".weight"], tp[key + ".bias"], False, 0.0, 1e-5)  # noqa: E731
    for k in (0, 20):
        acts = T.activations(fix["mats"][k], P)
        pooled = []
        for branch, x0 in (("model", acts["x_img"]), ("model_kmer", acts["x_kmer"])):
            x = torch.from_numpy(x0)[None]
            for b in range(3):
                key = "%s.%d" % (branch, b)
                t = F.relu(bn(F.conv2d(x, tp[key + ".conv1.weight"], padding=1), key + ".bn1"))
                assert np.abs(t[0].numpy() - acts[key + ".relu1"]).max() <= 1e-9, key
                y = bn(F.conv2d(t, tp[key + ".conv2.weight"], padding=1), key + ".bn2")
                s = bn(F.conv2d(x, tp[key + ".shortcut.0.weight"]), key + ".shortcut.1")
                assert np.abs(y[0].numpy() - acts[key + ".bn2"]).max() <= 1e-9 and np.abs(s[0].numpy() - acts[key + ".shortcut"]).max() <= 1e-9, key
                x = F.relu(y + s)
                assert np.abs(x[0].numpy() - acts[key]).max() <= 1e-9, key
            pooled.append(F.adaptive_avg_pool2d(x, (1, 1)).flatten(1))
        h = torch.cat(pooled, 1)
        assert np.abs(h[0].numpy() - acts["pooled"]).max() <= 1e-9 and np.abs(acts["pooled"] - fix["pooled"][k]).max() <= 1e-12
        h = F.relu(bn(F.linear(h, tp["fc_layers.0.weight"], tp["fc_layers.0.bias"]), "fc_layers.1"))
        assert np.abs(h[0].numpy() - acts["fc1"]).max() <= 1e-9
        h = F.relu(bn(F.linear(h, tp["fc_layers.4.weight"], tp["fc_layers.4.bias"]), "fc_layers.5"))
        assert np.abs(h[0].numpy() - acts["fc2"]).max() <= 1e-9
        h = F.linear(h, tp["fc_layers.8.weight"], tp["fc_layers.8.bias"])
        assert np.abs(h[0].numpy() - acts["logits"]).max() <= 1e-9 and np.abs(acts["logits"] - fix["logits"][k]).max() <= 1e-12


def test_support_table():
    tab = T.support_table()
    differ = set()
    for t in range(1, 101):
        for c in range(0, t + 1):
            assert tab[c, t] == int((c / t) * 100)
            if tab[c, t] != 100 * c // t:
                differ.add((c, t))
    assert differ == {(29, 50), (29, 100), (57, 100), (58, 100)} == set(T.SPECIAL_SUPPORT)
    assert tab[29, 50] == 57 and tab[29, 100] == 28 and tab[57, 100] == 56 and tab[58, 100] == 57
    assert all(tab[c, t] == v for (c, t), v in T.SPECIAL_SUPPORT.items()) and not tab[:, 0].any()


def test_merge_equals_the_reference(fix):
    kinds = set()
    for m in fix["doc"]["merge"]:
        got = util.alter_deep_learning_results(m["deep"], m["homology"], m["names"])
        assert got == m["result"] == T.merge(m["deep"], m["homology"], m["names"]), m
        kinds.add((bool(m["deep"]), bool(m["homology"])))
        if "absent" in m["names"]:
            assert "absent" not in got and got["vetoed"] == 0
    assert kinds == {(False, False), (False, True), (True, False), (True, True)}


def test_model_params_round_trip(fix, tmp_path, monkeypatch):
    state = util.ltr_model_state(fix["params"])
    assert [k for k, _s in T.SPEC] == list(state) and sum(v.size for v in state.values()) == util.LTR_MODEL_PARAMS == T.PARAMS == 40026
    assert all(np.array_equal(state[k], T.unpack(fix["params"])[k].astype(np.float32)) for k in state)
    prefixed = {"module." + k: v for k, v in state.items()}
    prefixed["module.model.0.bn1.num_batches_tracked"] = np.array(7)
    assert np.array_equal(util.ltr_model_params(prefixed), fix["params"])
    missing = dict(state)
    del missing["model_kmer.1.shortcut.1.running_var"]
    with pytest.raises(ValueError, match="model_kmer.1.shortcut.1.running_var"):
        util.ltr_model_params(missing)
    wrong = dict(state, **{"fc_layers.4.weight": np.zeros((16, 8), dtype=np.float32)})
    with pytest.raises(ValueError, match="fc_layers.4.weight"):
        util.ltr_model_params(wrong)
    # load_ltr_model: the path, then $HITE_LTR_MODEL, then $HITE_FILTR_DIR/models/production_model.pth; None when nothing is there
    for var in ("HITE_LTR_MODEL", "HITE_FILTR_DIR", "HITE_LTR_DEEP"):
        monkeypatch.delenv(var, raising=False)
    assert util.load_ltr_model() is None and util.load_ltr_model(str(tmp_path / "none.npy")) is None
    npy = os.path.join(HERE, "golden", "ltr_deep_model.npy")
    assert np.array_equal(util.load_ltr_model(npy), fix["params"])
    monkeypatch.setenv("HITE_LTR_MODEL", npy)
    assert np.array_equal(util.load_ltr_model(), fix["params"])
    import torch
    os.makedirs(tmp_path / "filtr" / "models")
    torch.save({"model_state_dict": {k: torch.from_numpy(np.array(v)) for k, v in prefixed.items()}}, str(tmp_path / "filtr" / "models" / "production_model.pth"))
    monkeypatch.delenv("HITE_LTR_MODEL")
    monkeypatch.setenv("HITE_FILTR_DIR", str(tmp_path / "filtr"))
    assert np.array_equal(util.load_ltr_model(), fix["params"])
    monkeypatch.delenv("HITE_FILTR_DIR")
    monkeypatch.setenv("HITE_LTR_DEEP", "gpu")
    with pytest.raises(FileNotFoundError, match="HITE_LTR_MODEL"):
        util.ltr_flank_decide({}, cluster=lambda *a, **k: [], frame_vote=lambda *a, **k: [])


def test_hybrid_ltr_deep_directory_contract(fix, tmp_path):
    cases = fix["doc"]["cases"][:3]
    src, out = tmp_path / "high_copy_frames", tmp_path / "deep"
    os.makedirs(src)
    for c in cases:
        util._write_matrix(str(src / (c["name"] + ".matrix")), c["matrix"])
    util._write_matrix(str(src / "short.matrix"), cases[0]["matrix"][:4])          # fewer than 5 rows: not scored, in no table
    votes = util.hybrid_ltr_deep(str(src), os.path.join(HERE, "golden", "ltr_deep_model.npy"), str(out), fix["doc"]["threshold"], deep=T.ltr_deep)
    assert votes == {c["name"]: c["decision"] for c in cases}
    assert open(out / "is_LTR_deep.txt").read() == "".join("%s\t%d\n" % (c["name"], c["decision"]) for c in sorted(cases, key=lambda c: c["name"]))
    probs = dict(line.split("\t") for line in open(out / "deep_probs.csv").read().split("\n")[:-1])
    assert sorted(probs) == sorted(votes) and all((float(probs[n]) > 0.5) == bool(votes[n]) for n in votes)
