"""CPU twin of hite_ltr_deep (include/hite_gpu.h, "high-copy LTR vote"): a plain numpy restatement of the definition -- the
features in integers, the model in binary64 on the fp32-rounded inputs and parameters.  Nothing of the reference is imported; the
fixture tests/golden/ltr_deep.json.gz pins it to the reference."""
import numpy as np

ROWS, COLS, HALF, KMER, PARAMS = 100, 200, 100, 3872, 40026
DIGIT = {"A": 0, "G": 1, "C": 2, "T": 3}          # '-' (and every other byte) is digit 4
BASE_VALUE = np.array([50, 100, 75, 25, 0])     # A, G, C, T, '-'
SPECIAL_SUPPORT = {(29, 50): 57, (29, 100): 28, (57, 100): 56, (58, 100): 57}      # where int((c / t) * 100) is not 100 c // t


def support_table():
    """[count][total] -> int((count / total) * 100) as Python evaluates it in binary64 (0 where total is 0)"""
    tab = np.zeros((101, 101), dtype=np.int64)
    for t in range(1, 101):
        for c in range(0, t + 1):
            tab[c, t] = int((c / t) * 100)
    return tab


_SUPPORT = support_table()


def _rows(matrix):
    return ["".join(r) if isinstance(r, (tuple, list)) else (r.decode("latin-1") if isinstance(r, bytes) else r) for r in matrix]


def codes(matrix):
    """[100, 200] digits of a matrix (rows below the last are all 4), or None when the matrix is not scored"""
    rows = _rows(matrix)
    if len(rows) < 5 or len(rows) > ROWS or any(len(r) != COLS for r in rows):
        return None
    out = np.full((ROWS, COLS), 4, dtype=np.int64)
    for k, r in enumerate(rows):
        out[k] = [DIGIT.get(ch, 4) for ch in r]
    return out


def features(matrix):
    """(image int64 [3, 100, 200], k-mer counts int64 [2, 3872]) or None"""
    d = codes(matrix)
    if d is None:
        return None
    base = d < 4
    img = np.zeros((3, ROWS, COLS), dtype=np.int64)
    img[0] = np.where(base, 100, 0)
    total = base.sum(axis=0)
    for digit in range(4):
        hit = d == digit
        count = hit.sum(axis=0)
        img[1] += np.where(hit, _SUPPORT[count, total][None, :], 0)
    img[2] = BASE_VALUE[d]
    kmer = np.zeros((2, KMER), dtype=np.int64)
    for h in range(2):
        half = d[:, h * HALF:(h + 1) * HALF]
        at = 0
        for k in (3, 4, 5):
            n = HALF - k + 1
            word = np.zeros((ROWS, n), dtype=np.int64)
            for j in range(k):
                word = word * 5 + half[:, j:j + n]
            cnt = np.bincount(word.reshape(-1), minlength=5 ** k)
            kmer[h, at:at + 5 ** k - 1] = cnt[:5 ** k - 1]          # the all-gap word is the last number and has no slot
            at += 5 ** k - 1
        assert at == KMER
    return img, kmer


def normalise(x):
    """x / max(|x|_2, 1e-12) over axis 0 in binary64, rounded to fp32"""
    x = np.asarray(x, dtype=np.float64)
    return (x / np.maximum(np.sqrt((x * x).sum(axis=0, keepdims=True)), 1e-12)).astype(np.float32)


def _spec():
    bn = lambda key, c: [(key + "." + f, (c,)) for f in ("weight", "bias", "running_mean", "running_var")]  # noqa: E731
    spec = []
    for branch, c0 in (("model", 3), ("model_kmer", 2)):
        for k, (cin, cout) in enumerate(((c0, 8), (8, 16), (16, 32))):
            b = "%s.%d" % (branch, k)
            spec += [(b + ".conv1.weight", (cout, cin, 3, 3))] + bn(b + ".bn1", cout) + [(b + ".conv2.weight", (cout, cout, 3, 3))] + bn(b + ".bn2", cout)
            spec += [(b + ".shortcut.0.weight", (cout, cin, 1, 1))] + bn(b + ".shortcut.1", cout)
    spec += [("fc_layers.0.weight", (16, 64)), ("fc_layers.0.bias", (16,))] + bn("fc_layers.1", 16)
    spec += [("fc_layers.4.weight", (8, 16)), ("fc_layers.4.bias", (8,))] + bn("fc_layers.5", 8)
    spec += [("fc_layers.8.weight", (2, 8)), ("fc_layers.8.bias", (2,))]
    return spec


SPEC = _spec()


def unpack(params):
    """{state-dict key: binary64 array} of the fp32 values of the canonical flat array"""
    params = np.asarray(params, dtype=np.float32).reshape(-1)
    assert params.size == PARAMS
    out, at = {}, 0
    for key, shape in SPEC:
        n = int(np.prod(shape))
        out[key] = params[at:at + n].reshape(shape).astype(np.float64)
        at += n
    assert at == PARAMS
    return out


def conv(x, w):
    """x [cin, H, W], w [cout, cin, k, k] (k 1 or 3, padding k // 2, stride 1) -> [cout, H, W]"""
    k = w.shape[2]
    p = k // 2
    _c, H, W = x.shape
    xp = np.pad(x, ((0, 0), (p, p), (p, p)))
    out = np.zeros((w.shape[0], H, W))
    for ky in range(k):
        for kx in range(k):
            out += np.tensordot(w[:, :, ky, kx], xp[:, ky:ky + H, kx:kx + W], axes=1)
    return out


def batch_norm(x, P, key):
    shape = (-1,) + (1,) * (x.ndim - 1)
    g, b, m, v = (P[key + "." + f].reshape(shape) for f in ("weight", "bias", "running_mean", "running_var"))
    return (x - m) / np.sqrt(v + 1e-5) * g + b


def block(x, P, key, acts=None):
    t = np.maximum(batch_norm(conv(x, P[key + ".conv1.weight"]), P, key + ".bn1"), 0.0)
    y = batch_norm(conv(t, P[key + ".conv2.weight"]), P, key + ".bn2")
    s = batch_norm(conv(x, P[key + ".shortcut.0.weight"]), P, key + ".shortcut.1")
    out = np.maximum(y + s, 0.0)
    if acts is not None:
        acts[key + ".relu1"], acts[key + ".bn2"], acts[key + ".shortcut"], acts[key] = t, y, s, out
    return out


def activations(matrix, P, img_kmer=None):
    """every intermediate of one candidate (P = unpack(params)): {"x_img", "x_kmer", "<branch>.<k>.relu1" | ".bn2" | ".shortcut",
    "<branch>.<k>" (the block's output), "pooled" [64], "fc1" [16], "fc2" [8], "logits" [2]}; img_kmer replaces the features"""
    img, kmer = img_kmer if img_kmer is not None else features(matrix)
    acts = {"x_img": normalise(img).astype(np.float64), "x_kmer": normalise(kmer[:, None, :]).astype(np.float64)}
    pooled = []
    for branch, x in (("model", acts["x_img"]), ("model_kmer", acts["x_kmer"])):
        for k in range(3):
            x = block(x, P, "%s.%d" % (branch, k), acts)
        pooled.append(x.mean(axis=(1, 2)))
    acts["pooled"] = np.concatenate(pooled)
    h = P["fc_layers.0.weight"] @ acts["pooled"] + P["fc_layers.0.bias"]
    acts["fc1"] = np.maximum(batch_norm(h, P, "fc_layers.1"), 0.0)
    h = P["fc_layers.4.weight"] @ acts["fc1"] + P["fc_layers.4.bias"]
    acts["fc2"] = np.maximum(batch_norm(h, P, "fc_layers.5"), 0.0)
    acts["logits"] = P["fc_layers.8.weight"] @ acts["fc2"] + P["fc_layers.8.bias"]
    return acts


def ltr_deep(params, matrices, pooled=False):
    """the signature of Context.ltr_deep with the flat parameter array as the model: binary64 logits [n, 2] (, pooled [n, 64]), int8
    status [n]"""
    mats = list(matrices.values()) if isinstance(matrices, dict) else list(matrices)
    P = unpack(params)
    logits, pool, status = np.zeros((len(mats), 2)), np.zeros((len(mats), 64)), np.zeros(len(mats), dtype=np.int8)
    for k, m in enumerate(mats):
        f = features(m)
        if f is None:
            status[k] = 1
            continue
        a = activations(m, P, f)
        logits[k], pool[k] = a["logits"], a["pooled"]
    return (logits, pool, status) if pooled else (logits, status)


def ltr_deep_features(matrices):
    """the signature of Context.ltr_deep_features"""
    mats = list(matrices.values()) if isinstance(matrices, dict) else list(matrices)
    img, kmer = np.zeros((len(mats), 3, ROWS, COLS), dtype=np.uint8), np.zeros((len(mats), 2, KMER), dtype=np.int32)
    status = np.zeros(len(mats), dtype=np.int8)
    for k, m in enumerate(mats):
        f = features(m)
        if f is None:
            status[k] = 1
        else:
            img[k], kmer[k] = f
    return img, kmer, status


def merge(deep_table, homology_table, high_copy_names):
    """the merge of the two tables as the issue's definition states it (dicts {name: 0 | 1})"""
    if not deep_table and not homology_table:
        return {n: 1 for n in high_copy_names}
    if not deep_table or not homology_table:
        return dict(deep_table or homology_table)
    out = dict(deep_table)
    out.update({n: 0 for n, v in homology_table.items() if not v})
    return out
