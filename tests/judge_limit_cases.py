"""Alignments of an EXACT width around the two widths where a judge kernel's anchor text (the ungapped row + 2 bytes of match
record per text start) stops fitting its LDS mask tile, and at 9 / 64 / 65 rows (64 rows is where the wavefront class ends):
inputs of tests/test_gpu_parity.py test_judge_at_anchor_lds_limits.  Inputs and expectations come from casegen and the oracle
alone; nothing here touches the GPU."""
import numpy as np

import casegen
import oracle_lib as O

FLANK = 50
ROWS = (9, 64, 65)
WAVE_OFFSETS = (-16, -8, -1, 0, 1, 8, 16)
BLOCK_OFFSETS = (-16, -1, 0, 1, 16)
TE_TYPES = ("tir", "non_ltr", "helitron")
# (shift_l, shift_r) of the candidate against the element, by case number: +42 puts an anchor 8 columns from the alignment's edge
SHIFTS = ((42, 0), (0, 0), (3, 0), (0, 42), (0, -4), (0, 0))


def to_width(mc, width, seed):
    """mc with whole columns deleted or duplicated until it has `width` columns; the columns come from the middle third of the
    element (FLANK columns of flank either side), away from both anchors and boundaries"""
    C = mc.shape[1]
    L = C - 2 * FLANK
    lo, hi = FLANK + L // 3, FLANK + 2 * L // 3
    delta = width - C
    assert abs(delta) <= (hi - lo) // 2
    rng = np.random.default_rng(seed)
    pick = np.sort(rng.choice(np.arange(lo, hi), size=abs(delta), replace=False))
    if delta < 0:
        out = np.delete(mc, pick, axis=1)
    else:
        rep = np.ones(C, dtype=np.int64)
        rep[pick] = 2
        out = np.repeat(mc, rep, axis=1)
    assert out.shape[1] == width
    return np.ascontiguousarray(out)


def _clean(c):
    m = O.msa_array(c["seqs"])
    keep = O.sparse_cols(m).astype(bool)
    return np.ascontiguousarray(m[:, keep])


def _judge_all(cases):
    """the oracle's call for plant 0 and 1 of every case; the oracle keeps no state between calls and ctypes drops the
    interpreter lock, so a few threads share the work (judge_boundary_v6 searches both anchors in every row: ~1 s at 65 x 5104)"""
    import os
    from concurrent.futures import ThreadPoolExecutor

    jobs = [(c, plant) for c in cases for plant in (0, 1)]
    with ThreadPoolExecutor(max(1, min(8, os.cpu_count() or 1))) as ex:
        res = list(ex.map(lambda j: O.judge(j[0]["te_type"], j[0]["mc"], j[0]["cand"], j[1]), jobs))
    for (c, plant), r in zip(jobs, res):
        c.setdefault("exp", {})[plant] = r


def build(wave_limit, block_limit):
    """-> list of dict(te_type, rows, C, mc, cand, exp: {plant: (call, bounds)}, left_edge, right_edge)"""
    cases = []
    for ti, te_type in enumerate(TE_TYPES):
        j = 0
        for fi, (limit, offsets) in enumerate(((wave_limit, WAVE_OFFSETS), (block_limit, BLOCK_OFFSETS))):
            bases = {}
            for ri, rows in enumerate((9, 65)):
                bases[rows] = _clean(casegen.make_msa_case(seed=86000 + 100 * ti + 10 * fi + ri, te_type=te_type, rows=rows, te_len=limit - 2 * FLANK,
                                                           flank=FLANK, div=0.04, ins_cols=0, tsd_len=8, tsd_frac=1.0))
            bases[64] = np.ascontiguousarray(bases[65][:64])          # (the 65-row family without its last, truncated row)
            assert sorted(bases) == sorted(ROWS)
            for ri, rows in enumerate(ROWS):
                for off in offsets:
                    C = limit + off
                    mc = to_width(bases[rows], C, 1000 * C + rows)
                    assert mc.shape == (rows, C) and (mc[0] != ord("-")).all()          # the ungapped anchor text of row 0 is C bytes long
                    row0 = mc[0].tobytes().decode()
                    sl, sr = SHIFTS[(j + ri) % len(SHIFTS)]
                    cand = row0[FLANK - sl:C - FLANK + sr]
                    cases.append({"te_type": te_type, "rows": rows, "C": C, "mc": mc, "cand": cand,
                                  "left_edge": 0 <= row0.find(cand[:20]) < 20, "right_edge": row0.rfind(cand[-20:]) + 20 > C - 20})
                    j += 1
    _judge_all(cases)
    return cases


def build_repetitive(wave_limit, block_limit, reps=33):
    """the widths limit - 1, limit, limit + 1 with a tandem array of the candidate's first 20 bases 40 columns behind the element's
    start and one of its last 20 bases 40 columns before its end, in every row: the anchor filter flags more than 64 match ends,
    so the search keeps a match record per text start -- the records are what lies BEHIND the text in the mask tile, up to the
    tile's last bytes at the limit.  The true ends are the first and the last overlap group, so the call still depends on them."""
    cases = []
    for ti, te_type in enumerate(TE_TYPES):
        for fi, limit in enumerate((wave_limit, block_limit)):
            c = casegen.make_msa_case(seed=87000 + 10 * ti + fi, te_type=te_type, rows=9, te_len=limit - 2 * FLANK - 40 * reps, flank=FLANK,
                                      div=0.04, ins_cols=0, tsd_len=8, tsd_frac=1.0)
            head, tail = c["cand"][:20] * reps, c["cand"][-20:] * reps
            a = FLANK + 60
            seqs = [s[:a] + head + s[a:len(s) - a] + tail + s[len(s) - a:] for s in c["seqs"]]
            base = _clean(dict(c, seqs=seqs))
            for off in (-1, 0, 1):
                mc = to_width(base, limit + off, 77 + off)
                assert (mc[0] != ord("-")).all()
                cases.append({"te_type": te_type, "rows": 9, "C": limit + off, "mc": mc, "cand": c["cand"]})
    _judge_all(cases)
    return cases


def te_counts(cases, plant=1):
    """{te_type: {C: alignments the oracle calls TE}} and the totals the conditions are about"""
    out = {}
    for c in cases:
        d = out.setdefault(c["te_type"], {})
        d[c["C"]] = d.get(c["C"], 0) + (c["exp"][plant][0][0] is True)
    return out


def check_conditions(cases):
    for te_type in TE_TYPES:
        sub = [c for c in cases if c["te_type"] == te_type]
        n_te = sum(c["exp"][1][0][0] is True for c in sub)
        assert 3 * n_te >= len(sub), (te_type, n_te, len(sub))
        assert any(c["left_edge"] for c in sub) and any(c["right_edge"] for c in sub), te_type
