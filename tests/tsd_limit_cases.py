"""Sequences for tests/test_gpu_tsd_limits.py and tests/test_tsd_limit_cases.py: the two kernels of hite_amd/csrc/hite_tsd.hip at
the limits of their own code -- tsd_kmer_kernel (hite_tsd_kmer: flanks 0..63 in LDS windows of 128 slots walked in two passes of 64
lanes, the cut at 100 records in the canonical order, bytes outside ACGT) and nonltr_prep_kernel (hite_nonltr_prep: the closed form
np_near1 of "within one edit", the rounds of 64 lanes of the TSD search, python slices that go below zero on sequences shorter
than a flank, the tail of the four-candidates-per-block grid).  Pure numpy / python, seeded.  Written once and run twice: every
check_* takes a callable with the signature of Context.tsd_kmer(seqs, flank, plant) or Context.nonltr_prep(seqs, flank, win5) and
compares it with the CPU twin (oracle_lib.tir_kmer / oracle_lib.nonltr_prep) -- exact integer equality, no tolerance anywhere.

Every builder asserts the property its cases are named for on the CPU -- with the twin and, for the k-mer search, with a plain
python statement of the twin's rule that returns the list BEFORE the cut (kmer_records_uncut) -- and returns the figures."""
import numpy as np

import oracle_lib as O

KS = (2, 3, 4, 5, 6, 8, 9, 10, 11)     # the TSD lengths of the k-mer search
TOP = 100                              # records kept per candidate
PASS_LANES = 64                        # one pass over the LDS windows; one round of the non-LTR TSD search
BASES = "ACGT"

_memo = {}


def cached(key, build):
    if key not in _memo:
        _memo[key] = build()
    return _memo[key]


def rand_seq(rng, n, alphabet=BASES):
    return "".join(alphabet[i] for i in rng.integers(0, len(alphabet), size=n))


def put(s, at, piece):
    """s with `piece` written over it at `at` (clipped to s)"""
    if at < 0:
        piece, at = piece[-at:], 0
    piece = piece[:max(0, len(s) - at)]
    return s[:at] + piece + s[at + len(piece):]


def raises(call):
    try:
        call()
    except RuntimeError:
        return True
    return False


# ------------------------------------------------------------------------------------------------------------------------------
# k-mer seeds: the rule, stated a second time
# ------------------------------------------------------------------------------------------------------------------------------
def kmer_records_uncut(seq, flank, plant, fold=None):
    """The rule of oracle/hite_oracle_coarse.c: orc_tir_kmer in plain python, WITHOUT the cut at 100: every record
    (k, tir_start, tir_end, distance) in the canonical order (distance, tir_start, tir_end, k).
    Per k: a right k-mer that also occurs in the left window gives, at EVERY right occurrence, a record of the left occurrence
    closest to the raw start (the first wins ties) and the right occurrence closest to the raw end among those visited so far;
    k = 4 only for TTAA, k = 2 only for TA or (plant == 0) CCC after the start and GGG before the end; records are a set over
    (k-mer, start, end); then the filters: NN in the k-mer, fewer than 100 bases, TG..CA, TATATATA / ATATATAT.
    fold: a 256-byte translation applied to the k-mers before they are COMPARED (and to nothing else) -- the model of a search
    that takes different bytes for one letter; None compares bytes."""
    b = seq.encode() if isinstance(seq, str) else bytes(seq)
    n = len(b)
    raw_start, raw_end = flank, n - flank - 1
    assert raw_end >= 0
    ls = max(0, raw_start - flank)
    le = max(ls, min(n, raw_start + flank + 1))
    rs = max(0, raw_end - flank)
    re_ = max(rs, min(n, raw_end + flank + 1))
    key = (lambda km: km) if fold is None else (lambda km: km.translate(fold))
    recs = set()
    for k in KS:
        left = {}
        for j in range(le - ls - k + 1):
            lp = ls + j + k
            if lp > n - 1:
                continue
            km = key(b[ls + j:ls + j + k])
            if km not in left or abs(lp - raw_start) < abs(left[km] - raw_start):
                left[km] = lp
        right = {}
        for i in range(re_ - rs - k + 1):
            rp = rs + i - 1
            if rp < 0 or rp > n - 1:
                continue
            raw = b[rs + i:rs + i + k]
            km = key(raw)
            if km not in left:
                continue
            if km not in right or abs(rp - raw_end) < abs(right[km] - raw_end):
                right[km] = rp
            ts, te = left[km], right[km]
            if k == 4:
                ok = raw == b"TTAA"
            elif k == 2:
                ok = raw == b"TA" or (plant == 0 and b[ts:ts + 3] == b"CCC" and te - 2 >= 0 and b[te - 2:te + 1] == b"GGG")
            else:
                ok = True
            if ok:
                recs.add((k, km, ts, te, raw))
    out = set()
    for k, _km, ts, te, raw in recs:
        if b"NN" in raw:
            continue
        tir = b[ts:te + 1]
        if len(tir) < 100:
            continue
        if tir[:2] == b"TG" and tir[-2:] == b"CA":
            continue
        if tir.startswith(b"TATATATA") or tir.startswith(b"ATATATAT"):
            continue
        out.add((abs(ts - raw_start) + abs(te - raw_end), ts, te, k))
    return [(k, ts, te, d) for d, ts, te, k in sorted(out)]


FOLD_OTHERS = bytes(c if c in b"ACGT" else ord("N") for c in range(256))     # every byte outside ACGT taken for one letter


def kmer_expected(seqs, flank, plant):
    """the twin's records per candidate; a candidate no longer than one flank has none (the twin refuses it, the kernel answers 0)"""
    return [O.tir_kmer(s, flank + 1, len(s) - flank, flank, plant) if len(s) > flank else [] for s in seqs]


def compare_kmer(tsd_kmer, seqs, flank, plant, label, expected=None):
    exp = kmer_expected(seqs, flank, plant) if expected is None else expected
    got = tsd_kmer(seqs, flank, plant)
    assert len(got) == len(exp), (label, len(got), len(exp))
    for c, (g, e) in enumerate(zip(got, exp)):
        if [tuple(r) for r in g] != e:
            k = next((i for i, (a, x) in enumerate(zip(g, e)) if tuple(a) != x), min(len(g), len(e)))
            raise AssertionError("%s, flank %d, plant %d, candidate %d of %d (%d bases): %d records against the twin's %d; first "
                                 "difference at %d: %s / %s" % (label, flank, plant, c, len(seqs), len(seqs[c]), len(g), len(e), k,
                                                                g[k:k + 2], e[k:k + 2]))
    return got


# ------------------------------------------------------------------------------------------------------------------------------
# k-mer seeds, group A: flanks and lengths
# ------------------------------------------------------------------------------------------------------------------------------
KMER_FLANKS = (0, 1, 2, 5, 11, 31, 32, 33, 49, 50, 51, 62, 63)
WINDOW_KINDS = ("random", "repeat", "motif", "nn")
BODIES = (99, 100, 101)                # raw_end + 1 - raw_start: on either side of the "fewer than 100 bases" filter


def windows(rng, kind, w):
    """(left, right) windows of w bases: random; the right one repeats the left one; rich in CCC / GGG / TA / TTAA; with NN"""
    if kind == "repeat":
        left = rand_seq(rng, w)
        return left, left
    if kind == "motif":
        def mix(words):
            s = ""
            while len(s) < w:
                s += words[int(rng.integers(0, len(words)))]
            return s[:w]
        return mix(("CCC", "CCCC", "TA", "TTAA", "A", "G", "T")), mix(("GGG", "GGGG", "TA", "TTAA", "A", "C", "T"))
    left, right = rand_seq(rng, w), rand_seq(rng, w)
    if kind == "nn" and w >= 6:
        for _ in range(1 + w // 16):                               # NN on both sides, in k-mers the windows share
            word = rand_seq(rng, int(rng.integers(0, 3))) + "NN" + rand_seq(rng, int(rng.integers(0, 3)))
            left = put(left, int(rng.integers(0, w - 5)), word)
            right = put(right, int(rng.integers(0, w - 5)), word)
    return left, right


def kmer_candidate(rng, flank, body, kind, plant_k=None):
    """a candidate of 2 * flank + body bases whose two windows (2 * flank + 1 bases around the raw ends) are of the kind; plant_k:
    a k-mer directly before the raw start and directly after the raw end, the record at distance 0 whose length is `body`"""
    n = 2 * flank + body
    w = min(n, 2 * flank + 1)
    left, right = windows(rng, kind, w)
    s = put(rand_seq(rng, n), 0, left)
    s = put(s, n - w, right)
    if n > flank:
        s = put(s, flank, "C")                                     # not TG.., TATATATA or ATATATAT at the raw start
    if plant_k is not None and flank >= plant_k and body >= 2:
        word = {2: "TA", 4: "TTAA"}.get(plant_k) or rand_seq(rng, plant_k)
        s = put(put(s, flank - plant_k, word), n - flank, word)
    return s


def flank_cases():
    """{(flank, plant): [(label, sequence)]}: per flank the four window kinds at the three bodies around the length filter (with a
    planted record at distance 0) and at two other bodies up to 300, and the short candidates: flank + 1 bases, between flank + 1
    and 2 * flank + 1 (the windows overlap and are clipped), and no longer than one flank (no record, the twin is not asked)"""
    def build():
        out = {}
        for f in KMER_FLANKS:
            rng = np.random.default_rng(7000 + f)
            rows = []
            for ki, kind in enumerate(WINDOW_KINDS):
                for bi, body in enumerate(BODIES):
                    k = KS[(ki * 3 + bi + f) % len(KS)]
                    rows.append(("%s body %d k %d" % (kind, body, k), kmer_candidate(rng, f, body, kind, plant_k=k)))
                for body in (int(rng.integers(0, 99)), int(rng.integers(102, 301))):
                    rows.append(("%s body %d" % (kind, body), kmer_candidate(rng, f, body, kind)))
            for n in sorted(x for x in {f + 1, f + 2, (3 * f) // 2 + 1, 2 * f - 1, 2 * f} if x > f):
                for kind in ("repeat", "motif"):
                    s = rand_seq(rng, n)
                    left, _r = windows(rng, kind, n)
                    rows.append(("short %s %d" % (kind, n), left if kind == "motif" else put(s, n // 2, s[:n - n // 2])))
            for n in sorted({0, f // 2, f}):
                rows.append(("no longer than a flank %d" % n, rand_seq(rng, n)))
            for plant in (0, 1):
                out[(f, plant)] = rows
        return out
    return cached("flank_cases", build)


def check_flank_cases():
    """the planted record at distance 0 is there exactly when the body has 100 bases or more; plant changes answers; windows of
    65 and 67 slots (flanks 32 and 33) hold records from the slots past the first pass; -> figures"""
    fig = {"cases": 0, "with records": 0, "at 100": 0, "plant matters": 0, "past the first pass": 0, "empty by length": 0}
    past = {f: 0 for f in KMER_FLANKS}
    for (f, plant), rows in flank_cases().items():
        seqs = [s for _l, s in rows]
        exp = kmer_expected(seqs, f, plant)
        other = kmer_expected(seqs, f, 1 - plant)
        for (label, s), e, o in zip(rows, exp, other):
            fig["cases"] += 1
            fig["with records"] += bool(e)
            fig["at 100"] += len(e) == TOP
            fig["plant matters"] += plant == 0 and e != o
            fig["empty by length"] += len(s) <= f
            if len(s) <= f:
                assert e == []
                continue
            n = len(s)
            rs = max(0, n - f - 1 - f)
            late = any(te + 1 - rs >= PASS_LANES for _k, _ts, te, _d in e)      # a right k-mer in window slot 64 or later
            fig["past the first pass"] += late
            past[f] += late
            if " k " in label:
                body, k = int(label.split()[2]), int(label.split()[4])
                if f >= k:
                    zero = [r for r in e if r[3] == 0 and r[0] == k]
                    assert (zero == [(k, f, n - f - 1, 0)]) == (body >= 100), (f, plant, label, zero)
            assert e == kmer_records_uncut(s, f, plant)[:TOP], (f, plant, label)
    assert fig["plant matters"] >= 5 and fig["past the first pass"] >= 20 and fig["at 100"] >= 10, fig
    assert fig["empty by length"] >= 2 * len(KMER_FLANKS)
    # 65 slots (flank 32): slot 64 is walked by the second pass but no k-mer of 2 bases or more starts there; 67 slots (flank 33): k = 2, 3 do
    assert past[32] == 0 and past[33] >= 2 and all(past[f] >= 10 for f in KMER_FLANKS if f >= 49), past
    return fig


def check_flanks(tsd_kmer, flank):
    for plant in (0, 1):
        rows = flank_cases()[(flank, plant)]
        compare_kmer(tsd_kmer, [s for _l, s in rows], flank, plant, "flank cases")


# ------------------------------------------------------------------------------------------------------------------------------
# k-mer seeds, group B: the cut at 100 records
# ------------------------------------------------------------------------------------------------------------------------------
CUT_FLANKS = (25, 50, 63)
EXACT_COUNT_SEEDS = ((100, 60, 9013), (101, 60, 9063))  # (records before the cut, flank, seed of a random candidate that has as many)


def cut_cases():
    """[(label, flank, plant, sequence)]: per flank of CUT_FLANKS a candidate whose right window repeats the left one and one whose
    windows are rich in the short motifs (several k share a start and an end there: only k orders them), body 300"""
    def build():
        out = []
        for f in CUT_FLANKS:
            rng = np.random.default_rng(7100 + f)
            for kind in ("repeat", "motif", "random"):
                for plant in (0, 1):
                    out.append(("cut %s flank %d plant %d" % (kind, f, plant), f, plant, kmer_candidate(rng, f, 300, kind)))
        return out
    return cached("cut_cases", build)


def exact_cases():
    """[(label, flank, plant, sequence, records before the cut)]: one candidate with exactly 100 records and one with 101"""
    def build():
        out = []
        for want, f, seed in EXACT_COUNT_SEEDS:
            s = kmer_candidate(np.random.default_rng(seed), f, 300, "random")
            out.append(("exactly %d records" % want, f, 1, s, want))
        return out
    return cached("exact_cases", build)


def check_cut_cases():
    """per cut case: more than 100 records before the cut, the first 100 of them are the twin's answer; per flank one case whose
    records 100 and 101 are at the same distance; one case where two of the kept records differ in k alone; -> figures"""
    figs, tie_flanks, k_alone = [], set(), 0
    for label, f, plant, s in cut_cases():
        full = kmer_records_uncut(s, f, plant)
        exp = kmer_expected([s], f, plant)[0]
        if len(full) <= TOP:
            assert exp == full, label
            figs.append((label, len(full), None, 0))
            continue
        assert exp == full[:TOP], label
        tie = full[TOP - 1][3] == full[TOP][3]
        if tie:
            tie_flanks.add(f)
        keys = [(d, ts, te) for _k, ts, te, d in full[:TOP]]
        same = len(keys) - len(set(keys))
        k_alone += same > 0
        figs.append((label, len(full), tie, same))
    over = [x for x in figs if x[1] > TOP]
    assert len(over) >= 2 * len(CUT_FLANKS), figs
    assert tie_flanks == set(CUT_FLANKS), (tie_flanks, figs)
    assert k_alone >= 1, figs
    for label, f, plant, s, want in exact_cases():
        full = kmer_records_uncut(s, f, plant)
        assert len(full) == want and kmer_expected([s], f, plant)[0] == full[:TOP], (label, len(full))
        figs.append((label, len(full), None if want == TOP else full[TOP - 1][3] == full[TOP][3], 0))
    return figs


def check_cut(tsd_kmer):
    for label, f, plant, s in cut_cases():
        compare_kmer(tsd_kmer, [s], f, plant, label)
    for label, f, plant, s, _want in exact_cases():
        compare_kmer(tsd_kmer, [s], f, plant, label)


# ------------------------------------------------------------------------------------------------------------------------------
# k-mer seeds, group C: bytes outside ACGT
# ------------------------------------------------------------------------------------------------------------------------------
# (left k-mer, right k-mer, what follows the left one, what precedes the right one): the two differ only in WHICH letter outside
# ACGT they hold.  The k = 2 pairs sit between CCC and GGG (the rule of plant == 0), their right k-mer is not NN (the filter).
ALPHABET_PAIRS = (("ACR", "ACY", "", ""), ("NN", "NR", "CCC", "GGG"), ("RY", "KM", "CCC", "GGG"), ("GATTKCAGTCA", "GATTMCAGTCA", "", ""),
                  ("SACGT", "WACGT", "", ""), ("CANTG", "CARTG", "", ""), ("TTGNCA", "TTGSCA", "", ""), ("ACGTWACG", "ACGTNACG", "", ""),
                  ("AYCGGTCAG", "AKCGGTCAG", "", ""), ("CTGAMTTGCA", "CTGANTTGCA", "", ""))
ALPHABET_FLANKS = (20, 50)


def alphabet_cases():
    """[(label, flank, plant, sequence)]: each pair alone in an ACGT candidate (left k-mer ending near the raw start, right k-mer
    starting near the raw end), all pairs in one candidate, and a candidate whose windows are random over ACGT + RYKMSWN"""
    def build():
        out = []
        for f in ALPHABET_FLANKS:
            rng = np.random.default_rng(7200 + f)
            n = 2 * f + 160
            for pi, (lk, rk, after, before) in enumerate(ALPHABET_PAIRS):
                s = rand_seq(rng, n)
                a = f - len(lk) - pi % 3
                s = put(s, a, lk + after)
                s = put(s, n - f + pi % 2 - len(before), before + rk)
                for plant in (0, 1):
                    out.append(("%s / %s flank %d plant %d" % (lk, rk, f, plant), f, plant, s))
            s = rand_seq(rng, n)
            at_l, at_r = 1, n - 2 * f
            for lk, rk, after, before in ALPHABET_PAIRS:
                if at_l + len(lk + after) > 2 * f or at_r + len(before + rk) > n - 1:
                    break
                s = put(put(s, at_l, lk + after), at_r, before + rk)
                at_l += len(lk + after) + 1
                at_r += len(before + rk) + 1
            out.append(("all pairs flank %d" % f, f, 0, s))
            w = 2 * f + 1
            s = put(put(rand_seq(rng, n), 0, rand_seq(rng, w, "ACGTRYKMSWN")), n - w, rand_seq(rng, w, "ACGTRYKMSWN"))
            out.append(("ACGTRYKMSWN windows flank %d" % f, f, 0, s))
        return out
    return cached("alphabet_cases", build)


def check_alphabet_cases():
    """the twin compares bytes: it equals the plain rule, has no record for a planted pair, and a search that takes every byte
    outside ACGT for one letter answers differently on every case but the k = 2 pairs under plant == 1; -> figures"""
    differ, cases = 0, 0
    for label, f, plant, s in alphabet_cases():
        exp = kmer_expected([s], f, plant)[0]
        assert exp == kmer_records_uncut(s, f, plant)[:TOP], label
        folded = kmer_records_uncut(s, f, plant, fold=FOLD_OTHERS)[:TOP]
        k2 = " / " in label and len(label.split()[0]) == 2
        if " / " in label:
            lk, rk = label.split()[0], label.split()[2]
            lp, rp = s.index(lk) + len(lk), s.rindex(rk) - 1
            assert not any(r[0] == len(lk) and r[1] == lp and r[2] == rp for r in exp), label
            if not (k2 and plant == 1):
                assert any(r[0] == len(lk) and r[1] == lp and r[2] == rp for r in kmer_records_uncut(s, f, plant, fold=FOLD_OTHERS)), label
        if not (k2 and plant == 1):
            assert folded != exp, label
        differ += folded != exp
        cases += 1
    return {"cases": cases, "a folding search differs on": differ}


def check_alphabet(tsd_kmer):
    for label, f, plant, s in alphabet_cases():
        compare_kmer(tsd_kmer, [s], f, plant, "alphabet: " + label)


# ------------------------------------------------------------------------------------------------------------------------------
# k-mer seeds, group D: batch independence and guards
# ------------------------------------------------------------------------------------------------------------------------------
def mixed_batch():
    """flank 50: empty, too short, cut, exact and ordinary candidates in one batch"""
    def build():
        rows = [("empty", ""), ("one base", "A"), ("a flank", "ACGT" * 12 + "AC")]
        rows += [(l, s) for l, f, p, s in cut_cases() if f == 50 and p == 1]
        rows += [(l, s) for l, f, p, s, _w in exact_cases()]
        rows += [(l, s) for l, s in flank_cases()[(50, 1)] if "body" in l]
        return rows
    return cached("mixed_batch", build)


def check_batch_independence(tsd_kmer):
    rows = mixed_batch()
    seqs = [s for _l, s in rows]
    exp = kmer_expected(seqs, 50, 1)
    assert sum(len(e) == TOP for e in exp) >= 3 and sum(e == [] for e in exp) >= 3 and sum(0 < len(e) < TOP for e in exp) >= 3
    first = compare_kmer(tsd_kmer, seqs, 50, 1, "mixed batch", exp)
    for name, perm in (("reversed", list(range(len(seqs)))[::-1]), ("shuffled", np.random.default_rng(73).permutation(len(seqs)).tolist())):
        got = compare_kmer(tsd_kmer, [seqs[i] for i in perm], 50, 1, "mixed batch " + name, [exp[i] for i in perm])
        assert all(got[j] == first[i] for j, i in enumerate(perm)), name


def check_kmer_guards(tsd_kmer):
    """flank 64 and flank -1 are errors, an empty batch an empty list; the same callable then answers"""
    s = [mixed_batch()[-1][1]]
    assert raises(lambda: tsd_kmer(s, 64, 1)), "flank 64 did not raise"
    assert raises(lambda: tsd_kmer(s, -1, 1)), "flank -1 did not raise"
    assert tsd_kmer([], 50, 1) == []
    compare_kmer(tsd_kmer, s, 50, 1, "after the refused calls")
    compare_kmer(tsd_kmer, s, 63, 0, "flank 63 after the refused calls")


# ------------------------------------------------------------------------------------------------------------------------------
# non-LTR preparation: comparison
# ------------------------------------------------------------------------------------------------------------------------------
def nonltr_expected(seqs, flank, win5):
    return O.nonltr_prep(seqs, flank, win5)


def compare_nonltr(nonltr_prep, seqs, flank, win5, label, expected=None):
    exp = nonltr_expected(seqs, flank, win5) if expected is None else expected
    got = nonltr_prep(seqs, flank, win5)
    assert len(got) == len(exp), (label, len(got), len(exp))
    bad = [i for i, (g, e) in enumerate(zip(got, exp)) if tuple(g) != tuple(e)]
    if bad:
        i = bad[0]
        raise AssertionError("%s, flank %d, win5 %d: %d of %d differ from the twin; first: candidate %d (%d bases) %s against %s"
                             % (label, flank, win5, len(bad), len(seqs), i, len(seqs[i]), tuple(got[i]), tuple(exp[i])))
    return got


def plain(rng, n, first=None, last=None):
    """n random bases without a run of three equal bases and without a unit of 2..6 bases directly repeated: nothing a poly-A /
    poly-T / tandem search takes; first / last: letters the ends must not be"""
    while True:
        s = ""
        while len(s) < n:
            ok = [c for c in BASES if not (s[-2:] == c + c or any((s + c)[-m:] == (s + c)[-2 * m:-m] for m in range(2, 7)))
                  and not (first and not s and c in first) and not (last and len(s) == n - 1 and c in last)]
            if not ok:
                break
            s += ok[int(rng.integers(0, len(ok)))]
        if len(s) == n:
            return s


# ------------------------------------------------------------------------------------------------------------------------------
# non-LTR preparation, group E: the closed form np_near1
# ------------------------------------------------------------------------------------------------------------------------------
NEAR_FLANK = 26            # the windows around the two raw ends do not reach each other's runs
NEAR_BODY = 40
POLY_RUN = 13              # poly-A / poly-T run: the longest tandem inside it has 12 bases, the poly end wins


def near_layout(seed=81):
    rng = np.random.default_rng(seed)
    return {"left": plain(rng, NEAR_FLANK), "body": plain(rng, NEAR_BODY, first="T", last="AT"), "right": plain(rng, NEAR_FLANK + 8, first="ACG")}


def near_plus(tsd, kmer, win5, lay, stop=False):
    """poly-A candidate: left flank + body + A-run + TSD + right flank, flank NEAR_FLANK; the 5' window [flank + 1 - win5,
    flank + 1 + win5) starts with `kmer`.  stop: an N directly after the TSD, so that no longer TSD counts.
    -> (sequence, where the TSD starts)"""
    k = len(tsd)
    tail = tsd + ("N" if stop else "") + lay["right"]
    s = lay["left"] + lay["body"] + "A" * POLY_RUN + tail[:NEAR_FLANK]
    return put(s, NEAR_FLANK + 1 - win5, kmer), NEAR_FLANK + NEAR_BODY + POLY_RUN


def near_minus(tsd, kmer, win5, lay):
    """the mirror: left flank ending with the TSD + T-run + body + right flank; the 5' window [L - flank - win5, L - flank + win5)
    starts with `kmer`"""
    s = put(lay["left"], NEAR_FLANK - len(tsd), tsd) + "T" * POLY_RUN + lay["body"][::-1] + lay["right"][:NEAR_FLANK]
    return put(s, len(s) - NEAR_FLANK - win5, kmer), NEAR_FLANK - len(tsd)


def all_8mers(letters="CG"):
    return ["".join(letters[(v >> (7 - i)) & 1] for i in range(8)) for v in range(256)]


def exhaustive_plus():
    """all 65 536 (TSD, k-mer) pairs of 8-mers over C / G, win5 = 4: the 5' window has 8 bases, only k = 8 has a position in it"""
    def build():
        lay, w = near_layout(), all_8mers()
        rows = [near_plus(p, t, 4, lay) for p in w for t in w]
        return [s for s, _a in rows], rows[0][1]
    return cached("exhaustive_plus", build)


def exhaustive_minus():
    """the poly-T mirror for 4 096 of the pairs (seeded choice)"""
    def build():
        lay, w = near_layout(), all_8mers()
        pick = np.sort(np.random.default_rng(82).choice(65536, size=4096, replace=False))
        rows = [near_minus(w[v >> 8], w[v & 255], 4, lay) for v in pick.tolist()]
        return [s for s, _a in rows], rows[0][1]
    return cached("exhaustive_minus", build)


def near1_model(p, t):
    """some substring of t within one edit of p, both of length k: common prefix + common suffix >= k - 1 for t itself, for t
    without its last and for t without its first character"""
    k = len(p)

    def pre(a, b):
        i = 0
        while i < min(len(a), len(b)) and a[i] == b[i]:
            i += 1
        return i
    lp, ls = pre(p, t), pre(p[::-1], t[::-1])
    if lp == k or lp + ls >= k - 1:
        return True
    if lp + pre(p[::-1], t[:k - 1][::-1]) >= k - 1:
        return True
    return pre(p, t[1:]) + ls >= k - 1


def exhaustive_expected(name):
    seqs, _at = exhaustive_plus() if name == "poly-A" else exhaustive_minus()
    return cached(("exhaustive expected", name), lambda: nonltr_expected(seqs, NEAR_FLANK, 4))


def check_exhaustive_cases():
    """every one of the 65 536 has direct == 1 and, where found, the TSD at the planted place with 8 bases; found is the closed form;
    the mirror has direct == 2; -> figures"""
    fig, found = {}, {}
    for name, (seqs, at), direct in (("poly-A", exhaustive_plus(), 1), ("poly-T", exhaustive_minus(), 2)):
        e = np.asarray(exhaustive_expected(name), dtype=np.int64)
        assert (e[:, 1] == direct).all(), (name, int((e[:, 1] != direct).sum()))
        f = found[name] = e[:, 0] == 1
        assert (e[f, 2] == at).all() and (e[f, 3] == 8).all() and (e[~f, 3] == 0).all(), name
        fig[name] = (len(seqs), int(f.sum()))
    w = all_8mers()
    model = np.asarray([near1_model(p, t) for p in w for t in w])
    assert (model == found["poly-A"]).all()
    assert fig["poly-A"] == (65536, 5324), fig
    assert 100 < fig["poly-T"][1] < 4096
    return fig


def check_exhaustive(nonltr_prep):
    for name, (seqs, _at) in (("poly-A", exhaustive_plus()), ("poly-T", exhaustive_minus())):
        compare_nonltr(nonltr_prep, seqs, NEAR_FLANK, 4, "all pairs of 8-mers, " + name, exhaustive_expected(name))


def edit_family(rng, p):
    """strings of len(p) bases one edit from p: every substitution; every deletion, padded at either end; every insertion, cut at
    either end; and each of these with one more substitution"""
    k, out = len(p), []
    other = lambda c: BASES[(BASES.index(c) + 1 + int(rng.integers(0, 3))) % 4]  # noqa: E731
    for i in range(k):
        for c in BASES:
            if c != p[i]:
                out.append(p[:i] + c + p[i + 1:])
        d = p[:i] + p[i + 1:]
        out += [d + BASES[int(rng.integers(0, 4))], BASES[int(rng.integers(0, 4))] + d]
    for i in range(k + 1):
        for c in BASES:
            ins = p[:i] + c + p[i:]
            out += [ins[:k], ins[1:]]
    more = []
    for t in out:
        i = int(rng.integers(0, k))
        more.append(t[:i] + other(t[i]) + t[i + 1:])
    return [p] + out + more


def family_cases():
    """{k: (win5, [sequence], TSD start)} for k = 9..20: one random TSD (not starting with A, which would lengthen the run) against
    its family, win5 = ceil(k / 2): k has one (even k) or two (odd k) places in the window; an N after the TSD stops longer ones"""
    def build():
        lay, out = near_layout(), {}
        for k in range(9, 21):
            rng = np.random.default_rng(8300 + k)
            p = plain(rng, k, first="A")
            win5 = (k + 1) // 2
            rows = [near_plus(p, t, win5, lay, stop=True) for t in edit_family(rng, p)]
            out[k] = (win5, [s for s, _a in rows], rows[0][1])
        return out
    return cached("family_cases", build)


def check_family_cases():
    fig = {}
    for k, (win5, seqs, at) in family_cases().items():
        e = np.asarray(nonltr_expected(seqs, NEAR_FLANK, win5), dtype=np.int64)
        assert (e[:, 1] == 1).all(), k
        f = e[:, 0] == 1
        assert (e[f, 2] == at).all() and (e[f, 3] <= k).all() and e[0, 3] == k, k
        at_k, below = int((e[:, 3] == k).sum()), int((f & (e[:, 3] < k)).sum())
        assert at_k >= 6 * k and int((~f).sum()) >= k, (k, at_k, int((~f).sum()))
        fig[k] = (len(seqs), at_k, below, int((~f).sum()))
    assert 2000 <= sum(v[0] for v in fig.values()) <= 9000
    return fig


def check_family(nonltr_prep):
    for k, (win5, seqs, _at) in family_cases().items():
        compare_nonltr(nonltr_prep, seqs, NEAR_FLANK, win5, "edit family k = %d" % k)


def tie_cases():
    """[(sequence, direct, where the first run ends (poly-A) or starts (poly-T))]: two runs of equal length, 9..11 bases and 1 or 3
    bases apart, in the window of the poly-A or the poly-T search: the first one counts"""
    def build():
        lay, f, out = near_layout(), NEAR_FLANK, []
        rng = np.random.default_rng(84)
        for r in (9, 10, 11):
            for gap in (1, 3):
                s = lay["left"] + plain(rng, 60) + lay["right"][:f]
                a2 = len(s) - f - r
                a1 = a2 - gap - r
                s = put(put(put(put(s, a1 - 1, "C"), a1, "A" * r), a1 + r, "C" * gap), a2, "A" * r)
                out.append((s, 1, a1 + r))
                s = lay["left"] + plain(rng, 60) + lay["right"][:f]
                s = put(put(put(put(put(s, f - 1, "C"), f, "T" * r), f + r, "C" * gap), f + r + gap, "T" * r), f + 2 * r + gap, "C")
                out.append((s, 2, f))
        return out
    return cached("tie_cases", build)


def check_tie_cases():
    exp = nonltr_expected([s for s, _d, _at in tie_cases()], NEAR_FLANK, 4)
    for (s, direct, at), (found, d, _ts, _tn, lo, hi) in zip(tie_cases(), exp):
        assert (found, d) == (0, direct) and (hi if direct == 1 else lo) == at, (direct, at, lo, hi)
    return len(exp)


def check_ties(nonltr_prep):
    compare_nonltr(nonltr_prep, [s for s, _d, _at in tie_cases()], NEAR_FLANK, 4, "two equal runs")


# ------------------------------------------------------------------------------------------------------------------------------
# non-LTR preparation, group F: the wrapped 5' window (second round of 64 lanes)
# ------------------------------------------------------------------------------------------------------------------------------
WRAP_PARAMS = ((100, 0), (100, 5), (120, 10), (90, 0))


def wrapped_cases():
    """{(flank, win5): [(sequence, L, T-run start, N bytes)]}: L in [flank - 16, flank - win5): raw_end = L - flank is negative and
    raw_end + win5 too, so the python slice of the 5' window wraps to [0, 2 L - flank + win5).  A T-run of 8..13 bases starts
    0..5 bases into the window of the poly-T search (flank - 24), the TSDs end where it starts -- and match THEMSELVES in the 5'
    window where that reaches so far; 0..13 N bytes from 20 bases before the run take the longer TSDs out."""
    def build():
        out = {}
        for f, w in WRAP_PARAMS:
            rng = np.random.default_rng(8400 + f + w)
            rows = []
            for L in range(f - 16, f - w):
                for rep in range(4):
                    j, run, nn = int(rng.integers(0, 6)), int(rng.integers(8, 14)), int(rng.integers(0, 14))
                    if (L + rep) % 3 == 0:
                        nn = int(rng.integers(8, 13))
                    t0 = f - 24 + j
                    s = plain(rng, L)
                    s = put(s, t0, "T" * run)
                    if t0 + run < L and s[t0 + run] == "T":
                        s = put(s, t0 + run, "G")
                    if s[t0 - 1] == "T":
                        s = put(s, t0 - 1, "C")
                    s = put(s, t0 - 20, "N" * nn)
                    rows.append((s, L, t0, nn))
            out[(f, w)] = rows
        return out
    return cached("wrapped_cases", build)


def check_wrapped_cases():
    """at least a quarter of the cases are found at a window index of 64 or more, some below 64, some not at all; -> figures"""
    fig = {"cases": 0, "direct 2": 0, "found": 0, "index >= 64": 0, "index < 64": 0, "not found": 0}
    for (f, w), rows in wrapped_cases().items():
        exp = nonltr_expected([r[0] for r in rows], f, w)
        for (s, L, t0, nn), (found, direct, ts, tn, lo, hi) in zip(rows, exp):
            assert L - f < 0 and L - f + w < 0
            fig["cases"] += 1
            fig["direct 2"] += direct == 2
            if found:
                assert direct == 2 and ts + tn == t0
                # end_5 = 0 + index of the first match; end_3 = t0: [lo, hi) = [index, t0)
                assert hi == t0 and 0 <= lo < t0
                fig["found"] += 1
                fig["index >= 64" if lo >= PASS_LANES else "index < 64"] += 1
            else:
                fig["not found"] += 1
    assert 4 * fig["index >= 64"] >= fig["cases"] and fig["index < 64"] >= 10 and fig["not found"] >= 10, fig
    return fig


def check_wrapped(nonltr_prep):
    for (f, w), rows in wrapped_cases().items():
        compare_nonltr(nonltr_prep, [r[0] for r in rows], f, w, "wrapped window")


# ------------------------------------------------------------------------------------------------------------------------------
# non-LTR preparation, group G: short sequences and parameters
# ------------------------------------------------------------------------------------------------------------------------------
GRID_FLANKS = (0, 1, 10, 24, 25, 26, 50, 63, 100)
GRID_WIN5 = (0, 1, 4, 10, 24, 25)
GRID_L = tuple(range(80)) + (99, 100, 101, 125, 150, 201, 260)
TANDEM_UNITS = ("CA", "TTG", "GAAT", "ACGTC", "GATTCA")


def grid_sequence(rng, L, flank, variant):
    """variant 0: an A-run (or a tandem) ending at the raw end L - flank and a copy of the bases after it around the raw start;
    1: a T-run (or a tandem) starting at the raw start and a copy of the bases before it around the raw end; 2: runs and tandems
    at random places.  Sequences no longer than a flank have the runs where the searches then look."""
    s = rand_seq(rng, L)
    if L < 8:
        return put(s, 0, "A" * int(rng.integers(0, L + 1)))
    unit = TANDEM_UNITS[int(rng.integers(0, len(TANDEM_UNITS)))]
    run = unit * int(rng.integers(4, 7)) if rng.integers(0, 4) == 0 else None
    k = int(rng.integers(8, 21))
    if variant == 0:
        tail = run or "A" * int(rng.integers(5, 18))
        # L <= flank: the raw end is before the sequence and the poly-A search looks at its first bases (its slice wraps)
        end = L - flank if L > flank else (len(tail) + int(rng.integers(0, 3)) if rng.integers(0, 4) else int(rng.integers(6, L + 1)))
        s = put(s, end - len(tail), tail)
        tsd = s[end:end + k]
        if len(tsd) >= 8:
            word = tsd if rng.integers(0, 3) else put(tsd, int(rng.integers(0, len(tsd))), "C")
            s = put(s, min(L, flank + 1) - len(word) - int(rng.integers(0, 6)), word)
    elif variant == 1:
        # L <= flank: the poly-T search looks at [flank - 24, L)
        start = flank if L > flank else (max(0, flank - 24) + int(rng.integers(0, 3)) if rng.integers(0, 4) else int(rng.integers(0, max(1, L - 6))))
        head = run or "T" * int(rng.integers(5, 18))
        s = put(s, start, head)
        tsd = s[max(0, start - k):start]
        if len(tsd) >= 8:
            word = tsd if rng.integers(0, 3) else put(tsd, int(rng.integers(0, len(tsd))), "G")
            s = put(s, max(0, L - flank) + int(rng.integers(0, 6)), word)
    else:
        for _ in range(int(rng.integers(1, 4))):
            piece = ("A" * int(rng.integers(6, 15)), "T" * int(rng.integers(6, 15)), unit * 4, "N" * int(rng.integers(1, 4)))[int(rng.integers(0, 4))]
            s = put(s, int(rng.integers(0, L)), piece)
    return s[:L]


def grid_cases():
    """{(flank, win5): [sequence]}: every flank x win5 x L of the grid x three variants"""
    def build():
        out = {}
        for f in GRID_FLANKS:
            for w in GRID_WIN5:
                rng = np.random.default_rng(8500 + 100 * f + w)
                out[(f, w)] = [grid_sequence(rng, L, f, v) for L in GRID_L for v in range(3)]
        return out
    return cached("grid_cases", build)


def skipped_search_cases():
    """[(flank, sequence)]: L = flank - 1 with a T-run at the very end: direct == 2 with end_5 == raw_end == -1, the value that
    means "no 5' end": the TSD search is skipped although with win5 = 0 the wrapped window [0, L - 1) holds the TSD itself"""
    def build():
        out = []
        for f in (24, 25, 26, 50, 63, 100):
            rng = np.random.default_rng(8600 + f)
            L = f - 1
            s = put(plain(rng, L, last="T"), L - 10, "T" * 10)
            if s[L - 11] == "T":
                s = put(s, L - 11, "C")
            out.append((f, s))
        return out
    return cached("skipped", build)


def check_grid_cases():
    fig = {"cases": 0, "direct 1": 0, "direct 2": 0, "found": 0, "below one flank": 0}
    for (f, w), seqs in grid_cases().items():
        exp = nonltr_expected(seqs, f, w)
        assert len(seqs) == 3 * len(GRID_L)
        per = {"d": 0, "f": 0}
        for s, (found, direct, ts, tn, lo, hi) in zip(seqs, exp):
            fig["cases"] += 1
            fig["direct 1"] += direct == 1
            fig["direct 2"] += direct == 2
            fig["found"] += found
            fig["below one flank"] += len(s) < f
            per["d"] += direct != 0
            assert 0 <= lo <= hi <= len(s) and (not found or (8 <= tn <= 20 and 0 <= ts and ts + tn <= len(s)))
        assert per["d"] >= 3, (f, w, per)                         # every flank x win5 has cases with a direction
    assert fig["cases"] == len(GRID_FLANKS) * len(GRID_WIN5) * len(GRID_L) * 3 == 14094
    assert fig["direct 1"] >= 500 and fig["direct 2"] >= 500 and fig["found"] >= 200 and fig["below one flank"] >= 3000, fig
    for f, s in skipped_search_cases():
        found, direct, ts, tn, lo, hi = nonltr_expected([s], f, 0)[0]
        t0 = len(s) - 10
        assert (found, direct) == (0, 2) and "N" not in s and t0 <= len(s) - 1, (f, found, direct)
        # one base fewer: end_5 == -2, the search runs, and its wrapped window [0, L - 4) holds the TSD itself
        assert nonltr_expected([s[1:]], f, 0)[0][:2] == (1, 2), f
    fig["search skipped at end_5 == -1"] = len(skipped_search_cases())
    return fig


def check_grid(nonltr_prep):
    for (f, w), seqs in grid_cases().items():
        compare_nonltr(nonltr_prep, seqs, f, w, "short sequences")
    for f, s in skipped_search_cases():
        compare_nonltr(nonltr_prep, [s, s[1:]], f, 0, "L = flank - 1")


# ------------------------------------------------------------------------------------------------------------------------------
# non-LTR preparation, group H: block tail and guards
# ------------------------------------------------------------------------------------------------------------------------------
BATCHES = (1, 3, 4, 5, 257)


def batch_pool():
    """257 candidates at flank 50, win5 25 with both directions, found and not found, in every residue of the block of four"""
    def build():
        rng = np.random.default_rng(8700)
        seqs = []
        for i in range(max(BATCHES)):
            L = int(rng.integers(130, 260))
            s = grid_sequence(rng, L, 50, i % 2)
            seqs.append(s)
        return seqs
    return cached("batch_pool", build)


def check_batch_cases():
    exp = nonltr_expected(batch_pool(), 50, 25)
    tail = exp[-5:]
    assert sum(e[1] == 1 for e in exp) >= 60 and sum(e[1] == 2 for e in exp) >= 60 and sum(e[0] for e in exp) >= 40
    assert any(e[1] for e in tail)
    return {"candidates": len(exp), "direct": sum(e[1] != 0 for e in exp), "found": sum(e[0] for e in exp)}


def check_batches(nonltr_prep):
    pool = batch_pool()
    exp = nonltr_expected(pool, 50, 25)
    for n in BATCHES:
        seqs = pool[len(pool) - n:]
        compare_nonltr(nonltr_prep, seqs, 50, 25, "batch of %d" % n, exp[len(pool) - n:])
    assert nonltr_prep([], 50, 25) == []


def check_nonltr_guards(nonltr_prep):
    """win5 of 26 or -1 and flank -1 are errors; the same callable then answers"""
    s = batch_pool()[:3]
    assert raises(lambda: nonltr_prep(s, 50, 26)), "win5 26 did not raise"
    assert raises(lambda: nonltr_prep(s, 50, -1)), "win5 -1 did not raise"
    assert raises(lambda: nonltr_prep(s, -1, 25)), "flank -1 did not raise"
    compare_nonltr(nonltr_prep, s, 50, 25, "after the refused calls")


# ------------------------------------------------------------------------------------------------------------------------------
# a thinned set of the small cases for a fixture recorded from the reference's own python (oracle/gen_golden.py: gen_tsd_limits)
# ------------------------------------------------------------------------------------------------------------------------------
def fixture_cases():
    """[record without results]: kind "kmer" (seq, flank, plant) or "nonltr" (seq, flank, win5), each with a label of its own"""
    def build():
        out = []

        def kmer(label, s, f, plant):
            if len(s) > f:                                         # (the reference is never called with a raw end before the sequence)
                out.append({"kind": "kmer", "label": "%s [%d]" % (label, len(out)), "seq": s, "flank": f, "plant": plant})

        def nonltr(label, s, f, w):
            out.append({"kind": "nonltr", "label": "%s [%d]" % (label, len(out)), "seq": s, "flank": f, "win5": w})
        n = 0
        for (f, plant), rows in flank_cases().items():
            for label, s in rows:
                n += 1
                if n % 6 == 0:
                    kmer("flank %d plant %d %s" % (f, plant, label), s, f, plant)
        for label, f, plant, s in cut_cases() + [r[:4] for r in exact_cases()] + alphabet_cases():
            kmer(label, s, f, plant)
        seqs, _at = exhaustive_plus()
        found = [i for i, e in enumerate(exhaustive_expected("poly-A")) if e[0]]
        for i in sorted(set(range(0, len(seqs), 1024)) | set(found[::100])):
            nonltr("8-mer pair %d poly-A" % i, seqs[i], NEAR_FLANK, 4)
        seqs, _at = exhaustive_minus()
        for i in range(0, len(seqs), 128):
            nonltr("8-mer pair %d poly-T" % i, seqs[i], NEAR_FLANK, 4)
        for k, (w, seqs, _at) in family_cases().items():
            for i in range(k % 7, len(seqs), 100):
                nonltr("edit family k %d" % k, seqs[i], NEAR_FLANK, w)
        for s, _d, _at in tie_cases():
            nonltr("two equal runs", s, NEAR_FLANK, 4)
        for (f, w), rows in wrapped_cases().items():
            for s, _L, _t0, _nn in rows[::3]:
                nonltr("wrapped window", s, f, w)
        n = 0
        for (f, w), seqs in grid_cases().items():
            for s in seqs:
                n += 1
                if n % 97 == 0:
                    nonltr("short", s, f, w)
        for f, s in skipped_search_cases():
            nonltr("L = flank - 1", s, f, 0)
            nonltr("L = flank - 2", s[1:], f, 0)
        return out
    return cached("fixture_cases", build)


def kmer_items(seq, recs):
    """records -> the canonical multiset [distance, TSD, sequence] the reference's names and values carry"""
    return sorted([d, seq[ts - k:ts], seq[ts:te + 1]] for (k, ts, te, d) in recs)


def fixture_kmer_result(items):
    """what the fixture keeps of the reference's answer: below 100 records all of them; at the cut only those closer than the
    farthest kept one (the reference's pick among equal distances follows PYTHONHASHSEED)"""
    items = sorted(items)
    n = len(items)
    if n >= TOP:
        items = [x for x in items if x[0] < items[-1][0]]
    return {"n": n, "items": items}


def nonltr_as_reference(seq, six):
    """the six numbers -> (found_TSD, TSD_seq, non_ltr_seq) as the reference returns them"""
    found, direct, ts, tn, lo, hi = six
    nl = seq[lo:hi] if direct else ""
    if direct == 2:
        comp = {"A": "T", "T": "A", "C": "G", "G": "C"}
        nl = "".join(comp.get(c, "N") for c in reversed(nl))
    return [bool(found), seq[ts:ts + tn] if found else "", nl]


def check_fixture(tsd_kmer, nonltr_prep, records):
    """the recorded inputs are today's cases, and the callables give what the reference gave"""
    today = fixture_cases()
    assert [r["label"] for r in records] == [c["label"] for c in today]
    groups = {}
    for rec, c in zip(records, today):
        assert all(rec[key] == c[key] for key in c), rec["label"]
        key = (rec["kind"], rec["flank"], rec["plant"] if rec["kind"] == "kmer" else rec["win5"])
        groups.setdefault(key, []).append(rec)
    for (kind, f, x), recs in groups.items():
        seqs = [r["seq"] for r in recs]
        if kind == "kmer":
            for r, got in zip(recs, tsd_kmer(seqs, f, x)):
                items = kmer_items(r["seq"], got)
                assert len(items) == r["n"], (r["label"], len(items), r["n"])
                if r["n"] < TOP:
                    assert items == r["items"], r["label"]
                else:
                    dcut = items[-1][0]
                    assert [i for i in items if i[0] < dcut] == r["items"], r["label"]
        else:
            for r, got in zip(recs, nonltr_prep(seqs, f, x)):
                assert nonltr_as_reference(r["seq"], got) == [r["found"], r["tsd"], r["non_ltr"]], (r["label"], tuple(got))
