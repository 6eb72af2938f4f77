"""TEST INFRASTRUCTURE: labelled inputs of the LTR candidate scan (hite_ltr_scan; include/hite_gpu.h, "LTR candidate scan"), the
smallest at which each step of the definition can go wrong, each with a closed-form expectation where one exists.  A case is a dict:
label, seqs, kw (the limits), records (the closed form of the result, or None) and stats (the closed form of some counters, or None).
tests/test_ltrscan_cases.py holds the twin to the closed forms and the two forms of the twin to each other; tests/test_gpu_ltrscan.py
holds the HIP code to the twin on every case."""
import functools

import numpy as np

import ltrscan_twin as LT

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
SMALL = dict(min_len=100, max_len=4000, min_ltr=100, max_ltr=1000, identity=85)
PLAN = [("clean", 12), ("recomb", 3), ("nested", 3), ("overhang", 3), ("shifted", 3), ("dirty", 3), ("dup", 2)]


def rand(rng, n):
    return rng.integers(0, 4, size=int(n)).astype(np.uint8)


def text(*parts):
    return b"".join(ACGT[p].tobytes() if isinstance(p, np.ndarray) else p for p in parts).decode()


def guard(rng, pair, n=12):
    """n bases from a two-letter alphabet: next to the first copy from {A, C}, next to the second from {G, T}, so that no alignment
    of the two copies goes on into them"""
    return np.array(pair, dtype=np.uint8)[rng.integers(0, 2, size=n)]


def subs(codes, positions):
    s = codes.copy()
    s[list(positions)] = (s[list(positions)] + 1) & 3
    return s


def element(rng, left, right, internal, lead=300, tail=300):
    """random lead | guard | left | guard | internal | guard | right | guard | random tail -> (text, ls, le, rs, re)"""
    parts = [rand(rng, lead), guard(rng, (0, 1)), left, guard(rng, (0, 1)), rand(rng, internal), guard(rng, (2, 3)), right, guard(rng, (2, 3)),
             rand(rng, tail)]
    at = np.cumsum([0] + [len(p) for p in parts])
    return text(*parts), int(at[2]), int(at[3]), int(at[6]), int(at[7])


def case(label, seqs, kw=None, records=None, stats=None):
    return dict(label=label, seqs=list(seqs), kw=dict(kw or SMALL), records=records, stats=stats)


def exact(rng, L, internal, label, kw=None, lead=300, tail=300, keep=True, stats=None):
    """an exact repeat of L bases between guards: one record with every base matched (both lattices find it), or none"""
    r = rand(rng, L)
    s, ls, le, rs, re_ = element(rng, r, r, internal, lead, tail)
    return case(label, [s], kw, [(0, ls, le, rs, re_, 2 * L, L, L)] if keep else [], stats)


# ---- sequences -------------------------------------------------------------------------------------------------------------------
def sequences():
    rng = np.random.default_rng(101)
    out = [case("no sequence", [], None, [], dict(words=0, hits=0, records=0)),
           case("empty sequences", ["", ""], None, [], dict(words=0)),
           case("12 and 13 bases", ["ACGTTGCAAGCT", "ACGTTGCAAGCTA", ""], None, [], dict(words=1, hits=0)),
           case("a word with another byte at each place", ["ACGTTGNAAGCTA", "NACGTTGCAAGCTAN", "ACGTTGCAAGCT-"], None, [], dict(words=1))]
    r = rand(rng, 300)
    a, b = text(rand(rng, 400), r, rand(rng, 50)), text(rand(rng, 80), r, rand(rng, 400))
    out.append(case("the second copy in the next sequence", [a, b], None, [], dict(words=738 + 768, hits=0)))
    out.append(case("both copies in the second sequence", [a, text(guard(rng, (0, 1)), r, guard(rng, (0, 1)), rand(rng, 500), guard(rng, (2, 3)), r,
                                                                   guard(rng, (2, 3)))], None, [(1, 12, 312, 836, 1136, 600, 300, 300)]))
    r = rand(rng, 200)
    s = text(r, guard(rng, (0, 1)), rand(rng, 576), guard(rng, (2, 3)), r)
    out.append(case("a repeat at the first and the last position of its sequence", [s], None, [(0, 0, 200, 800, 1000, 400, 200, 200)],
                    dict(hits=188, runs=2, alignments=2, redos=0)))
    out.append(case("the same between two other sequences", [text(rand(rng, 100)), s, text(rand(rng, 40))], None,
                    [(1, 0, 200, 800, 1000, 400, 200, 200)], dict(hits=188)))
    return out


# ---- links -----------------------------------------------------------------------------------------------------------------------
def _two_copies(rng, r, d, lead=200, tail=200):
    """r twice, the second copy d after the first, between guards"""
    return text(rand(rng, lead), guard(rng, (0, 1)), r, guard(rng, (0, 1)), rand(rng, d - len(r) - 24), guard(rng, (2, 3)), r, guard(rng, (2, 3)),
                rand(rng, tail))


def links():
    rng = np.random.default_rng(102)
    kw = dict(min_len=100, max_len=1000, min_ltr=200, max_ltr=1000, identity=85)       # dmin 200, dmax 800
    out = []
    for d, hits in ((199, 0), (200, 48), (800, 48), (801, 0)):
        out.append(case("a word and its copy %d apart (dmin 200, dmax 800)" % d, [_two_copies(rng, rand(rng, 60), d)], kw, [], dict(hits=hits)))
    # T copies of a word 14 apart, one more 500 after the first: with dmin 495 only the first copy can link to it, and does when no
    # more than HITE_LTRSCAN_MAX_OCC - 1 copies lie between
    kw2 = dict(min_len=100, max_len=4000, min_ltr=495, max_ltr=1000, identity=85)
    w = rand(rng, 13)
    for T, hits in ((16, 1), (17, 0)):
        unit = np.concatenate([w, [(w[0] + 1) & 3]]).astype(np.uint8)
        tandem = np.tile(unit, T)
        lead = np.concatenate([rand(rng, 100), guard(rng, (0, 1))])
        fill = rand(rng, 500 - len(tandem))
        s = text(lead, tandem, fill, w, guard(rng, (2, 3)), rand(rng, 100))
        out.append(case("%d nearer copies before the one that qualifies" % (T - 1), [s], kw2, [], dict(hits=hits)))
    r = rand(rng, 150)
    s, ls, le, rs, re_ = element(rng, r, r, 500)
    out.append(case("lower case", [s.lower()], None, [(0, ls, le, rs, re_, 300, 150, 150)]))
    out.append(case("mixed case", [s[:700].lower() + s[700:]], None, [(0, ls, le, rs, re_, 300, 150, 150)]))
    sn = s[:ls + 50] + "N" + s[ls + 51:]
    out.append(case("an N inside the first copy", [sn], None, [(0, ls, le, rs, re_, 2 * 149 - 4, 149, 150)], dict(words=len(s) - 12 - 13, hits=138 - 13)))
    sn = s[:ls + 50] + "n" + s[ls + 51:rs + 50] + "N" + s[rs + 51:]
    out.append(case("an N at the same place of both copies", [sn], None, [(0, ls, le, rs, re_, 2 * 149 - 4, 149, 150)], dict(hits=138 - 13)))
    return out


# ---- runs ------------------------------------------------------------------------------------------------------------------------
def _islands(rng, sizes, gaps1, gaps2, d0, lead=150, tail=150):
    """exact shared islands (sizes) in two copies: gaps1 / gaps2 unrelated bases between them in the first / second copy, the first
    island of the second copy d0 after that of the first; the first and the last base of a gap differ between the copies and guards
    lie around the copies, so that an island is shared exactly"""
    isl = [rand(rng, k) for k in sizes]
    c1, c2 = [isl[0]], [isl[0]]
    for k in range(1, len(isl)):
        g1, g2 = rand(rng, gaps1[k - 1]), rand(rng, gaps2[k - 1])
        g2[0], g2[-1] = (g1[0] + 1) & 3, (g1[-1] + 1) & 3
        c1 += [g1, isl[k]]
        c2 += [g2, isl[k]]
    mid = rand(rng, d0 - sum(len(p) for p in c1) - 24)
    return text(rand(rng, lead), guard(rng, (0, 1)), *c1, guard(rng, (0, 1)), mid, guard(rng, (2, 3)), *c2, guard(rng, (2, 3)), rand(rng, tail))


def runs():
    rng = np.random.default_rng(103)
    out = []
    # two islands of 14 bases (two hits each): the first on diagonal 992, the second 63 / 64 further.  992 and 1055 share a bin of
    # lattice 32 only; 992 and 1056 share none: one run of four hits (too short for an HSP), or none
    for drift, st in ((63, dict(hits=4, runs=1, alignments=1, no_hsp=1)), (64, dict(hits=4, runs=0))):
        out.append(case("hit diagonals 992 and %d" % (992 + drift), [_islands(rng, (14, 14), (20,), (20 + drift,), 992)], None, [], st))
    for gap, st in ((100, dict(hits=4, runs=2, no_hsp=2)), (101, dict(hits=4, runs=0))):
        out.append(case("a gap of %d between hits" % gap, [_islands(rng, (14, 14), (gap - 13,), (gap - 13,), 600)], None, [], st))
    for k, st in ((15, dict(hits=3, runs=0)), (16, dict(hits=4, runs=2, alignments=2, no_hsp=2))):
        out.append(case("%d hits" % (k - 12), [_islands(rng, (k,), (), (), 600)], None, [], st))
    kw = dict(min_len=100, max_len=4000, min_ltr=100, max_ltr=200, identity=85)
    out.append(exact(rng, 200, 400, "a run that spans max_ltr - 13 positions", kw, stats=dict(runs=2, runs_span=0)))
    out.append(exact(rng, 201, 400, "a run that spans max_ltr - 12 positions", kw, keep=False, stats=dict(runs=2, runs_span=2, alignments=0)))
    return out


# ---- extension -------------------------------------------------------------------------------------------------------------------
def _seeded_terminals(rng, hl, hr):
    """two terminals that share one exact 40-mer, hl bases before it and hr after it 90 % identical with a substitution at every
    tenth base (never the first or the last base): only the 40-mer holds shared words"""
    t = rand(rng, hl + 40 + hr)
    pos = [p for p in list(range(hl - 1, 0, -10)) + list(range(hl + 40, hl + 40 + hr, 10)) if 3 <= p < len(t) - 3]
    return t, subs(t, pos), len(pos)


def _redos(half):
    """redos a side needs: the HSP must begin >= 32 bases inside the window, whose pad is 256, 1 024, 4 096, max_ltr"""
    return sum(half > p - 32 for p in (256, 1024, 4096))


def extension():
    rng = np.random.default_rng(104)
    kw = dict(min_len=400, max_len=22000, min_ltr=100, max_ltr=8192, identity=85)
    out = []
    for k, (hl, hr) in enumerate(((224, 100), (225, 100), (100, 224), (100, 225), (992, 60), (993, 60), (60, 4064), (60, 4065), (4100, 100),
                                  (300, 300), (1000, 1000), (4070, 4070), (4070, 300), (300, 1100))):
        far = 9000 if max(hl, hr) > 4000 else 1200
        for seed in range(1000 * k, 1000 * k + 50):       # the first seed at which no other words are shared (long sequences: no other run)
            rng = np.random.default_rng(seed)
            t, t2, nsub = _seeded_terminals(rng, hl, hr)
            s, ls, le, rs, re_ = element(rng, t, t2, 1500, lead=far, tail=far)
            st = {}
            LT.scan([s], stats=st, **kw)
            if st["runs"] == 2 and (far == 9000 or st["hits"] == 28):
                break
        T, redo = len(t), max(_redos(hl), _redos(hr))
        out.append(case("terminals of %d + 40 + %d bases around their only shared words" % (hl, hr), [s], kw,
                        [(0, ls, le, rs, re_, 2 * (T - nsub) - 4 * nsub, T - nsub, T)], dict(runs=2, alignments=2 * (1 + redo), redos=2 * redo, **({} if far == 9000 else dict(hits=28)))))
    rng = np.random.default_rng(104)
    # the pads clipped by both ends of the sequence
    t, t2, nsub = _seeded_terminals(rng, 600, 600)
    s = text(t, guard(rng, (0, 1)), rand(rng, 800), guard(rng, (2, 3)), t2)
    out.append(case("long terminals at both ends of their sequence", [s], kw,
                    [(0, 0, 1240, 2064, 3304, 2 * (1240 - nsub) - 4 * nsub, 1240 - nsub, 1240)], dict(redos=2, alignments=4)))
    # three bases more / fewer inside the second copy
    r = rand(rng, 300)
    ins = np.concatenate([r[:100], (r[100:103] + 2) & 3, r[100:]])
    out.append(case("an insertion of 3 bases", [element(rng, r, ins, 600)[0]], None, None, dict(records=1)))
    out.append(case("a deletion of 3 bases", [element(rng, r, np.delete(r, np.arange(100, 103)), 600)[0]], None, None, dict(records=1)))
    # 95 / 97 more bases in the second copy after its first 400: the words before them and the words after them are two runs, 95 / 97
    # diagonals apart.  At 95 the band of either holds the other diagonal and both give the whole terminal; at 97 neither does
    kw = dict(SMALL, max_ltr=2000)
    for drift in (95, 97):
        t, ins = rand(rng, 1000), rand(rng, drift)
        ins[0], ins[-1] = (t[400] + 1) & 3, (t[399] + 1) & 3
        s, ls, le, rs, re_ = element(rng, t, np.concatenate([t[:400], ins, t[400:]]), 700, 600, 600)
        whole = [(0, ls, le, rs, re_, 2 * 1000 - 5 * 95, 1000, 1095)]
        # (at 97: the 400 bases before and the 600 after, each with whatever few columns chance adds at the inserted bases)
        out.append(case("a drift of %d diagonals" % drift, [s], kw, whole if drift == 95 else None, dict(runs=4, records=1 if drift == 95 else 2)))
    return out


# ---- filters ---------------------------------------------------------------------------------------------------------------------
def filters():
    rng = np.random.default_rng(105)
    out = [exact(rng, 99, 300, "terminals of min_ltr - 1 bases", keep=False, stats=dict(drop_ltr=2)),
           exact(rng, 100, 300, "terminals of min_ltr bases", stats=dict(drop_ltr=0))]
    kw = dict(min_len=400, max_len=1000, min_ltr=100, max_ltr=1000, identity=85)
    for E, keep in ((399, False), (400, True), (999, True), (1000, True), (1001, False)):
        out.append(exact(rng, 120, E - 240 - 24, "an element of %d bases (min_len 400, max_len 1000)" % E, kw, keep=keep,
                         stats=dict(hits=108, drop_len=0 if keep else 2)))
    # a tandem pair: the copies begin with bases of {A, C} and end with bases of {G, T}, so that the alignment ends where they meet
    x = np.concatenate([guard(rng, (0, 1)), rand(rng, 126), guard(rng, (2, 3))])
    lead, tail = np.concatenate([rand(rng, 200), guard(rng, (0, 1))]), np.concatenate([guard(rng, (2, 3)), rand(rng, 200)])
    out.append(case("le == rs", [text(lead, x, x, tail)], None, [(0, 212, 362, 362, 512, 300, 150, 150)], dict(drop_overlap=0)))
    out.append(case("le == rs + 1", [text(lead, x, x, x[:1], tail)], None, [], dict(drop_overlap=2, alignments=2)))
    # 180 matches in 200 columns against identity 90 / 91; 107 matches in 123 columns: 100 * 107 is one below 87 * 123
    t, t2, nsub = _seeded_terminals(rng, 80, 80)
    assert (len(t), nsub) == (200, 16)
    t2 = subs(t2, (34, 54, 144, 164))
    for ident, keep in ((90, True), (91, False)):
        s, ls, le, rs, re_ = element(np.random.default_rng(7), t, t2, 400)
        out.append(case("180 matches in 200 columns at identity %d" % ident, [s], dict(SMALL, identity=ident),
                        [(0, ls, le, rs, re_, 360 - 80, 180, 200)] if keep else [], dict(drop_identity=0 if keep else 2)))
    t = rand(rng, 123)
    t2 = subs(t, list(range(5, 48, 6)) + list(range(75, 118, 6)))
    for ident, keep in ((86, True), (87, False)):
        s, ls, le, rs, re_ = element(np.random.default_rng(8), t, t2, 400)
        out.append(case("107 matches in 123 columns at identity %d" % ident, [s], dict(SMALL, identity=ident),
                        [(0, ls, le, rs, re_, 214 - 64, 107, 123)] if keep else [], dict(hits=15, drop_identity=0 if keep else 2)))
    return out


# ---- order -----------------------------------------------------------------------------------------------------------------------
def detour_element(rng):
    """an element whose second terminal leaves the diagonal D of its first 200 bases by -3 for 100 bases and comes back for 300 more,
    and 40 shared bases behind both terminals on diagonal D + 94: the runs of the terminals' own hits have bands that hold D - 3, the
    run of the 40 bases has the band D - 2 .. D + 189 and crosses the 100 bases off their diagonal -- the same place at a lower score"""
    A, N, B, C = rand(rng, 200), rand(rng, 100), rand(rng, 300), rand(rng, 40)
    one, two = np.concatenate([A, rand(rng, 3), N, B]), np.concatenate([A, N, rand(rng, 3), B])
    parts = [rand(rng, 500), guard(rng, (0, 1)), one, guard(rng, (0, 1)), rand(rng, 8), C, rand(rng, 700), guard(rng, (2, 3)), two, guard(rng, (2, 3)),
             rand(rng, 8 + 94), C, rand(rng, 400)]
    at = np.cumsum([0] + [len(p) for p in parts])
    return text(*parts), int(at[2]), int(at[3]), int(at[8]), int(at[9])


def order():
    rng = np.random.default_rng(106)
    out = [exact(rng, 400, 800, "two runs of one element, one record", stats=dict(runs=2, alignments=2, records=1))]
    s, ls, le, rs, re_ = detour_element(rng)
    out.append(case("one place from two bands at two scores", [s], dict(SMALL, identity=60), [(0, ls, le, rs, re_, 2 * 600 - 5 * 6, 600, 606)], None))
    a = exact(rng, 150, 300, "")["seqs"][0]
    b = exact(rng, 130, 500, "")["seqs"][0]
    out.append(case("records of three sequences, two elements in one", [a, b + a, b], None, None, dict(records=4)))
    return out


@functools.lru_cache(maxsize=None)
def small_cases():
    return tuple(sequences() + links() + runs() + extension() + filters() + order())


# ---- planted truth ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planted():
    """the genome of 32 planted elements of the issue -> (names, sequences, truth, [(seq, ls, le, rs, re)] the true place of every
    element, 0-based and half-open)"""
    from hite_amd import synth

    g = synth.make_ltr_element_genome(PLAN, seed=1)
    names = list(g["contigs"])
    places = []
    for t in g["truth"]:
        p = (t.get("adjusted") or t["line"]).split(" ")
        over = 120 if t["kind"] == "overhang" else 0
        places.append((names.index(p[11]), int(p[3]) - 1 - over, int(p[4]) + over, int(p[6]) - 1 - over, int(p[7]) + over))
    return names, [g["contigs"][n] for n in names], g["truth"], places


# ---- volume ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def volume(mbp=5.0, n_elements=40, seed=9):
    """one random sequence of mbp million bases with n_elements planted elements (terminals of 150 .. 1 200 bases, the second 1 .. 8 %
    diverged, internal sequences of 1 500 .. 6 000) -> (sequence as bytes, cut points between the elements)"""
    rng = np.random.default_rng(seed)
    n = int(mbp * 1e6)
    g = ACGT[rng.integers(0, 4, size=n)]
    slot = n // n_elements
    cuts = []
    for e in range(n_elements):
        term = rand(rng, int(rng.integers(150, 1201)))
        right = term.copy()
        m = rng.random(len(term)) < float(rng.uniform(0.01, 0.08))
        right[m] = (right[m] + rng.integers(1, 4, size=int(m.sum())).astype(np.uint8)) & 3
        unit = np.concatenate([term, rand(rng, int(rng.integers(1500, 6001))), right])
        pos = e * slot + int(rng.integers(100, slot - len(unit) - 100))
        g[pos:pos + len(unit)] = ACGT[unit]
        cuts.append(e * slot)
    return g.tobytes(), cuts[1:]


def split(seq, cuts, pieces):
    """the sequence in `pieces` pieces, cut at cut points spread evenly"""
    take = [cuts[(k * len(cuts)) // pieces] for k in range(1, pieces)]
    at = [0] + take + [len(seq)]
    return [seq[a:b] for a, b in zip(at, at[1:])]
