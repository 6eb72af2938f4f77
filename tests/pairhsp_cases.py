"""TEST INFRASTRUCTURE: the inputs of the pairwise-HSP tests (tests/test_pairhsp_cases.py and tests/test_host_compiled_pairhsp.py on
the CPU, tests/test_gpu_pairhsp.py on the device).  A case is (label, q, s, diag_min): the two sequences of one pair and the diag_min
of its call (None: no limit).  closed_forms() adds the records that follow from the definition by hand.

Most constructions plant exact cores (random ACGT) into backgrounds that cannot match each other -- Q's background is drawn from
{A, C}, S's from {G, T} -- so that the word hits, the votes and the reach of every alignment are known exactly."""
import numpy as np

import pairhsp_twin as T

GRID = (1, 11, 12, 13, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257)


def dna(rng, n, alphabet="ACGT"):
    return "".join(alphabet[k] for k in rng.integers(0, len(alphabet), n))


def mutate(rng, s, div, indel=0.2):
    """a copy of s at about `div` divergence: substitutions, and a share `indel` of the events single-base insertions or deletions"""
    out = []
    for c in s:
        if rng.random() < div:
            r = rng.random()
            if r < indel / 2:
                continue
            if r < indel:
                out.append(c + dna(rng, 1))
                continue
            out.append("ACGT"[("ACGT".index(c.upper()) + int(rng.integers(1, 4))) % 4] if c.upper() in "ACGT" else c)
        else:
            out.append(c)
    return "".join(out)


def planted(rng, qlen, slen, cores):
    """Q (background {A, C}) and S (background {G, T}) with the cores (q_pos, s_pos, text or length), 0-based, written into both"""
    q, s = list(dna(rng, qlen, "AC")), list(dna(rng, slen, "GT"))
    for qp, sp, core in cores:
        if isinstance(core, int):
            core = dna(rng, core)
        if isinstance(core, str):
            core = (core, core)
        q[qp:qp + len(core[0])] = core[0]
        s[sp:sp + len(core[1])] = core[1]
    assert len(q) == qlen and len(s) == slen
    return "".join(q), "".join(s)


def closed_forms():
    """(label, q, s, diag_min, records): pairs whose HSP set follows from the definition by hand"""
    rng = np.random.default_rng(101)
    out = []
    a = dna(rng, 199)
    out.append(("identical", a, a, None, [(1, 199, 1, 199, 398, 199, 199)]))
    b = a[:100] + ("A" if a[100] != "A" else "C") + a[101:]
    out.append(("one substitution", a, b, None, [(1, 199, 1, 199, 2 * 198 - 4, 198, 199)]))
    # three bases of Q are missing in S; the bases around the gap are chosen so that the gap cannot slide or close
    g = dna(rng, 98) + "AC" + "GGG" + "TA" + dna(rng, 95)
    out.append(("one 3-base gap", g, g[:100] + g[103:], None, [(1, 200, 1, 197, 2 * 197 - 15, 197, 200)]))
    for n, recs in ((30, [(101, 130, 51, 80, 60, 30, 30)]), (28, [(101, 128, 51, 78, 56, 28, 28)]), (27, [])):
        q, s = planted(rng, 260, 170, [(100, 50, n)])
        out.append(("a %d-base exact core in flanks that cannot match" % n, q, s, None, recs))
    # 18 + 11 + 11 matching bases around two mismatches: 7 words, one short of a window; 19 + 11 + 11: 8 words, score 2 * 41 - 8
    for n, recs in ((18, []), (19, [(101, 143, 51, 93, 74, 41, 43)])):
        x, y, z = dna(rng, n), dna(rng, 11), dna(rng, 11)
        q, s = planted(rng, 300, 200, [(100, 50, (x + "A" + y + "A" + z, x + "G" + y + "G" + z))])
        out.append(("a window of %d votes" % (n - 11), q, s, None, recs))
    # the same 30-base core 8 times in Q casts 8 x 19 hits, 9 times none
    core = dna(rng, 30)
    for k in (8, 9):
        q, s = planted(rng, 200 * k + 100, 300, [(50 + 200 * c, 100, core) for c in range(k)])
        # 8 copies: windows are taken by votes; every copy has 19, so the lowest bins win -- the copies nearest the end of Q
        recs = sorted([(51 + 200 * c, 80 + 200 * c, 101, 130, 60, 30, 30) for c in range(k - 4, k)]) if k == 8 else []
        out.append(("a word %d times in Q" % k, q, s, None, recs))
    # two cores next to each other in Q, 30 apart in S: the longer one is the first HSP, the 28 rows before it hold the other
    c1, c2 = dna(rng, 28), dna(rng, 60)
    q, s = planted(rng, 28 + 60 + 40, 28 + 30 + 60 + 40, [(0, 0, c1), (28, 58, c2)])
    out.append(("a rectangle of 28 rows before the first HSP", q, s, None, [(29, 88, 59, 118, 120, 60, 60), (1, 28, 1, 28, 56, 28, 28)]))
    q, s = planted(rng, 40 + 60 + 28, 40 + 60 + 30 + 28, [(40, 40, c2), (100, 130, c1)])
    out.append(("a rectangle of 28 rows after the first HSP", q, s, None, [(41, 100, 41, 100, 120, 60, 60), (101, 128, 131, 158, 56, 28, 28)]))
    # a self-pair with diag_min: the main diagonal is cut away, the repeat 700 bases on stays (once: j - i >= 500 only)
    # (the bases next to the two copies differ, so the alignment of the copies ends where they end)
    rep = dna(rng, 60)
    u = dna(rng, 98) + "AA" + rep + "GG" + dna(rng, 636) + "CC" + rep + "TT" + dna(rng, 138)
    out.append(("the self-pair with diag_min = 500", u, u, 500, [(101, 160, 801, 860, 120, 60, 60)]))
    return out


def length_grid():
    """m, n crossed over the strip edges: a random, a related and an unrelated (disjoint alphabets) pair each"""
    rng = np.random.default_rng(7)
    out = []
    for m in GRID:
        for n in GRID:
            a = dna(rng, m)
            out.append(("grid random %d x %d" % (m, n), a, dna(rng, n), None))
            rel = mutate(rng, (a + dna(rng, n))[:n + 8], 0.1)
            out.append(("grid related %d x %d" % (m, n), a, (rel + dna(rng, n))[:n], None))
            out.append(("grid unrelated %d x %d" % (m, n), dna(rng, m, "AC"), dna(rng, n, "GT"), None))
    return out


def word_and_window_rules():
    rng = np.random.default_rng(11)
    out = [c[:4] for c in closed_forms()]
    # five candidate windows, far apart, with 19 .. 23 votes: the four largest are taken
    cores = [(100 + 400 * k, 100 + 400 * (4 - k), 30 + k) for k in range(5)]
    q, s = planted(rng, 2200, 2200, cores)
    out.append(("five candidate windows", q, s, None))
    # the same with equal votes: the lowest bins win
    q, s = planted(rng, 2200, 2200, [(qp, sp, 30) for qp, sp, _ in cores])
    out.append(("five candidate windows with equal votes", q, s, None))
    # bin 0: the end of Q against the start of S; the last bin: the start of Q against the end of S; both at once
    q, s = planted(rng, 700, 900, [(700 - 40, 0, 40)])
    out.append(("a window at bin 0", q, s, None))
    q, s = planted(rng, 700, 900, [(0, 900 - 40, 40)])
    out.append(("a window at the last bin", q, s, None))
    q, s = planted(rng, 700, 900, [(700 - 40, 0, 40), (0, 900 - 40, 40), (300, 400, 50)])
    out.append(("windows at bin 0, in the middle and at the last bin", q, s, None))
    for m, n in ((64, 64), (65, 64), (64, 65), (128, 129)):      # the last bin right at a multiple of 64
        q, s = planted(rng, m, n, [(0, n - 32, 32), (m - 32, 0, 32)])
        out.append(("corner windows %d x %d" % (m, n), q, s, None))
    # two windows whose bands share an alignment: an insertion in S moves the second half by `ins` diagonals
    a, b = dna(rng, 300), dna(rng, 300)
    for ins in (20, 64, 70, 100, 127, 128, 129, 150, 200):
        out.append(("halves %d diagonals apart" % ins, a + b, a + dna(rng, ins) + b, None))
        out.append(("halves %d diagonals apart, the other way" % ins, a + dna(rng, ins) + b, a + b, None))
    return out


def diag_min_cases():
    rng = np.random.default_rng(13)
    out = []
    a = dna(rng, 600)
    rel = mutate(rng, a, 0.08, indel=0.5)
    for dm in (-40, -3, 0, 2, 5, 40):
        out.append(("diag_min %d through the band of a related pair" % dm, a, rel, dm))
        out.append(("diag_min %d through the band of a related pair, swapped" % dm, rel, a, dm))
    # the self-pair with diag_min = 500: direct repeats 500 .. 900 apart inside one sequence
    for k in range(4):
        rep = dna(rng, 300)
        u = dna(rng, 200) + rep + dna(rng, 200 + 150 * k) + mutate(rng, rep, 0.04) + dna(rng, 250)
        out.append(("self-pair %d with diag_min 500" % k, u, u, 500))
        out.append(("self-pair %d without diag_min" % k, u, u, None))
    return out


def bytes_cases():
    """runs of N, other bytes and lower case"""
    rng = np.random.default_rng(17)
    out = []
    a = dna(rng, 500)
    rel = mutate(rng, a, 0.05)
    out.append(("lower case", a.lower(), rel, None))
    out.append(("mixed case", "".join(c.lower() if k % 3 else c for k, c in enumerate(a)), rel.lower(), None))
    out.append(("runs of N in Q", a[:100] + "N" * 15 + a[115:300] + "n" * 40 + a[340:], rel, None))
    out.append(("runs of N in both", a[:100] + "N" * 15 + a[115:], rel[:98] + "N" * 20 + rel[118:], None))
    out.append(("other bytes", (a[:200] + "-RYKM*" + a[206:]).encode(), rel[:300].encode() + b"\x00\xff" + rel[302:].encode(), None))
    out.append(("only N", "N" * 100, "N" * 100, None))
    out.append(("N at every twelfth base", "".join("N" if k % 12 == 5 else c for k, c in enumerate(a)), a, None))
    return out


def drifting(rng, n, every, size, delete):
    """a sequence and a copy that loses (or gains) `size` bases every `every` bases: the alignment drifts across the diagonals"""
    a = dna(rng, n)
    out, k = [], 0
    while k < n:
        out.append(a[k:k + every])
        k += every
        if delete:
            k += size
        else:
            out.append(dna(rng, size))
    return a, "".join(out)


def band_edges():
    """alignments that reach or leave the edges of their band"""
    rng = np.random.default_rng(19)
    out = []
    for every, size in ((80, 8), (60, 3), (120, 12), (200, 31), (200, 33)):
        for delete in (True, False):
            a, b = drifting(rng, 1600, every, size, delete)
            out.append(("drift %d per %d, %s" % (size, every, "deletions" if delete else "insertions"), a, b, None))
            out.append(("drift %d per %d, %s, swapped" % (size, every, "deletions" if delete else "insertions"), b, a, None))
    # one jump of exactly the room below / above the diagonal of the votes, and one more
    a, b = dna(rng, 400), dna(rng, 150)
    for jump in (30, 31, 32, 33, 34, 94, 95, 96, 97, 98, 158, 159, 160, 161):
        out.append(("a jump of %d, insertion in S" % jump, a + b, a + dna(rng, jump, "GT") + b, None))
        out.append(("a jump of %d, insertion in Q" % jump, a + dna(rng, jump, "AC") + b, a + b, None))
    return out


def ties():
    """equal scores at every level of the order"""
    rng = np.random.default_rng(23)
    out = []
    x = dna(rng, 80)
    out.append(("tandem in Q", x + x, x, None))
    out.append(("tandem in S", x, x + x, None))
    out.append(("tandem in both", x + x, x + x, None))
    out.append(("three copies in both", x * 3, x * 3, None))
    q, s = planted(rng, 400, 400, [(50, 60, 40), (200, 210, 40)])
    out.append(("two cores of one score on one diagonal", q, s, None))
    q, s = planted(rng, 400, 400, [(50, 60, 40), (200, 230, 40), (300, 310, 40)])
    out.append(("three cores of one score in one band", q, s, None))
    c = dna(rng, 40)
    q, s = planted(rng, 400, 400, [(50, 60, c), (200, 215, c)])
    out.append(("one core twice in both", q, s, None))
    y = dna(rng, 30)
    out.append(("a gap that can sit in many places", y + "A" * 10 + y[::-1], y + "A" * 7 + y[::-1], None))
    out.append(("a short tandem repeat", "ACGTTGCA" * 30, "ACGTTGCA" * 25, None))
    out.append(("homopolymers", "A" * 300, "A" * 200, None))
    out.append(("dinucleotides", "AC" * 150, "CA" * 170, None))
    return out


def rectangles():
    rng = np.random.default_rng(29)
    out = []
    for pre in (26, 27, 28, 29, 40):
        c1, c2 = dna(rng, pre), dna(rng, 60)
        q, s = planted(rng, pre + 60 + 40, pre + 30 + 60 + 40, [(0, 0, c1), (pre, pre + 30, c2)])
        out.append(("%d rows before the first HSP" % pre, q, s, None))
        q, s = planted(rng, 40 + 60 + pre, 40 + 60 + 30 + pre, [(40, 40, c2), (100, 130, c1)])
        out.append(("%d rows after the first HSP" % pre, q, s, None))
        q, s = planted(rng, pre + 30 + 60 + 40, pre + 60 + 40, [(0, 0, c1), (pre + 30, pre, c2)])
        out.append(("%d columns before the first HSP" % pre, q, s, None))
    a, b, c = dna(rng, 200), dna(rng, 300), dna(rng, 150)
    out.append(("three blocks, two insertions", a + b + c, a + dna(rng, 40, "GT") + b + dna(rng, 35, "GT") + c, None))
    out.append(("three blocks, insertions on either side", a + dna(rng, 40, "AC") + b + c, a + b + dna(rng, 35, "GT") + c, None))
    return out


def production():
    """two pairs at production size: an element's internal sequence against a diverged copy, a terminal against a sequence at the limit"""
    rng = np.random.default_rng(31)
    a = dna(rng, 7100)
    b = (mutate(rng, a[:3000], 0.06) + dna(rng, 150) + mutate(rng, a[3000:], 0.03) + dna(rng, 200))[:7100]
    t = dna(rng, 300)
    long = dna(rng, 9000) + mutate(rng, t, 0.05) + dna(rng, 12000) + t + dna(rng, T.MAX_LEN)
    return [("7 100 x 7 100", a, b, None), ("300 x 32 768", t, long[:T.MAX_LEN], None)]


def refused():
    """(seqs, pairs, expected status pattern): a length beyond the limit, empty intervals, intervals and ids outside"""
    rng = np.random.default_rng(37)
    a, big = dna(rng, 100), dna(rng, T.MAX_LEN + 1)
    seqs = [a, big, a]
    pairs = [(0, 0, 100, 2, 0, 100), (0, 0, 100, 1, 0, T.MAX_LEN + 1), (1, 0, T.MAX_LEN + 1, 0, 0, 100), (0, 0, 100, 1, 1, T.MAX_LEN + 1),
             (0, 0, 101, 2, 0, 100), (0, 0, 100, 2, 50, 101), (0, -1, 50, 2, 0, 100), (0, 60, 50, 2, 0, 100), (0, 10, 10, 2, 0, 100),
             (0, 0, 100, 2, 100, 100), (3, 0, 100, 2, 0, 100), (0, 0, 100, -1, 0, 100), (0, 0, 100, 0, 0, 100)]
    ok = [True, False, False, True, False, False, False, False, False, False, False, False, True]
    return seqs, pairs, ok


def mixed(n=3000, seed=41):
    """many small pairs of every kind in one call: (seqs, pairs)"""
    rng = np.random.default_rng(seed)
    seqs, pairs = [], []
    for k in range(n):
        m = int(rng.integers(30, 400))
        a = dna(rng, m)
        kind = k % 5
        if kind == 0:
            b = mutate(rng, a, 0.08)
        elif kind == 1:
            b = dna(rng, int(rng.integers(30, 400)))
        elif kind == 2:
            b = dna(rng, 50) + mutate(rng, a[m // 3:], 0.03) + dna(rng, 20)
        elif kind == 3:
            b = a[:m // 2] + dna(rng, int(rng.integers(1, 60))) + a[m // 2:]
        else:
            b = a.lower()
        seqs += [a, b]
        lo = int(rng.integers(0, 10))
        pairs.append((2 * k, lo, len(a), 2 * k + 1, 0, len(b) - int(rng.integers(0, 10))))
    return seqs, pairs


def small_cases():
    """every case the Python form of the twin can take in reasonable time"""
    out = word_and_window_rules()[:14] + rectangles() + ties() + bytes_cases()[:3]
    grid = length_grid()
    out += [c for c in grid if max(len(c[1]), len(c[2])) <= 65][::3] + [c for c in grid if "related" in c[0] and min(len(c[1]), len(c[2])) >= 63][::5]
    return [c for c in out if len(c[1]) * min(len(c[2]), 192) <= 200000]


def all_cases():
    return word_and_window_rules() + length_grid() + diag_min_cases() + bytes_cases() + band_edges() + ties() + rectangles()


def run(fn, cases):
    """the cases through fn(seqs, pairs, diag_min) -> one result per case, one call per diag_min"""
    res = [None] * len(cases)
    for dm in sorted({c[3] for c in cases}, key=lambda d: (d is not None, d)):
        idx = [k for k, c in enumerate(cases) if c[3] == dm]
        seqs, pairs = [], []
        for k in idx:
            seqs += [cases[k][1], cases[k][2]]
            pairs.append((len(seqs) - 2, 0, len(cases[k][1]), len(seqs) - 1, 0, len(cases[k][2])))
        for k, r in zip(idx, fn(seqs, pairs, dm)):
            res[k] = r
    return res
