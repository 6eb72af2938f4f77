"""Copy tables for tests/test_fine_row_cases.py and tests/test_gpu_fine_rows.py: the front of a fine-stage pass
(hite_amd/csrc/hite_pipeline.hip: select_rows_kernel -> row_meta_kernel -> row_gather_kernel with emit_padded, emit_span / emit_span4
of hite_genome.h, and clip_probe_kernel) at the limits of its own code.  The device's rows come out of hite_fine_rows
(Context.fine_rows), which runs the launches of the stage itself; the expectation is tests/oracle_pipeline.py: pass_rows, the rows
fine_stage_candidate judges.  Rows, their order, the truncation flag, the lengths and EVERY WINDOW BYTE are compared, exactly.

One genome (GENOME) for every case: four contigs of at most 40 003 bases whose "<name>:" byte order differs from the packing order,
the second with runs of N of 1 .. 33 bases at every offset 0 .. 33 of a 32-base word of the packed genome, the third with a planted
family for the probed pads.  Seeded, pure python + numpy.

A check_* function takes the object under test -- a hite_amd.Context, or Twin (the same calls answered by the twin) -- and compares it
with the twin; the selfcheck_* functions show, BY THE TWIN ALONE, that a case sits on the limit it is named for (CPU test)."""
import numpy as np

import oracle_lib as O
import oracle_pipeline as OP

FLANK = 50
MAXROWS = OP.MAXROWS
NAMES = ["chr10", "chr2", "chr1_random", "chrX"]     # byte order of "<name>:": chr10 < chr1_random < chr2 < chrX -> ranks 0, 2, 1, 3
RUN_LENS = (1, 15, 16, 17, 31, 32, 33)
RUN_OFFS = tuple(range(34))
RUN_STEP = 128
PADS = tuple(range(18)) + (31, 32, 33)
CLIP_K, CLIP_MM = 21, 5
DUMMY = "ACGTTGCAAGCTTAGGCATC" * 3

_COMP = str.maketrans("ACGTNacgtn", "TGCANtgcan")
_B = np.frombuffer(b"ACGT", dtype=np.uint8)


def revcomp(s):
    return s.translate(_COMP)[::-1]


def rand_seq(rng, n):
    return _B[rng.integers(0, 4, n)].tobytes().decode()


def _other(ch):
    return "CGTA"["ACGT".index(ch)]


# ------------------------------------------------------------------------------------------------------------------------------
# the genome
# ------------------------------------------------------------------------------------------------------------------------------
FAM_LEN, FAM_AT, FAM_STEP, FAM_N = 300, 20000, 600, 8
_genome = None


def genome():
    """contigs, coff, runs [(length, offset in the 32-base word, position in contig 1)], family (the planted sequence)"""
    global _genome
    if _genome is None:
        rng = np.random.default_rng(8032)
        lens = [40003, 512 + RUN_STEP * len(RUN_LENS) * len(RUN_OFFS) + 700, 30001, 8009]
        contigs = [list(rand_seq(rng, n)) for n in lens]
        coff = [0]
        for n in lens:
            coff.append(coff[-1] + n)
        runs, r = [], 0
        for L in RUN_LENS:
            for off in RUN_OFFS:
                g = (coff[1] + 512 + RUN_STEP * r + 31) // 32 * 32 + off          # global position: `off` past a word's first base
                p = g - coff[1]
                contigs[1][p:p + L] = "N" * L
                runs.append((L, off, p))
                r += 1
        fam = rand_seq(rng, FAM_LEN)
        for i in range(FAM_N):
            at = FAM_AT + FAM_STEP * i
            contigs[2][at:at + FAM_LEN] = revcomp(fam) if i % 2 else fam
        _genome = {"contigs": ["".join(c) for c in contigs], "coff": coff, "runs": runs, "family": fam}
        assert all(len(c) <= 40003 for c in _genome["contigs"]) and "N" * 33 in _genome["contigs"][1]
    return _genome


def clen(ci):
    return len(genome()["contigs"][ci])


def win(ci, lo, n, minus=0, clip=0, flank=FLANK):
    """the copy record whose window at `flank` is [lo, lo + n) of contig ci, with its clip word"""
    return (ci, lo + flank + 1, lo + n - flank, int(minus), 0, int(clip))


def padcopy(ci, lo, n, minus, a, b, flank=FLANK):
    """... padded by a bytes in front of and b behind the window AS IT IS READ (the word is kept in genome orientation)"""
    left, right = (b, a) if minus else (a, b)
    return win(ci, lo, n, minus, left | (right << 16), flank)


def front_back(cp):
    a, b = cp[5] & 0xffff, cp[5] >> 16
    return (b, a) if cp[3] else (a, b)


# ------------------------------------------------------------------------------------------------------------------------------
# the twin in the device's place
# ------------------------------------------------------------------------------------------------------------------------------
def twin_rows(contigs, names, cands, copies, flank=FLANK, rows_pass=0):
    """Context.fine_rows by the twin: pass 0 = the first500 + last500 forms where a window > 1000 exists, else the full windows; pass 1 =
    the full windows of the candidates that have a window > 1000"""
    out = []
    for cand, cps in zip(cands, copies):
        recs = OP.pass_records(cand, cps, contigs, flank, names)
        big = any(r[5] for r in recs)
        if rows_pass == 0:
            keep, wins = OP.pass_rows(cand, cps, contigs, flank, names, cut=big, recs=recs)
            tr = big
        else:
            keep, wins = OP.pass_rows(cand, cps, contigs, flank, names, cut=False, recs=recs) if big else ([], [])
            tr = False
        out.append([(i, w.encode(), tr) for i, w in zip(keep, wins)])
    ls = [len(r[1]) for rows in out for r in rows]
    return out, [len(ls), sum((n + 15) & ~15 for n in ls), max(ls) if ls else 0, 0]


def twin_clips(contigs, cands, copies):
    """Context.clip_probe by the twin: words in the orientation of the genome; 0 for a contig index out of range"""
    out = []
    for cand, cps in zip(cands, copies):
        ws = []
        for cp in cps:
            ci, s, e, mn = cp[:4]
            if not 0 <= ci < len(contigs):
                ws.append(0)
                continue
            pr = O.clip_probe(cand, OP._interval(contigs[ci], s, e, mn))
            ws.append(((pr >> 16) | ((pr & 0xffff) << 16)) if mn else pr)
        out.append(ws)
    return out


class Twin:
    """the calls of hite_amd.Context the checks use, answered by the twin"""

    def genome_pack(self, contigs):
        self.contigs, self.names = list(contigs), None          # (packing a genome drops the contig order, as the library does)

    def set_contig_order(self, names):
        self.names = names

    def fine_rows(self, cands, copies, flank=FLANK, rows_pass=0):
        return twin_rows(self.contigs, self.names, cands, copies, flank, rows_pass)

    def clip_probe(self, cands, copies):
        return twin_clips(self.contigs, cands, copies)

    def flank_region_align(self, te_type, cands, copies, plant=1, flank=FLANK):
        res, stats = [], [0] * 12
        for cand, cps in zip(cands, copies):
            r = OP.fine_stage_candidate(te_type, cand, cps, self.contigs, plant=plant, flank=flank, contig_names=self.names)
            res.append((r[0], r[1], r[2], r[3], -1, -1))
            a, ta = twin_rows(self.contigs, self.names, [cand], [cps], flank, 0)
            stats[0] += ta[0]
            stats[1] += ta[1]
            if a[0] and a[0][0][2]:
                ra, _ = OP.judge_windows(te_type, cand, [w.decode() for _i, w, _t in a[0]], plant)
                if ra[0] != "EXC" and ra[0]:
                    _b, tb = twin_rows(self.contigs, self.names, [cand], [cps], flank, 1)
                    stats[4] += tb[0]
                    stats[5] += tb[1]
        return res, stats


def use(dev, order=True):
    """GENOME resident in dev (packed once per object), the contig order set or cleared"""
    g = genome()
    if getattr(dev, "_fine_row_genome", None) is not g:
        dev.genome_pack(g["contigs"])
        dev._fine_row_genome = g
    dev.set_contig_order(NAMES if order else None)
    return g


def compare(dev, case, order=True, passes=(0, 1)):
    """rows, order, truncation flags, lengths, every window byte and the three totals, both passes -> the twin's rows per pass"""
    g = use(dev, order)
    out = []
    for p in passes:
        exp, et = twin_rows(g["contigs"], NAMES if order else None, case["cands"], case["copies"], case.get("flank", FLANK), p)
        got, gt = dev.fine_rows(case["cands"], case["copies"], flank=case.get("flank", FLANK), rows_pass=p)
        assert len(got) == len(exp), (case["name"], p)
        for k, (gr, er) in enumerate(zip(got, exp)):
            assert [(r[0], r[2], len(r[1])) for r in gr] == [(r[0], r[2], len(r[1])) for r in er], (case["name"], p, k)
            for a, b in zip(gr, er):
                if a[1] != b[1]:
                    bad = [i for i in range(len(b[1])) if a[1][i] != b[1][i]]
                    raise AssertionError("%s pass %d candidate %d copy %d: %d bytes differ, first at %d: %r != %r" %
                                         (case["name"], p, k, a[0], len(bad), bad[0], a[1][bad[0]:bad[0] + 8], b[1][bad[0]:bad[0] + 8]))
        assert [int(x) for x in gt] == et, (case["name"], p, gt, et)
        out.append(exp)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# select_rows_kernel: copies per candidate, eligibility, the mode thresholds
# ------------------------------------------------------------------------------------------------------------------------------
def _ineligible(i):
    """a window that does not exist, four ways"""
    kind, mn = i % 4, (i >> 2) & 1
    if kind == 0:
        return (0, FLANK, 300, mn, 0, 0)                              # s1 - 1 - flank = -1
    if kind == 1:
        return (3, clen(3) - 300, clen(3) - FLANK + 1, mn, 0, 0)      # e1 + flank = clen + 1
    if kind == 2:
        return win(2, 500 + i, 99, mn)                                # 99 bases
    return (4 if i & 4 else -1, 1000, 1300, mn, 0, 0)                 # no such contig


SELECT_K = ((0, 0), (1, 1), (1, 0), (100, 100), (101, 101), (101, 100), (255, 100), (255, 101), (256, 100), (256, 101), (257, 100),
            (257, 101), (257, 257), (513, 100), (513, 101), (513, 513))


def _select_candidate(rng, k, E):
    must = sorted({i for i in (0, 255, 256, 257, 511, 512, k - 1) if 0 <= i < k})[:E]
    rest = [i for i in range(k) if i not in must]
    el = set(must) | set(int(x) for x in rng.choice(rest, E - len(must), replace=False)) if E > len(must) else set(must)
    copies = []
    for i in range(k):
        if i not in el:
            copies.append(_ineligible(i))
            continue
        ci = int(rng.integers(0, 4))
        n = int(rng.integers(380, 400) if i in must and E > MAXROWS else rng.integers(100, 400))      # (the rank path keeps the rows at the chunk edges)
        copies.append(win(ci, int(rng.integers(0, clen(ci) - n)), n, int(rng.integers(0, 2))))
    return copies, sorted(el)


_cases = {}


def case_select():
    if "select" not in _cases:
        rng = np.random.default_rng(10409)
        cps, els = [], []
        for k, E in SELECT_K:
            c, el = _select_candidate(rng, k, E)
            cps.append(c)
            els.append(el)
        _cases["select"] = {"name": "select", "cands": [DUMMY] * len(cps), "copies": cps, "eligible": els}
    return _cases["select"]


def case_modes():
    """window lengths 99 / 100 / 1000 / 1001 and the candidates whose mode they decide"""
    if "modes" not in _cases:
        rng = np.random.default_rng(10439)
        thr = [win(2, 1000, 99), win(2, 1200, 100), win(2, 1400, 1000, 1)]
        thr2 = [win(2, 3000, 1000), win(2, 4100, 1001, 1)]
        one_big = [win(0, int(rng.integers(0, 38000)), 1000 - 50 * (i % 8), i & 1) for i in range(150)]     # 18 or 19 of each length
        one_big.insert(77, win(2, 6000, 1001))
        all_1000 = [win(i % 3 if i % 3 != 1 else 3, 100 + 53 * i, 1000, (i >> 1) & 1) for i in range(120)]
        cps = [thr, thr2, one_big, all_1000]
        _cases["modes"] = {"name": "modes", "cands": [DUMMY] * len(cps), "copies": cps}
    return _cases["modes"]


def check_select(dev):
    compare(dev, case_select())
    compare(dev, case_modes())


def selfcheck_select():
    g, c = genome(), case_select()
    rows, _t = twin_rows(g["contigs"], NAMES, c["cands"], c["copies"], FLANK, 0)
    reached = set()
    for (k, E), cps, el, r in zip(SELECT_K, c["copies"], c["eligible"], rows):
        kept = [x[0] for x in r]
        assert len(cps) == k and len(el) == E and len(kept) == min(E, MAXROWS) and set(kept) <= set(el) and kept == sorted(kept), (k, E)
        assert not any(x[2] for x in r)
        if E <= MAXROWS:
            assert kept == el
            reached.add("keep-all" + (" k > E" if k > E else ""))
        else:
            assert kept != el[:MAXROWS], (k, E)          # not simply the first 100 eligible
            reached.add("rank" + (" k > E" if k > E else ""))
        if k > 256 and E >= MAXROWS:
            assert min(kept) < 256 <= max(kept), (k, E)
            reached.add("both sides of 256")
        if k > 512 and E >= MAXROWS:
            assert any(256 <= x < 512 for x in kept) and max(kept) >= 512, (k, E)
            reached.add("both sides of 512")
    assert len(reached) == 6, reached
    m = case_modes()
    a, _t = twin_rows(g["contigs"], NAMES, m["cands"], m["copies"], FLANK, 0)
    b, _t = twin_rows(g["contigs"], NAMES, m["cands"], m["copies"], FLANK, 1)
    assert [(x[0], x[2], len(x[1])) for x in a[0]] == [(1, False, 100), (2, False, 1000)] and b[0] == []
    assert [(x[0], x[2], len(x[1])) for x in a[1]] == [(1, True, 1000)] and [(x[0], len(x[1])) for x in b[1]] == [(0, 1000), (1, 1001)]
    assert [(x[0], x[2]) for x in a[2]] == [(77, True)] and len(b[2]) == MAXROWS and 77 in [x[0] for x in b[2]]
    lens = sorted((cp[2] - cp[1] + 1 + 2 * FLANK for cp in m["copies"][2]), reverse=True)
    assert sorted((len(x[1]) for x in b[2]), reverse=True) == lens[:MAXROWS] and lens[MAXROWS - 1] == lens[MAXROWS]      # a tie across the cut
    assert len(a[3]) == MAXROWS and not any(x[2] for x in a[3]) and all(len(x[1]) == 1000 for x in a[3]) and b[3] == []


# ------------------------------------------------------------------------------------------------------------------------------
# length ties across the cut: the name alone decides
# ------------------------------------------------------------------------------------------------------------------------------
def _shuffled(rng, xs):
    return [xs[int(i)] for i in rng.permutation(len(xs))]


def tie_cases():
    """[(case, numeric)]: one candidate each; numeric: the numeric order of starts / ends would keep another set"""
    if "ties" not in _cases:
        rng = np.random.default_rng(8110)
        out = []
        # starts 9 / 10, 99 / 100, 999 / 1000, 9999 / 10000 as decimal strings (flank 8: the window of start 9 begins at genome position 0)
        st = list(range(9, 131)) + [999, 1000, 9999, 10000]
        out.append(({"name": "tie_starts", "flank": 8, "copies": [_shuffled(rng, [win(0, s - 9, 200, 0, 0, 8) for s in st])]}, True))
        # one start, ends 9945 .. 10055: windows > 1000, their first500 + last500 forms tie at 1000
        out.append(({"name": "tie_ends", "copies": [_shuffled(rng, [(0, 8901, e, 0, 0, 0) for e in range(9945, 10056)])]}, True))
        # one interval on both strands
        both = [win(2, 700 + 211 * i, 300, m) for i in range(60) for m in (0, 1)] + [win(3, 4000, 300)]
        out.append(({"name": "tie_strands", "copies": [_shuffled(rng, both)]}, False))
        # the same record twice: the cut falls between the two
        pairs = [win(0, 1500 + 307 * i, 250, i & 1) for i in range(55)]
        out.append(({"name": "tie_twice", "copies": [[win(3, 4000, 250)] + pairs + pairs[::-1]]}, False))
        # contigs whose "<name>:" order is not the packing order
        ct = [win(1, 2000 + 150 * i, 180, i & 1) for i in range(60)] + [win(2, 2000 + 150 * i, 180, i & 1) for i in range(60)] + \
             [win(0, 2000 + 150 * i, 180, i & 1) for i in range(10)]
        out.append(({"name": "tie_contigs", "copies": [_shuffled(rng, ct)]}, False))
        for c, _n in out:
            c["cands"] = [DUMMY]
        _cases["ties"] = out
    return _cases["ties"]


def check_ties(dev):
    """with the contig order set, and again with none (contigs then compare by index)"""
    for c, _numeric in tie_cases():
        compare(dev, c, order=True)
        compare(dev, c, order=False)


def tie_tables(c, names):
    """(names, lengths the selection goes by, indices) of the windows of a tie case in the pass where they tie"""
    g = genome()
    recs = OP.pass_records(c["cands"][0], c["copies"][0], g["contigs"], c.get("flank", FLANK), names)
    big = any(r[5] for r in recs)
    recs = [r for r in recs if r[5]] if big else recs
    return [r[2] for r in recs], [1000 if big else len(r[1]) for r in recs], [r[0] for r in recs]


def selfcheck_ties():
    g = genome()
    kept_by = {}
    for c, numeric in tie_cases():
        cps = c["copies"][0]
        for names in (NAMES, None):
            nm, ln, idx = tie_tables(c, names)
            rows, _t = twin_rows(g["contigs"], names, c["cands"], c["copies"], c.get("flank", FLANK), 0)
            kept = [x[0] for x in rows[0]]
            kept_by[(c["name"], names is None)] = kept
            assert len(nm) > MAXROWS and len(kept) == MAXROWS, c["name"]
            cut = sorted(ln, reverse=True)
            assert cut[MAXROWS - 1] == cut[MAXROWS], c["name"]                              # a tie across the cut
            in_order = [idx[i] for i in OP.select_rows(ln, None)]
            assert kept != in_order, c["name"]
            if numeric:         # the greater contig, then the greater start, end, strand AS NUMBERS
                by_name = sorted(range(len(NAMES)), key=lambda k: (NAMES[k] + ":").encode())
                lens = dict(zip(idx, ln))
                num = sorted(idx, key=lambda i: (-lens[i], -(by_name.index(cps[i][0]) if names else cps[i][0]), -cps[i][1], -cps[i][2], -cps[i][3]))
                assert kept != sorted(num[:MAXROWS]), c["name"]
    t = tie_cases()[3][0]["copies"][0]
    kept = kept_by[("tie_twice", False)]
    split = [i for i in range(1, 56) if (i in kept) != (111 - i in kept)]                  # record i and its repeat 111 - i
    assert len(split) == 1 and split[0] in kept and t[split[0]] == t[111 - split[0]]        # ... the earlier one is kept
    both = tie_cases()[2][0]["copies"][0]
    kept = kept_by[("tie_strands", False)]
    half = [i for i in kept if both[i][0] == 2 and sum(1 for j in kept if both[j][:3] == both[i][:3]) == 1]
    assert half and all(both[i][3] == 1 for i in half)                                     # '-' sorts behind '+': the minus window is the greater name
    assert kept_by[("tie_contigs", False)] != kept_by[("tie_contigs", True)]
    ct = tie_cases()[4][0]["copies"][0]
    assert sum(1 for i in kept_by[("tie_contigs", False)] if ct[i][0] == 1) == 60 and sum(1 for i in kept_by[("tie_contigs", True)] if ct[i][0] == 2) == 60


# ------------------------------------------------------------------------------------------------------------------------------
# row_meta_kernel / slots: rows per call, the last candidate of a batch
# ------------------------------------------------------------------------------------------------------------------------------
def slot_cases():
    if "slots" not in _cases:
        w = [win(2, 1000 + 300 * i, 100 + 7 * i, i & 1) for i in range(8)]
        shapes = {"rows_1": [[w[0]]], "rows_1_last_empty": [[w[1]], []], "rows_4": [[w[0]], [], [w[1], w[2], w[3]]],
                  "rows_5": [[w[0], w[1]], [w[2], w[3], w[4]]], "rows_5_last_empty": [[], w[:5], [_ineligible(2)]],
                  "rows_0": [[], [_ineligible(1)]]}
        _cases["slots"] = [{"name": k, "cands": [DUMMY] * len(v), "copies": v} for k, v in shapes.items()]
    return _cases["slots"]


def check_slots(dev):
    for c in slot_cases():
        compare(dev, c)


def selfcheck_slots():
    g = genome()
    want = {"rows_1": 1, "rows_1_last_empty": 1, "rows_4": 4, "rows_5": 5, "rows_5_last_empty": 5, "rows_0": 0}
    for c in slot_cases():
        rows, t = twin_rows(g["contigs"], NAMES, c["cands"], c["copies"], FLANK, 0)
        assert t[0] == want[c["name"]] and t[1] == sum((len(x[1]) + 15) // 16 * 16 for r in rows for x in r)
        assert ("last_empty" in c["name"] or c["name"] == "rows_0") == (rows[-1] == [])


def check_stage_stats(dev):
    """stats[0], stats[1] (pass A) and stats[4], stats[5] (pass B) of the whole stage are the totals of the rows under test, on tables
    where no candidate has a first500 + last500 form (pass B is empty)"""
    use(dev)
    for c in slot_cases() + [case_select(), tie_cases()[2][0]]:
        _res, stats = dev.flank_region_align("tir", c["cands"], c["copies"], plant=1, flank=c.get("flank", FLANK))
        _rows, t = twin_rows(genome()["contigs"], NAMES, c["cands"], c["copies"], c.get("flank", FLANK), 0)
        assert [int(stats[0]), int(stats[1]), int(stats[4]), int(stats[5])] == [t[0], t[1], 0, 0], (c["name"], list(stats), t)


def check_stage_stats_passing(dev, seed=41):
    """the same on families (tests/synth_small.py) where every candidate that has a first500 + last500 form passes on it: pass B then
    holds exactly the rows of hite_fine_rows' pass 1"""
    import synth_small

    g = synth_small.make(seed, n_fam=10)
    dev.genome_pack(g["contigs"])
    dev._fine_row_genome = None
    tw = Twin()
    tw.genome_pack(g["contigs"])
    cands, copies, n_big = [], [], 0
    for cand, cps in zip(g["cands"], g["copies"]):
        big = any(r[5] for r in OP.pass_records(cand, cps, g["contigs"], FLANK, None))
        if big and not OP.fine_stage_candidate("tir", cand, cps, g["contigs"], plant=1)[0]:
            continue
        cands.append(cand)
        copies.append(cps)
        n_big += big
    assert n_big >= 2 and len(cands) > n_big
    _res, stats = dev.flank_region_align("tir", cands, copies, plant=1)
    _eres, est = tw.flank_region_align("tir", cands, copies, plant=1)
    _ra, ta = dev.fine_rows(cands, copies, rows_pass=0)
    _rb, tb = dev.fine_rows(cands, copies, rows_pass=1)
    assert [int(stats[k]) for k in (0, 1, 4, 5)] == [est[k] for k in (0, 1, 4, 5)] == [ta[0], ta[1], tb[0], tb[1]] and tb[0] > 0, (list(stats), est, ta, tb)


# ------------------------------------------------------------------------------------------------------------------------------
# row_gather_kernel / emit_span / emit_span4: lengths, positions, N runs, the first500 + last500 form
# ------------------------------------------------------------------------------------------------------------------------------
SHORT_LENS = tuple(range(100, 164))
LONG_LENS = tuple(range(1023, 1042))
TRUNC_LENS = (1001, 1015, 1016, 1017, 1999, 2000)


def gather_cases():
    if "gather" not in _cases:
        g = genome()
        out = []
        for m in (0, 1):
            out.append({"name": "lengths_100_163_%s" % "+-"[m], "copies": [[win(2, 3000 + 211 * j, n, m) for j, n in enumerate(SHORT_LENS)]]})
            out.append({"name": "lengths_1023_1041_%s" % "+-"[m], "copies": [[win(0, 700 + 1051 * j, n, m) for j, n in enumerate(LONG_LENS)]]})
            out.append({"name": "trunc_%s" % "+-"[m], "copies": [[win(2, 90 + 2003 * j, n, m) for j, n in enumerate(TRUNC_LENS)]]})
        ends = []
        for n in range(100, 120):
            ends.append([win(0, 0, n, m) for m in (0, 1)] + [win(3, clen(3) - n, n, m) for m in (0, 1)] +
                        [win(ci, 0, n, m) for ci in (1, 2, 3) for m in (0, 1)])
        out.append({"name": "contig_ends", "copies": ends})
        # a window of > 1000 at genome position 0 and one at the last base: the halves of the first500 + last500 form at both ends
        out.append({"name": "contig_ends_long", "copies": [[win(0, 0, n, m), win(3, clen(3) - n, n, m)] for n in (1001, 1018) for m in (0, 1)]})
        per, grp = [], []
        for (L, off, p) in g["runs"]:
            for m in (0, 1):
                grp += [win(1, p - 30, 100 + (L + off) % 64, m), win(1, p, 100 + off, m), win(1, p + L - 120 - off % 7, 120 + off % 7, m)]
            if len(grp) + 6 > MAXROWS:
                per.append(grp)
                grp = []
        per.append(grp)
        out.append({"name": "n_runs", "copies": per})
        for c in out:
            c["cands"] = [DUMMY] * len(c["copies"])
        _cases["gather"] = out
    return _cases["gather"]


def check_gather(dev, name):
    compare(dev, [c for c in gather_cases() if c["name"] == name][0])


def gather_names():
    return [c["name"] for c in gather_cases()]


def selfcheck_gather():
    g = genome()
    ct = g["contigs"]
    seen_runs = set()
    for c in gather_cases():
        a, ta = twin_rows(ct, NAMES, c["cands"], c["copies"], FLANK, 0)
        b, tb = twin_rows(ct, NAMES, c["cands"], c["copies"], FLANK, 1)
        nm = c["name"]
        if nm.startswith("lengths_100"):
            assert tuple(len(x[1]) for x in a[0]) == SHORT_LENS and tb[0] == 0
        elif nm.startswith("lengths_1023"):
            assert tuple(len(x[1]) for x in b[0]) == LONG_LENS and all(x[2] and len(x[1]) == 1000 for x in a[0]) and len(a[0]) == len(LONG_LENS)
            assert min(LONG_LENS) // 16 < 64 < max(LONG_LENS) // 16 + 1                 # 64 groups of 16 bytes: a lane's second turn begins
        elif nm.startswith("trunc"):
            assert tuple(len(x[1]) for x in b[0]) == TRUNC_LENS and all(x[2] for x in a[0])
            for x, y in zip(a[0], b[0]):
                assert x[1] == y[1][:500] + y[1][-500:]
        elif nm.startswith("contig_ends"):
            for cps, rows in zip(c["copies"], b if "long" in nm else a):
                assert len(rows) == len(cps)
                for cp, x in zip(cps, rows):
                    lo, n = cp[1] - 1 - FLANK, len(x[1])
                    assert lo == 0 or lo + n == clen(3)
                    w = ct[cp[0]][lo:lo + n]
                    assert x[1].decode() == (revcomp(w) if cp[3] else w)
            assert any(cp[0] == 0 and cp[3] for cps in c["copies"] for cp in cps)       # a minus row at genome position 0
        elif nm == "n_runs":
            for cps, rows in zip(c["copies"], a):
                assert len(rows) == len(cps) <= MAXROWS
                for cp, x in zip(cps, rows):
                    w = x[1].decode()
                    assert w == (revcomp(ct[1][cp[1] - 51:cp[2] + 50]) if cp[3] else ct[1][cp[1] - 51:cp[2] + 50])
                    plus = revcomp(w) if cp[3] else w
                    for (L, off, p) in g["runs"]:
                        q = p - (cp[1] - 51)
                        if q == 0 and ct[1][p - 1] != "N":
                            seen_runs.add((L, off, "first", cp[3]))
                            assert plus[:L] == "N" * L and plus[L] != "N"
                        elif q + L == len(w):
                            seen_runs.add((L, off, "last", cp[3]))
                            assert plus[-L:] == "N" * L and plus[-L - 1] != "N"
                        elif q == 30:
                            seen_runs.add((L, off, "inside", cp[3]))
                            assert plus[30:30 + L] == "N" * L and plus[29] != "N" and plus[30 + L] != "N"
    assert len(seen_runs) == len(RUN_LENS) * len(RUN_OFFS) * 6, len(seen_runs)
    assert {(g["coff"][1] + p) % 32 for (_L, _o, p) in g["runs"]} == set(range(32))


# ------------------------------------------------------------------------------------------------------------------------------
# emit_padded: clip words given
# ------------------------------------------------------------------------------------------------------------------------------
def _pad_candidates(centre, rows):
    return [[centre] + rows[i:i + MAXROWS - 1] for i in range(0, len(rows), MAXROWS - 1)]


def pad_cases():
    if "pads" not in _cases:
        g = genome()
        out = []
        for m0 in (0, 1):
            # every front pad x every back pad x both strands of the row, the centre on strand m0 with no clip of its own; the row's
            # first base at slot offset a mod 16
            rows = [padcopy(0, 100 + 37 * j, 100 + j % 16, j & 1, a, b) for j, (a, b) in enumerate((a, b) for a in PADS for b in PADS for _m in (0, 1))]
            out.append({"name": "pads_grid_%s" % "+-"[m0], "copies": _pad_candidates(win(2, 5000, 140, m0), rows)})
            # a centre with clips (5, 7) of its own: a <, =, > a0
            rows = [padcopy(0, 300 + 41 * j, 100 + j % 16, j & 1, a, b) for j, (a, b) in
                    enumerate((a, b) for a in (0, 4, 5, 6, 17, 33) for b in (0, 6, 7, 8, 17, 33) for _m in (0, 1))]
            out.append({"name": "pads_centre_clip_%s" % "+-"[m0], "copies": _pad_candidates(padcopy(2, 5300, 140, m0, 5, 7), rows), "centre": (5, 7)})
            # pads longer than the centre
            rows = [padcopy(0, 900 + 43 * j, 100 + j % 16, j & 1, a, b) for j, (a, b) in
                    enumerate((a, b) for a in (0, 99, 100, 101, 150) for b in (0, 99, 100, 101, 150) for _m in (0, 1))]
            out.append({"name": "pads_past_centre_%s" % "+-"[m0], "copies": _pad_candidates(win(2, 5600, 100, m0), rows)})
            # a centre that begins and ends in a run of N
            (L, _o, p), (L2, _o2, p2) = g["runs"][-3], g["runs"][-2]
            rows = [padcopy(0, 1300 + 47 * j, 100 + j % 16, j & 1, a, b) for j, (a, b) in
                    enumerate((a, b) for a in (0, 1, 16, 33, 40) for b in (0, 1, 16, 33, 40) for _m in (0, 1))]
            out.append({"name": "pads_n_centre_%s" % "+-"[m0], "copies": _pad_candidates(win(1, p, p2 + L2 - p, m0), rows)})
            # rows of > 1000: the first500 + last500 form cut from the padded window
            ab = [(a, 0) for a in (1, 499, 500, 501, 520)] + [(0, b) for b in (1, 499, 500, 501, 520)] + \
                 [(499, 499), (500, 500), (501, 501), (499, 501), (501, 499), (520, 520), (1200, 0), (0, 1200), (1200, 1200)]
            rows = [padcopy(0, 2000 + 1100 * (j % 30), n, j & 1, a, b) for j, (a, b, n) in
                    enumerate((a, b, n) for (a, b) in ab for n in (1001, 1016) for _m in (0, 1))]
            out.append({"name": "pads_trunc_%s" % "+-"[m0], "copies": _pad_candidates(win(2, 9000, 1100, m0), rows)})
        for c in out:
            c["cands"] = [DUMMY] * len(c["copies"])
        _cases["pads"] = out
    return _cases["pads"]


def pad_names():
    return [c["name"] for c in pad_cases()]


def check_pads(dev, name):
    compare(dev, [c for c in pad_cases() if c["name"] == name][0])


def selfcheck_pads():
    """every padded window differs from the unpadded one in the expected number of bytes: max(0, a - a0) + max(0, b - b0) pad bytes
    (lower case, or HITE_ROW_PAD where the centre has no such position), the bases between them untouched"""
    g = genome()
    ct = g["contigs"]
    seen, slots = set(), set()
    for c in pad_cases():
        bare = {"name": c["name"], "cands": c["cands"], "copies": [[cp[:5] + (0,) for cp in cps] for cps in c["copies"]]}
        tr = "trunc" in c["name"]
        pad, _t = twin_rows(ct, NAMES, c["cands"], c["copies"], FLANK, 1 if tr else 0)
        raw, _t = twin_rows(ct, NAMES, bare["cands"], bare["copies"], FLANK, 1 if tr else 0)
        a0, b0 = c.get("centre", (0, 0))
        for cps, pr, rr in zip(c["copies"], pad, raw):
            assert len(pr) == len(cps) == len(rr) and pr[0] == rr[0]                       # the centre is never padded
            m = len(pr[0][1])
            for cp, x, y in zip(cps[1:], pr[1:], rr[1:]):
                a, b = front_back(cp)
                a, b = max(0, a - a0), max(0, b - b0)
                w = x[1].decode()
                assert len(w) == len(y[1]) + a + b and w[a:len(w) - b] == y[1].decode()
                assert sum(1 for ch in w if ch not in "ACGTN") == a + b
                assert all(ch == "." for ch in w[m:a]) and all(ch == "." for ch in w[len(w) - b:len(w) - b + max(0, b - m)])
                seen.add((cp[3], cps[0][3]))
                slots.add(a % 16)
                if "n_centre" in c["name"] and a:
                    assert w[0] == "n"
                if "n_centre" in c["name"] and b:
                    assert w[-1] == "n"
                if "past_centre" in c["name"] and (a > m or b > m):
                    assert "." in w
        if tr:
            cut, _t = twin_rows(ct, NAMES, c["cands"], c["copies"], FLANK, 0)
            where = set()
            for cps, pr, cr in zip(c["copies"], pad, cut):
                for cp, x, z in zip(cps, pr, cr):
                    assert z[2] and z[1] == x[1][:500] + x[1][-500:]
                    a, b = front_back(cp)
                    n = len(x[1]) - a - b
                    where.add(("first half", "pad only" if a >= 500 else "pad + bases" if a else "bases"))
                    where.add(("second half", "pad only" if b >= 500 else "bases + pad" if b else "bases"))
                    if a > 500 or b > 500:
                        where.add("a pad cut by the form")
                    assert n > 1000                                                         # (a row of the form has > 1000 bases: its halves never meet)
            assert len(where) == 7, where
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)} and slots == set(range(16))


# ------------------------------------------------------------------------------------------------------------------------------
# clip_probe_kernel
# ------------------------------------------------------------------------------------------------------------------------------
def probe_end(q, y, right, att):
    """(fewest mismatches, its smallest offset, largest offset tried) of one attempt of one end, or None when the attempt cannot run:
    the definition in the header of orc_clip_probe restated with python strings"""
    q, y = q.upper(), y.upper()
    Lq, Ly, sh = len(q), len(y), att * CLIP_K
    if Ly < CLIP_K or Lq < CLIP_K or Ly < sh + CLIP_K:
        return None
    dm = min(Lq // 20 + 32, Lq - CLIP_K, 0xffff, Lq - CLIP_K - sh)
    if dm < 0:
        return None
    best, arg = CLIP_K + 1, 0
    for d in range(dm + 1):
        mm = 0
        for i in range(CLIP_K):
            a = q[Lq - d - sh - CLIP_K + i] if right else q[d + sh + i]
            b = y[Ly - sh - CLIP_K + i] if right else y[sh + i]
            mm += not (a == b and a in "ACGT")
        if mm < best:
            best, arg = mm, d
    return best, arg, dm


def _mutate(s, positions):
    s = list(s)
    for p in positions:
        s[p] = _other(s[p]) if s[p] in "ACGT" else "A"
    return "".join(s)


def probe_cases():
    """[(label, candidate, record, (left, right) in the candidate's orientation or None, what the case must show)] -- every record on
    both strands; the interval Y is read from the genome, the candidate is built around it"""
    if "probe" not in _cases:
        g = genome()
        ct = g["contigs"]
        rng = np.random.default_rng(8026)
        out = []
        slot = [0]

        def interval(n, ci=0, at=None):
            """a fresh interval of n bases -> records (plus, minus) with the interval as each reads it"""
            if at is None:
                at = 1000 + 760 * slot[0]
                slot[0] += 1
                assert at + n + 60 < clen(0)
            recs = []
            for mn in (0, 1):
                rec = (ci, at + 1, at + n, mn)
                recs.append((rec, OP._interval(ct[ci], at + 1, at + n, mn).decode()))
            return recs

        def add(label, n, build, expect, show=None, show_minus="same", expect_minus=None, **kw):
            for rec, y in interval(n, **kw):
                out.append((label + "+-"[rec[3]], build(y), rec, expect_minus if rec[3] and expect_minus else expect,
                            show_minus if rec[3] and show_minus != "same" else show))

        r = lambda n: rand_seq(rng, n)  # noqa: E731
        for n in (20, 21, 22, 41, 42, 43):
            add("cand_len_%d" % n, n, lambda y: y, (0, 0))
            pre, post = r(5), r(5)
            for rec, y in interval(50):
                rec2 = (rec[0], rec[1], rec[1] + n - 1, 0) if not rec[3] else (rec[0], rec[2] - n + 1, rec[2], 1)
                out.append(("interval_len_%d%s" % (n, "+-"[rec[3]]), pre + y + post, rec2, (5, 55 - n) if n >= CLIP_K else (0, 0), None))
        # exactly 5 / 6 mismatches at the best offset; a net insertion of 3 in the candidate tells the fall-back from a found offset
        pre, mid, post = r(10), r(3), r(7)
        mk = lambda pos: (lambda y: pre + _mutate(y[:50], pos) + mid + y[50:] + post)  # noqa: E731
        add("mismatch_5", 100, mk([0, 4, 9, 15, 20]), (10, 7), ("first", 0, 5))
        add("mismatch_6", 100, mk([0, 4, 9, 12, 15, 20]), (10, 7), ("first", 0, 6))
        add("mismatch_6_6", 100, mk([0, 4, 9, 12, 15, 20, 21, 25, 30, 33, 37, 41]), (13, 7), ("both", 0, 6))
        # ... and where nothing else can find the offset: an interval of 41 bases has no second attempt, and 3 bases more in the
        # candidate (between the two probes, which share base 20) make the fall-back say 7 where the offset is 4
        pre4, mid3 = r(4), r(3)
        only = lambda f: (lambda y: pre4 + f(y[:21]) + mid3 + y[21:])  # noqa: E731
        add("mismatch_5_only", 41, only(lambda p: _mutate(p, [0, 4, 9, 15, 19])), (4, 0), ("only", 0, 5))
        add("mismatch_6_only", 41, only(lambda p: _mutate(p, [0, 4, 9, 12, 15, 19])), (7, 0), ("only", 0, 6))
        # two offsets with equal mismatch counts: the smaller wins
        add("tie_left", 80, lambda y: y[:21] + y[:21] + y[21:], (0, 0), ("tie", 0, 0))
        add("tie_left_2mm", 80, lambda y: _mutate(y[:21], [3, 17]) + _mutate(y[:21], [5, 11]) + y[21:], (0, 0), ("tie", 0, 2))
        add("tie_right", 80, lambda y: y[:59] + y[59:] + y[59:], (0, 0), ("tie", 1, 0))
        # an indel inside the first 21 bases: only the second attempt finds the offset; an interval of 41 has no second attempt
        pre, ins = r(10), r(4)
        add("second_attempt", 90, lambda y: pre + y[:10] + y[11:60] + ins + y[60:], (9, 0), ("second", 0))      # (the fall-back would say 13)
        post = r(5)
        add("second_attempt_41", 41, lambda y: pre + y[:10] + y[11:] + post, (9, 5), ("none", 0))
        # the true offset at the last offset tried and one beyond it
        for Lq, d, exp in ((53, 32, (32, 0)), (54, 33, (33, 0)), (55, 34, (34, 0)), (56, 35, (34, 0))):
            pre = r(d)
            add("bound_%d_%d" % (Lq, d), Lq - d, lambda y: pre + y, exp, ("bound", 0, d))
        pre67, pre68 = r(67), r(68)
        add("bound_700_67", 633, lambda y: pre67 + y, (67, 0), ("bound", 0, 67))
        add("bound_700_68", 632, lambda y: pre68 + y, (67, 0), ("bound", 0, 68))
        # the alphabet
        pre = r(4)
        nn = lambda y, pos: "".join("N" if i in pos else ch for i, ch in enumerate(y))  # noqa: E731
        add("n_in_cand_5", 60, lambda y: pre + _mutate(nn(y, (2, 8, 14)), [5, 11]), (4, 0), ("first", 0, 5))
        add("n_in_cand_6", 60, lambda y: pre + _mutate(nn(y, (2, 8, 14)), [5, 11, 17]), (4, 0), ("first", 0, 6))
        (L1, _o, p1), (L15, _o15, p15) = g["runs"][3], g["runs"][len(RUN_OFFS) + 5]
        assert L1 == 1 and L15 == 15
        add("n_in_interval", 60, lambda y: pre + y.replace("N", "A"), (4, 0), ("first", 0, 1), ("first", 1, 1), ci=1, at=p1 - 3)
        add("n_in_interval_15", 80, lambda y: pre + y.replace("N", "C"), (4, 0), ("first", 0, 15), ("first", 1, 15), ci=1, at=p15 - 6)
        add("n_in_both", 60, lambda y: pre + _mutate(y, [k for k in (0, 6, 9, 13, 19, 20) if y[k] != "N"][:5]), (4, 0), ("first", 0, 6), ("first", 1, 1), ci=1, at=p1 - 3)
        add("lower_case", 60, lambda y: (pre + y).lower(), (4, 0))
        nn21 = lambda p, pos: "".join("N" if i in pos else ch for i, ch in enumerate(p))  # noqa: E731
        add("n_in_cand_5_only", 41, only(lambda p: _mutate(nn21(p, (2, 8, 14)), [5, 11])), (4, 0), ("only", 0, 5))
        add("n_in_cand_6_only", 41, only(lambda p: _mutate(nn21(p, (2, 8, 14)), [5, 11, 17])), (7, 0), ("only", 0, 6))
        # N in both at the same probe position is a mismatch: with 5 more the offset is not found (on the minus strand the N lies in
        # the other probe, which finds its offset with it)
        add("n_in_both_only", 41, only(lambda p: _mutate(p, [k for k in (0, 6, 9, 13, 17, 19) if p[k] != "N"][:5])), (7, 0), ("only", 0, 6), None,
            expect_minus=(4, 0), ci=1, at=p1 - 3)
        # one end found and the other not: the rest of the length difference, clamped at 0; neither end found
        junk = r(21)
        add("fallback_clamp_0", 100, lambda y: y[:40] + junk, (0, 0), ("none", 1))
        junk80 = r(80)
        add("neither_end", 100, lambda y: junk80, (0, 0), ("none", 0))
        # records clamped at the contig ends; no such contig
        n3 = clen(3)
        out.append(("clamped_start", ct[2][:60], (2, -5, 60, 0), (0, 0), None))
        out.append(("clamped_start-", revcomp(ct[2][:60]), (2, -5, 60, 1), (0, 0), None))
        out.append(("clamped_end", ct[3][n3 - 60:], (3, n3 - 59, n3 + 9, 0), (0, 0), None))
        out.append(("clamped_end-", revcomp(ct[3][n3 - 60:]), (3, n3 - 59, n3 + 9, 1), (0, 0), None))
        out.append(("no_contig", DUMMY, (9, 100, 200, 0), (0, 0), None))
        out.append(("no_contig-", DUMMY, (-1, 100, 200, 1), (0, 0), None))
        _cases["probe"] = out
    return _cases["probe"]


def probe_batches():
    """the probe records as candidates of one record each behind a candidate of 127 / 128 / 129 records (the two ends of record k are
    lanes 2 k and 2 k + 1, which exchange their offsets: 128 records fill a block of 256 threads, so the records under test begin on
    the last pair of the first block, on the first pair of the second, and one pair into it), the last batch with an odd record count;
    then the planted family, whose probed words pad the rows"""
    pc = probe_cases()
    fam = family_case()
    out = []
    for k in (127, 128, 129):
        at = 9000
        filler = [(2, at + 1, at + 80, 0)] * k
        cands = [genome()["contigs"][2][at:at + 80]] + [c[1] for c in pc] + fam["cands"]
        copies = [filler] + [[c[2]] for c in pc] + fam["copies"]
        if (sum(len(c) for c in copies) & 1) == 0 and k == 129:
            copies[0] = filler + filler[:1]
        out.append({"name": "probe_after_%d" % k, "cands": cands, "copies": copies})
    return out


FAM_CLIPS = ((0, 0), (3, 0), (0, 9), (17, 5), (16, 16), (33, 2), (1, 31), (40, 40))


def family_case():
    """the planted family: record i covers the family less FAM_CLIPS[i] at its ends (odd i on the minus strand)"""
    fam = genome()["family"]
    cps = []
    for i, (a, b) in enumerate(FAM_CLIPS):
        at = FAM_AT + FAM_STEP * i
        lo, hi = (at + b, at + FAM_LEN - a) if i % 2 else (at + a, at + FAM_LEN - b)
        cps.append((2, lo + 1, hi, i % 2))
    return {"name": "family", "cands": [fam], "copies": [cps]}


def check_probe(dev):
    """hite_clip_probe against the twin, then the rows of the same tables with the words probed (4-tuples: clip == NULL)"""
    g = use(dev)
    for b in probe_batches():
        got = dev.clip_probe(b["cands"], b["copies"])
        exp = twin_clips(g["contigs"], b["cands"], b["copies"])
        assert got == exp, (b["name"], [(k, x, y) for k, (x, y) in enumerate(zip(got, exp)) if x != y][:5])
    compare(dev, probe_batches()[2])
    compare(dev, family_case())


def selfcheck_probe():
    g = genome()
    ct = g["contigs"]
    shown = set()
    for label, cand, rec, expect, show in probe_cases():
        w = twin_clips(ct, [cand], [[rec]])[0][0]
        l, r = (w >> 16, w & 0xffff) if rec[3] else (w & 0xffff, w >> 16)       # back to the candidate's orientation
        assert (l, r) == expect, (label, (l, r), expect)
        if show is None or not 0 <= rec[0] < len(ct):
            continue
        y = OP._interval(ct[rec[0]], rec[1], rec[2], rec[3]).decode()
        kind, right = show[0], show[1]
        a0, a1 = probe_end(cand, y, right, 0), probe_end(cand, y, right, 1)
        if kind == "first":           # the first attempt's best offset has exactly show[2] mismatches
            assert a0[0] == show[2] and (a0[0] <= CLIP_MM or (a1 and a1[0] <= CLIP_MM)), (label, a0, a1)
        elif kind == "only":          # ... and there is no second attempt
            assert a0[0] == show[2] and a1 is None, (label, a0, a1)
        elif kind == "both":
            assert a0[0] == show[2] and a1[0] == show[2], (label, a0, a1)
        elif kind == "tie":
            q = cand.upper()
            at = [d for d in range(a0[2] + 1) if sum(1 for i in range(CLIP_K) if (q[len(q) - d - CLIP_K + i] if right else q[d + i]) !=
                                                     (y[len(y) - CLIP_K + i] if right else y[i])) == a0[0]]
            assert a0[0] == show[2] and len(at) >= 2 and a0[1] == at[0] == 0, (label, a0, at)
        elif kind == "second":
            assert a0[0] > CLIP_MM and a1[0] <= CLIP_MM and a1[1] == expect[0], (label, a0, a1)
        elif kind == "none":
            assert a0[0] > CLIP_MM and (a1 is None or a1[0] > CLIP_MM), (label, a0, a1)
        elif kind == "bound":
            d = show[2]
            assert (a0[2] == d and a0[0] == 0 and a0[1] == d) or (a0[2] == d - 1 and a0[0] > CLIP_MM and (a1 is None or a1[0] > CLIP_MM)), (label, a0, a1)
            shown.add("at the bound" if a0[2] == d else "one beyond")
        shown.add(kind)
    assert shown == {"first", "only", "both", "tie", "second", "none", "bound", "at the bound", "one beyond"}, shown
    assert {len(c[1]) for c in probe_cases()} >= {20, 21, 22, 41, 42, 43, 53, 54, 55, 56, 700}
    # the family: the probed words are the clips it was built with, and they pad the rows
    f = family_case()
    ws = twin_clips(ct, f["cands"], f["copies"])[0]
    assert [((w >> 16, w & 0xffff) if i % 2 else (w & 0xffff, w >> 16)) for i, w in enumerate(ws)] == list(FAM_CLIPS)
    rows, _t = twin_rows(ct, NAMES, f["cands"], f["copies"], FLANK, 0)
    assert [sum(1 for ch in x[1].decode() if ch not in "ACGTN") for x in rows[0]] == [0] + [a + b for a, b in FAM_CLIPS[1:]]
    nrec = [sum(len(c) for c in b["copies"]) for b in probe_batches()]
    assert [len(b["copies"][0]) for b in probe_batches()][:2] == [127, 128] and nrec[2] % 2 == 1 and min(nrec) > 128


# ------------------------------------------------------------------------------------------------------------------------------
# independence of the candidates of a batch; the thinned end-to-end set
# ------------------------------------------------------------------------------------------------------------------------------
def independence_cases():
    return [case_select(), case_modes()] + [c for c, _n in tie_cases()] + pad_cases()


def check_independence(dev, part, parts):
    """every candidate searched alone, and the batch in reverse candidate order, give the rows the candidate has in its batch"""
    g = use(dev)
    for c in independence_cases()[part::parts]:
        fl = c.get("flank", FLANK)
        for p in (0, 1):
            exp, _t = twin_rows(g["contigs"], NAMES, c["cands"], c["copies"], fl, p)
            got, _t = dev.fine_rows(c["cands"][::-1], c["copies"][::-1], flank=fl, rows_pass=p)
            assert got[::-1] == exp, (c["name"], p, "reversed")
            for k in range(len(c["cands"])):
                got, tot = dev.fine_rows([c["cands"][k]], [c["copies"][k]], flank=fl, rows_pass=p)
                assert got == [exp[k]], (c["name"], p, k)
                assert tot[0] == len(exp[k]) and tot[2] == max([len(x[1]) for x in exp[k]] + [0])


def e2e_tables(te_type):
    """at most 12 candidates per type out of the padded and the tie cases"""
    k = ("tir", "helitron", "non_ltr").index(te_type)
    pool = [(c["cands"][i], c["copies"][i], c.get("flank", FLANK)) for c in pad_cases() + [t for t, _n in tie_cases()] for i in range(len(c["cands"]))]
    pick = [x for x in pool if x[2] == FLANK][k::3]
    step = max(1, len(pick) // 12)
    return pick[::step][:12]


def check_end_to_end(dev, te_type):
    """the stage's answers on the tables whose rows are under test, against fine_stage_candidate"""
    g = use(dev)
    tabs = e2e_tables(te_type)
    got, _stats = dev.flank_region_align(te_type, [t[0] for t in tabs], [t[1] for t in tabs], plant=1, flank=FLANK)
    for (cand, cps, _fl), r in zip(tabs, got):
        exp = OP.fine_stage_candidate(te_type, cand, cps, g["contigs"], plant=1, flank=FLANK, contig_names=NAMES)
        assert [r[0], r[1], r[2], r[3]] == exp, (te_type, r, exp)
    return len(tabs)


def cons_pool_table(seed=11):
    """~8 families (tests/synth_small.py) for the consensus pool of the stage (merge_calls_kernel, copy_cons_kernel): candidates that
    pass in pass A only, in both passes, that fail, and one without a copy -- shown by the twin"""
    import synth_small

    g = synth_small.make(seed, n_fam=8)
    rng = np.random.default_rng(seed)
    cands, copies = list(g["cands"]), [list(c) for c in g["copies"]]
    # a candidate that fails in pass A on first500 + last500 forms, one that fails on full windows, one without a copy
    for n in (1400, 300):
        cands.append(rand_seq(rng, n))
        copies.append([(int(rng.integers(0, 3)), at + 1, at + n, int(rng.integers(0, 2))) for at in (int(x) for x in rng.integers(1000, 100000, 12))])
    cands.append(rand_seq(rng, 200))
    copies.append([])
    kinds, exp = set(), []
    for cand, cps in zip(cands, copies):
        r = OP.fine_stage_candidate("tir", cand, cps, g["contigs"], plant=1)
        big = any(x[5] for x in OP.pass_records(cand, cps, g["contigs"], FLANK, None))
        kinds.add("no copy" if not cps else ("both passes" if big else "pass A only") if r[0] else ("fails in pass A" if big else "fails"))
        exp.append(r)
    assert kinds >= {"no copy", "both passes", "pass A only", "fails in pass A", "fails"}, kinds
    return {"contigs": g["contigs"], "cands": cands, "copies": copies, "expect": exp}
