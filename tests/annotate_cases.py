"""TEST INFRASTRUCTURE: labelled inputs of the genome annotation (hite_annotate; include/hite_gpu.h, "genome annotation"), the
smallest at which each step of the definition can go wrong, each with the closed form of what it must reach.  A case is a dict: label,
seqs, lib, piece_len, stats (the closed form of some counters), records (the closed form of the result, or None), status (or None).
tests/test_annotate_cases.py holds the twin to the closed forms and the two forms of the twin to each other;
tests/test_gpu_annotate.py holds the HIP code to the twin on every case."""
import functools

import numpy as np

import annotate_twin as AT

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def rand(rng, n):
    return rng.integers(0, 4, size=int(n)).astype(np.uint8)


def text(*parts):
    return b"".join(ACGT[p].tobytes() if isinstance(p, np.ndarray) else p for p in parts).decode()


def revcomp(c):
    return (3 - c[::-1]).astype(np.uint8)


def changed(c, keep=()):
    """every base replaced by the next one, but for the ranges [a, b) of keep"""
    s = ((c + 1) & 3).astype(np.uint8)
    for a, b in keep:
        s[a:b] = c[a:b]
    return s


def sparse(c, core):
    """exact in the range core = (a, b) and with every 11th base replaced elsewhere: no 13-base word outside the core, and an alignment
    that goes on to both ends (the first and the last five bases are kept)"""
    s = c.copy()
    k = np.arange(len(c))
    m = sparse_mask(len(c), core)
    s[m] = (s[m] + 1) & 3
    return s


def sparse_mask(n, core):
    k = np.arange(n)
    return (k % 11 == 5) & ((k < core[0]) | (k >= core[1])) & (k >= 5) & (k < n - 5)


def sparse_hits(n, core):
    """the hits of sparse(): the words inside the exact stretch around the core"""
    at = np.flatnonzero(sparse_mask(n, core))
    return int(at[at >= core[1]].min() - at[at < core[0]].max() - 1 - 12)


def case(label, seqs, lib, stats=None, records=None, status=None, piece_len=0):
    return dict(label=label, seqs=list(seqs), lib=list(lib), piece_len=piece_len, stats=dict(stats or {}), records=records, status=status)


def full(seq, g, L, lib=0, strand=0):
    """the record of an exact copy of a whole entry of L bases at g"""
    return (seq, g, g + L, lib, strand, 0, L, 2 * L, L, L)


# ---- step 1: the table -----------------------------------------------------------------------------------------------------------
def table_cases():
    rng = np.random.default_rng(11)
    out = []
    w = rand(rng, 13)
    for n in (AT.MAX_OCC, AT.MAX_OCC + 1):
        # the bases beside the word: A in the genome, another one in every entry, so that no word but this one is shared
        lib = [text(rand(rng, 13), rng.integers(1, 4, size=1).astype(np.uint8), w, rng.integers(1, 4, size=1).astype(np.uint8), rand(rng, 13))
               for _ in range(n)]
        genome = text(rand(rng, 700), b"A", w, b"A", rand(rng, 700))
        out.append(case("a word with %d table entries" % n, [genome], lib,
                        dict(table=n * 2 * 29, silenced=0 if n == AT.MAX_OCC else 2 * n, hits=n if n == AT.MAX_OCC else 0, runs=0, records=0), []))
    a, b, c = rand(rng, AT.MAX_LIB_LEN), rand(rng, AT.MAX_LIB_LEN + 1), rand(rng, 300)
    genome = text(rand(rng, 480), changed(a[980:1000]), a[1000:1500], changed(a[1500:1520]), rand(rng, 280), b[2000:2500], rand(rng, 300), c,
                  rand(rng, 400))
    out.append(case("entries of MAX_LIB_LEN and MAX_LIB_LEN + 1 bases", [genome], [text(a), text(b), text(c)],
                    dict(too_long=1, table=2 * (AT.MAX_LIB_LEN - 12) + 2 * 288, records=2),
                    [(0, 500, 1000, 0, 0, 1000, 1500, 1000, 500, 500), full(0, 2100, 300, lib=2)], [0, -1, 0]))
    out.append(case("only an entry that is too long", [genome], [text(b)], dict(too_long=1, table=0, hits=0, records=0), [], [-1]))
    out.append(case("no entry", [genome], [], dict(table=0, hits=0, records=0), [], []))
    out.append(case("entries shorter than a word", [genome], ["ACGTACGTACGT", "", text(c)], dict(table=2 * 288, records=1), [full(0, 2100, 300, lib=2)],
                    [0, 0, 0]))
    return out


# ---- steps 2 and 3: hits and runs ------------------------------------------------------------------------------------------------
def run_cases():
    rng = np.random.default_rng(12)
    out = []
    e = rand(rng, 400)
    for n in (AT.MIN_HITS - 1, AT.MIN_HITS):      # n hits: n + 12 exact bases
        genome = text(rand(rng, 500), changed(e, [(100, 100 + n + 12)]), rand(rng, 500))
        out.append(case("a chain of %d hits" % n, [genome], [text(e)], dict(hits=n, runs=0 if n < AT.MIN_HITS else 2, hsps=0, records=0), []))
    for gap in (AT.GAP, AT.GAP + 1):               # two stretches of 3 hits, the first hit of the second `gap` after the last of the first
        genome = text(rand(rng, 500), changed(e, [(20, 35), (22 + gap, 37 + gap)]), rand(rng, 500))
        out.append(case("a gap of %d between two hits" % gap, [genome], [text(e)], dict(hits=6, runs=2 if gap == AT.GAP else 4, records=0), []))
    # diagonals 703 = 64 * 10 + 63 and 704: two bins on lattice 0, one on lattice 32
    genome = text(rand(rng, 703), changed(e[:150], [(100, 114)]), rand(rng, 1), changed(e[150:], [(0, 14)]), rand(rng, 400))
    out.append(case("a diagonal step across a bin edge of lattice 0", [genome], [text(e)], dict(hits=4, runs=1, alignments=1), None))
    genome = text(rand(rng, 720), changed(e[:150], [(100, 114)]), rand(rng, 1), changed(e[150:], [(0, 14)]), rand(rng, 400))
    out.append(case("the same step inside a bin of both lattices", [genome], [text(e)], dict(hits=4, runs=2, alignments=2), None))
    r = rand(rng, 300)
    for lead, label in ((720, "an exact copy in the middle of a bin: both lattices find it"), (703, "an exact copy on the last diagonal of a bin")):
        out.append(case(label, [text(rand(rng, lead), r, rand(rng, 500))], [text(r)],
                        dict(hits=288, runs=2, alignments=2, redos=0, hsps=2, duplicates=1, dominated=0, records=1), [full(0, lead, 300)], [0]))
    out.append(case("a copy of the reverse complement", [text(rand(rng, 600), revcomp(r), rand(rng, 500))], [text(r)],
                    dict(hits=288, hsps=2, duplicates=1, records=1), [full(0, 600, 300, strand=1)]))
    half = rand(rng, 150)
    pal = np.concatenate([half, revcomp(half)])
    out.append(case("an entry that is its own reverse complement", [text(rand(rng, 600), pal, rand(rng, 500))], [text(pal)],
                    dict(hits=2 * 288, hsps=4, duplicates=2, dominated=1, records=1), [full(0, 600, 300)]))
    g = text(rand(rng, 600), r, rand(rng, 500))
    out.append(case("lower-case genome and library", [g.lower()], [text(r).lower()], dict(hits=288, records=1), [full(0, 600, 300)]))
    gn = g[:700] + "N" + g[701:]
    out.append(case("another byte inside the copy", [gn], [text(r)], dict(hits=288 - 13, records=1), [(0, 600, 900, 0, 0, 0, 300, 2 * 299 - 4, 299, 300)]))
    ln = text(r)[:100] + "n" + text(r)[101:]
    out.append(case("another byte inside the entry", [g], [ln], dict(table=2 * (288 - 13), hits=288 - 13, records=1),
                    [(0, 600, 900, 0, 0, 0, 300, 2 * 299 - 4, 299, 300)]))
    return out


# ---- step 4: pads and spans ------------------------------------------------------------------------------------------------------
def pad_cases():
    rng = np.random.default_rng(13)
    out = []
    for L, redos in ((600, 1), (2500, 2), (9000, 3)):      # the core of 40 bases seeds; the pads grow until the window holds the copy
        e = rand(rng, L)
        core = (L // 2 - 20, L // 2 + 20)
        mism = int(sparse_mask(L, core).sum())
        genome = text(rand(rng, 1000), sparse(e, core), rand(rng, 1000))
        out.append(case("a copy of %d bases seeded in its middle: pad level %d" % (L, redos), [genome], [text(e)],
                        dict(runs=2, alignments=2 * (redos + 1), redos=2 * redos, hsps=2, records=1, **({"hits": sparse_hits(L, core)} if L < 5000 else {})),
                        [(0, 1000, 1000 + L, 0, 0, 0, L, 2 * (L - mism) - 4 * mism, L - mism, L)]))
    e = rand(np.random.default_rng(131), 20000)
    core = (10000 - 20, 10000 + 20)
    genome = text(rand(rng, 700), sparse(e, core), rand(rng, 700))
    out.append(case("a copy of 20 000 bases seeded in its middle: the last pad does not reach its ends", [genome], [text(e)],
                    dict(runs=2, alignments=8, redos=6, records=1), None))
    genome = text(rand(rng, 700), e, rand(rng, 700))
    # chains of the hits 0 .. 8191, 8192 .. 16383, 16384 .. 19987 on each lattice: six HSPs; the window of the second holds the whole copy
    # (20 000 random bases repeat some 15 of their own: the runs of those give no HSP and are not counted here)
    out.append(case("an exact copy of 20 000 bases: chains closed at MAX_SPAN", [genome], [text(e)],
                    dict(hsps=6, duplicates=3, dominated=2, records=1), [full(0, 700, 20000)]))
    r = rand(rng, 300)
    out.append(case("a copy at each end of a sequence", [text(r, rand(rng, 900), r)], [text(r)], dict(hits=2 * 288, redos=0, records=2),
                    [full(0, 0, 300), full(0, 1200, 300)]))
    out.append(case("empty and short sequences beside one with a copy", ["", "ACGTACGTACGT", text(rand(rng, 100), r, rand(rng, 100)), ""], [text(r)],
                    dict(hits=288, records=1), [full(2, 100, 300)]))
    out.append(case("no sequence", [], [text(r)], dict(table=2 * 288, hits=0, records=0), [], [0]))
    out.append(case("only sequences shorter than a word", ["ACGT", ""], [text(r)], dict(hits=0, records=0), []))
    a, b = rand(rng, 400), rand(rng, 350)
    out.append(case("copies in three sequences", [text(rand(rng, 300), a, rand(rng, 40), revcomp(b)), text(b, rand(rng, 500)),
                                                  text(rand(rng, 20), revcomp(a))], [text(a), text(b)], dict(records=4),
                    [full(0, 300, 400), full(0, 740, 350, lib=1, strand=1), full(1, 0, 350, lib=1), full(2, 20, 400, strand=1)]))
    return out


# ---- steps 2 and 5: pieces, the resolve ------------------------------------------------------------------------------------------
def piece_cases():
    rng = np.random.default_rng(14)
    out = []
    r = rand(rng, 600)
    genome = text(rand(rng, 3900), r, rand(rng, 7500))      # 12 000 bases, the copy across 4 096
    # pieces [0, 12000), [4096, 12000), [8192, 12000): the second holds the hits 4096 .. 4487 of the copy, its run grows to the same record
    out.append(case("a copy across a piece edge", [genome], [text(r)], dict(runs=4, hsps=4, duplicates=3, records=1),
                    [full(0, 3900, 600)], piece_len=4096))
    out.append(case("the same genome in one piece", [genome], [text(r)], dict(runs=2, hsps=2, duplicates=1, records=1), [full(0, 3900, 600)]))
    x = rand(rng, 1000)
    for extra, label in ((100, "80"), (105, "79")):         # B = the last 500 - extra bases of X and `extra` more: 400 / 395 of its 500 under A
        y = rand(rng, extra)
        genome = text(rand(rng, 1000), x, y, rand(rng, 800))
        b = np.concatenate([x[500 + extra:], y])
        kept = [full(0, 1000, 1000)] + ([] if extra == 100 else [full(0, 1000 + 500 + extra, 500, lib=1)])
        out.append(case("two entries on one locus, %s %% of the lesser under the better" % label, [genome], [text(x), text(b)],
                        dict(hsps=4, duplicates=2, dominated=1 if extra == 100 else 0, records=len(kept)), kept))
    return out


@functools.lru_cache(maxsize=None)
def small_cases():
    return table_cases() + run_cases() + pad_cases() + piece_cases()


# ---- planted truth ---------------------------------------------------------------------------------------------------------------
DIVERGENCES = (0.0, 0.05, 0.10, 0.15)


@functools.lru_cache(maxsize=None)
def planted(genome_len=2_000_000, n_entries=40, copies=8, seed=77):
    """a random genome with `copies` copies of each of n_entries entries of 300 .. 6 000 bases, at the divergences of DIVERGENCES in
    turn and on both strands, made with hite_amd.synth._mutate_copy -> (genome, lib, truth): truth rows (entry, strand, begin, end,
    divergence)"""
    from hite_amd import synth

    rng = np.random.default_rng(seed)
    lib = [rand(rng, int(rng.integers(300, 6001))) for _ in range(n_entries)]
    plan = [(e, k) for e in range(n_entries) for k in range(copies)]
    order = rng.permutation(len(plan))
    total = 0
    made = []
    for idx in order:
        e, k = plan[idx]
        div = DIVERGENCES[k % len(DIVERGENCES)]
        strand = (k // len(DIVERGENCES)) & 1
        c = synth._mutate_copy(rng, lib[e], div, div / 10)
        made.append((e, strand, div, revcomp(c) if strand else c))
        total += len(c)
    gaps = rng.multinomial(genome_len - total, np.ones(len(made) + 1) / (len(made) + 1))
    parts, truth, at = [], [], 0
    for (e, strand, div, c), gap in zip(made, gaps):
        parts.append(rand(rng, gap))
        at += int(gap)
        parts.append(c)
        truth.append((e, strand, at, at + len(c), div))
        at += len(c)
    parts.append(rand(rng, gaps[-1]))
    return text(*parts), [text(e) for e in lib], truth


def coverage(truth_row, recs):
    """the bases of a planted copy under records of its own entry and strand"""
    e, strand, begin, end, _div = truth_row
    mask = np.zeros(end - begin, dtype=bool)
    for r in recs:
        if r[3] == e and r[4] == strand and r[2] > begin and r[1] < end:
            mask[max(r[1], begin) - begin:min(r[2], end) - begin] = True
    return int(mask.sum())


@functools.lru_cache(maxsize=None)
def planted_twin():
    """the twin's (records, status, stats) on the planted genome, computed once"""
    genome, lib, _truth = planted()
    st = {}
    recs, status = AT.annotate([genome], lib, stats=st)
    return recs, status, st
