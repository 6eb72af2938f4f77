"""Genomes and candidates for tests/test_hit_sort_chunk_cases.py and tests/test_gpu_hit_sort_chunks.py: the per-candidate sort of the
hits (hit_segsort_kernel of hite_amd/csrc/hite_copies.hip) at the places where its passes change shape, and its contig test on both
sides of the capacity of the contig table it keeps in LDS.  Built from the blocks and the model of tests/copy_limit_cases.py; seeded,
pure python + numpy; no GPU and no twin in this file.

A thread of the sort owns a chunk of E = ceil(n / NT) | 1 keys of a candidate's n hits (NT = 256 threads up to 4096 hits, 512 above),
counts its digits in registers and keeps the keys there (the LDS classes of at most 1984 / 4096 / 8192 hits, E <= 9 / 17 / 17), or walks
the chunk in batches of 16 keys (the global class, above 8192 hits).  The hit counts of the cases:
  2, 3                 the smallest ranges that are sorted at all (1 hit is sorted by nobody): one and two threads with a key
  255, 256, 257        E = 1 -> 1 -> 3 at 256 threads (256: every thread one key, none idle)
  1984, 1985           the border of the first class (2 x 1984 keys of LDS: four workgroups per compute unit) and the second
  3840, 3841           E = 15 -> 17 in the 4096 class: the longest chunk of the LDS classes, the count of ONE digit reaches 17
  7680, 7681           the same with 512 threads in the 8192 class
  15872, 15873         the global class, E = 31 -> 33: batches of 16 + 15, then 16 + 16 + 1
  20000                the global class, E = 41: batches of 16 + 16 + 9; 2000 copies, the occurrence limit
As hit_classes builds them: a unit of m minimizers in an array of copies 70 N apart (m hits per copy, every copy its own cluster), plus
one for a 15-mer of unique sequence behind the unit.  Every builder asserts its counts with the model.

The contig test of a hit that continues a run reads the genome's contig offsets from a table of HS_NCTG = 96 entries in LDS when the
nc + 1 offsets fit (nc <= 95 contigs), from global memory otherwise: genomes of 94, 95 and 96 contigs, short ones of unique
sequence and, ACROSS THE LAST TWO, a run of hits with diagonal steps of exactly TD that the contig end between them cuts in two
(dense_array_cut, smaller): a table without its last entries, or a search that misses the last contig, changes the clusters."""
import numpy as np

import copy_limit_cases as CL
import seed_limit_cases as SC
from copy_limit_cases import K, MAXCOPY, MAXOCC, MINANCH, model, rand_seq, unit

NT_SMALL, NT_LARGE = 256, 512            # threads of the classes up to 4096 hits / above
HS_FIRST = 1984                          # hits of the largest range of the first class
HS_BATCH = 16                            # keys per batch of the global class
HS_NCTG = 96                             # entries of the contig table in LDS
LDS_CONTIGS = HS_NCTG - 1                # contigs whose nc + 1 offsets fit


def chunk(n):
    """E of a range of n hits"""
    nt = NT_SMALL if n <= CL.HS_MID else NT_LARGE
    return ((n + nt - 1) // nt) | 1


CASES = {}
_memo = {}


def case(fn):
    CASES[fn.__name__] = fn
    return fn


def names():
    return list(CASES)


def get(name):
    if name not in _memo:
        c = CASES[name]()
        c["name"] = name
        c.setdefault("aligned", True)
        c["alone"] = list(range(len(c["cands"])))
        _memo[name] = c
    return _memo[name]


def all_cases():
    return [(n, get(n)) for n in names()]


def _counts(seed, spec):
    """spec: [(m, ulen, copies, extra)] -> a case with, per entry, a candidate of m * copies hits (the unit, in an array of `copies`
    copies 70 N apart in a contig of its own) and, if extra, a second one of m * copies + 1 (unit + N + a 15-mer that is a minimizer
    of the last contig, which is unique sequence)"""
    rng = np.random.default_rng(seed)
    uniq = rand_seq(rng, 3000)
    vs = [uniq[p:p + K] for p, _hs, _w in SC.minimizers(uniq)[20:20 + 20 * len(spec):20]]
    contigs, cands, want, rows, clusters, chains = [], [], [], {}, 0, 0
    for (m, ulen, copies, extra), v in zip(spec, vs):
        assert copies <= MAXOCC
        u = unit(rng, ulen, m, both=False, also=(lambda x: len(SC.minimizers(x + "N" + v)) == m + 1) if extra else None)
        contigs.append(("N" * 70).join([u] * copies))
        rows[len(cands)] = min(copies, MAXCOPY) if m >= MINANCH else 0
        cands.append(u)
        want.append(m * copies)
        clusters += copies
        if extra:
            cands.append(u + "N" + v)
            want.append(m * copies + 1)
            clusters += copies + 1
        chains += (copies if m >= MINANCH else 0) * (2 if extra else 1)
    contigs.append(uniq)
    c = {"contigs": contigs, "cands": cands, "rows": rows, "hits": want, "stats": {"clusters": clusters, "chains": chains}}
    got = model(c)
    assert got["hits"] == want, (got["hits"], want)
    c["events"] = ["hits == %d" % h for h in want]
    return c


@case
def chunk_small():
    """2, 3, 255, 256 and 257 hits: the first class with one key, two keys, E = 1 with an idle thread, E = 1 with none, E = 3"""
    c = _counts(810, [(2, 30, 1, True), (5, 40, 51, False), (8, 60, 32, True)])
    assert [chunk(h) for h in c["hits"]] == [1, 1, 1, 1, 3]
    return c


@case
def chunk_mid():
    """1984 and 1985 hits (the last range of the first class and the first of the second), 3840 and 3841 (E = 15 -> 17 at 256 threads),
    7680 and 7681 (the same at 512 threads)"""
    c = _counts(811, [(8, 60, HS_FIRST // 8, True), (8, 60, 480, True), (8, 60, 960, True)])
    assert c["hits"][:2] == [HS_FIRST, HS_FIRST + 1] and [chunk(h) for h in c["hits"]] == [9, 9, 15, 17, 15, 17]
    return c


@case
def chunk_global():
    """15872 and 15873 hits (E = 31 -> 33: two batches, then three with a last one of ONE key) and 20000 hits (E = 41; 2000 copies of a
    unit of 10 minimizers: the occurrence limit): the global class in several batches per chunk"""
    c = _counts(812, [(8, 60, 1984, True), (10, 72, MAXOCC, False)])
    e = [chunk(h) for h in c["hits"]]
    assert e == [31, 33, 41] and [(x + HS_BATCH - 1) // HS_BATCH for x in e] == [2, 3, 3] and all(h > CL.HS_MEDIUM for h in c["hits"])
    return c


def _contigs(nc):
    """nc contigs: nc - 2 of 240 unique bases (one of them holds an element of 200 bases: the second candidate, one copy) and, in the
    last two, 100 copies of a unit of 54 bases and 8 minimizers 10 N apart, cut by the contig end between copy 50 and 51: the 8 hits of
    a copy share a diagonal and the next copy's lies exactly TD further, so the 800 hits are ONE run by strand and diagonal, and two
    clusters of 400 by the contig test alone"""
    u, arr = CL._array(740, 100, gap=10, m=8, ulen=54)
    rng = np.random.default_rng(820 + nc)
    el = rand_seq(rng, 200)
    contigs = [rand_seq(rng, 240) for _ in range(nc - 2)]
    contigs[nc // 2] = contigs[nc // 2][:20] + el + contigs[nc // 2][220:]
    half = 50 * 64
    contigs += [rand_seq(rng, 300) + "N" * 10 + arr[:half], arr[half:] + "N" * 10 + rand_seq(rng, 300)]
    assert len(contigs) == nc
    c = {"contigs": contigs, "cands": [u, el], "rows": {0: 0, 1: 1}, "hits": [800, None], "stats": {"clusters": 3, "chains": 1, "copies": 1}}
    index = CL.index_of(contigs)
    cl = CL.clusters_of(index, u)
    assert [(x["na"], x["contig"]) for x in cl] == [(400, nc - 2), (400, nc - 1)] and not any(x["span_ok"] for x in cl), cl
    one = CL.clusters_of(index, el)
    assert len(one) == 1 and one[0]["contig"] == nc // 2 and one[0]["na"] >= MINANCH and one[0]["span_ok"], one
    c["hits"][1] = one[0]["na"]
    assert model(c)["hits"] == c["hits"]
    c["events"] = ["%d contigs: %s" % (nc, "offsets in LDS" if nc + 1 <= HS_NCTG else "offsets in global memory"),
                   "a run of 800 hits cut by the end of contig %d" % (nc - 2)]
    return c


@case
def contigs_94():
    return _contigs(LDS_CONTIGS - 1)


@case
def contigs_95():
    return _contigs(LDS_CONTIGS)


@case
def contigs_96():
    return _contigs(LDS_CONTIGS + 1)


REQUIRED = (["hits == %d" % h for h in (2, 3, 255, 256, 257, 1984, 1985, 3840, 3841, 7680, 7681, 15872, 15873, 20000)] +
            ["94 contigs: offsets in LDS", "95 contigs: offsets in LDS", "96 contigs: offsets in global memory"] +
            ["a run of 800 hits cut by the end of contig %d" % k for k in (92, 93, 94)])


def coverage():
    ev = set()
    for n in names():
        ev.update(get(n)["events"])
    return ev


# ------------------------------------------------------------------------------------------------------------------------------
# checks shared by the CPU test (the twin's tables) and the GPU test (the device's, already compared with the twin's)
# ------------------------------------------------------------------------------------------------------------------------------
def check_closed_forms(name, table):
    """the rows per candidate the construction gives; `table`: per candidate list of (contig, start1, end1, minus, anchors, clip word)"""
    c = get(name)
    for k, n in c["rows"].items():
        assert len(table[k]) == n, (name, k, len(table[k]), n)


def check_stats(name, stats):
    """stats = copy_stats_ext() of the whole case: hits == the model's, and the closed forms of clusters, copies before the cap, chains"""
    c = get(name)
    assert stats[1] == sum(c["hits"]), (name, stats, sum(c["hits"]))
    got = {"clusters": stats[2], "copies": stats[3], "chains": stats[4] + stats[5]}
    for k, v in c["stats"].items():
        assert got[k] == v, (name, k, got[k], v)


def check_alone(name, k, stats):
    """copy_stats_ext() of candidate k searched alone"""
    c = get(name)
    assert stats[1] == c["hits"][k], (name, k, stats, c["hits"][k])
