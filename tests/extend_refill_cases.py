"""Inputs for tests/test_gpu_extend_refill.py: small genomes on which chain_extend_kernel walks ends of chosen lengths.  The end
extension takes its bases from windows refilled 16 at a time (hite_ext.h), so the lengths sit around the multiples of 16 and at the
limits of the chain list (EXT_LONG) and of the extension (EXT_MAXLEN); the candidate bytes are read 16 at a time from cand_off + x, so
the candidates start at every offset mod 16; and a batch of over 1000 (chain, end) tasks of mixed lengths makes lanes take task after
task when the grid is capped (HITE_EXT_BLOCKS).  The ends are "worn" as in copy_limit_cases: a substitution every 14 bases leaves no
15-mer, so no anchor lies there and the extension has to align through."""
import numpy as np

import copy_limit_cases as CL
from copy_limit_cases import K, MINANCH, clusters_of, index_of, spaced, worn
from seed_limit_cases import rand_seq, revcomp

END_LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 383, 384, 2047, 2048)


def _worn_element(rng, n, upto):
    """(the element, the element worn below `upto`, the position of its first anchor when it is searched from base 10 on)"""
    for _try in range(50):
        X = rand_seq(rng, n)
        w = worn(rng, X, upto)
        cl = [x for x in clusters_of(index_of([spaced(rng, [X], 300)]), w[10:]) if x["rel"] == 0 and x["na"] >= MINANCH]
        if cl:
            return X, w, max(cl, key=lambda x: x["na"])["qlo"]
    raise AssertionError("no element")


def end_lengths():
    """one element of 2960 bases, a copy on each strand; per end length t a candidate whose outermost anchor lies t bases from its
    left end, and its reverse complement (the end on the right): against the two copies every candidate has a chain on each strand,
    so every length is walked to the left and to the right, forward and as reverse complement"""
    rng = np.random.default_rng(1801)
    X, w, q0 = _worn_element(rng, 2960, 2085)
    contigs = [spaced(rng, [X, revcomp(X)], 900)]
    index = index_of(contigs)
    cands, ends = [], {0: set(), 1: set()}
    for t in END_LENGTHS:
        # (which k-mers of the first window are minimizers depends on where the candidate begins: look for the beginnings that put
        # the outermost anchor of the chain of either strand at t)
        want = {0, 1}
        for s in range(10 + q0 - t, 10 + q0 - t - 40, -1):
            if s < 0 or not want:
                break
            q = w[s:]
            cl = [x for x in clusters_of(index, q) if x["na"] >= MINANCH]
            assert len(cl) == 2, (t, s, cl)
            hit = {x["rel"] for x in cl if (x["qlo"] if x["rel"] == 0 else len(q) - x["qhi"] - K) == t} & want
            if hit:
                want -= hit
                cands += [q, revcomp(q)]
                for x in cl:
                    ends[x["rel"]].add(x["qlo"] if x["rel"] == 0 else len(q) - x["qhi"] - K)
        assert not want, (t, want)
    assert ends[0] >= set(END_LENGTHS) and ends[1] >= set(END_LENGTHS), ends
    return {"contigs": contigs, "cands": cands, "aligned": True, "alone": []}


def cand_offsets():
    """34 candidates of 16 m + 1 bases each: cand_off runs through every value mod 16, twice; every candidate has a worn end of its own
    length on the left and another on the right, every other one is stored as reverse complement"""
    rng = np.random.default_rng(1802)
    n = 900
    for _try in range(50):
        Y = rand_seq(rng, n)
        t = list(worn(rng, Y, 120))
        for i in range(n - 118, n, 14):
            t[i] = CL.other_base(t[i])
        w = "".join(t)
        contigs = [spaced(rng, [Y, revcomp(Y)], 500)]
        index = index_of(contigs)
        cl = [x for x in clusters_of(index, w) if x["na"] >= MINANCH]
        if len(cl) == 2 and all(40 <= x["qlo"] <= 130 and 40 <= n - x["qhi"] - K <= 130 for x in cl):
            break
    else:
        raise AssertionError("no element")
    cands, off = [], []
    for k in range(34):
        a = k % 23                                              # bases cut from the left end
        L = (n - a - (k * 5) % 19) // 16 * 16 + 1               # and from the right, down to a length of 16 m + 1
        q = w[a:a + L]
        off.append(sum(len(c) for c in cands) % 16)
        cands.append(revcomp(q) if k % 2 else q)
    assert sorted(off[:16]) == list(range(16)) and sorted(off[16:32]) == list(range(16))
    return {"contigs": contigs, "cands": cands, "aligned": True, "alone": []}


def mixed_batch():
    """over 1000 tasks of mixed lengths: six families (two of 2960 bases with ends of up to 2048 to walk, four of 700..1100), eight
    copies each on either strand, some copies cut short so that the walk leaves the copy (x-drop) or meets the end of the contig; sixteen
    candidates per family with ends of 0..2048 bases"""
    rng = np.random.default_rng(1803)
    pieces, cands = [], []
    for f in range(6):
        n = 2960 if f < 2 else int(rng.integers(700, 1100))
        upto = 2085 if f < 2 else n // 2
        X, w, q0 = _worn_element(rng, n, upto)
        for c in range(8):
            cut = 0 if c < 5 else int(rng.integers(1, upto))    # a copy without its first `cut` bases
            p = X[cut:]
            pieces.append(revcomp(p) if c % 2 else p)
        lens = [int(x) for x in rng.integers(0, 10 + q0, size=14)] + [0, q0 + 10 if f >= 2 else 2048]
        for j, t in enumerate(lens):
            t = min(t, 10 + q0)
            q = w[10 + q0 - t:]
            cands.append(revcomp(q) if j % 3 == 0 else q)
    order = rng.permutation(len(pieces))
    half = len(pieces) // 2
    contigs = [spaced(rng, [pieces[i] for i in order[:half]], 400), "".join(pieces[i] + rand_seq(rng, 350) for i in order[half:])]
    return {"contigs": contigs, "cands": cands, "aligned": True, "alone": []}


def many_contigs():
    """120 contigs (the set-up of a task searches the contig of its chain and takes both ends of it for jmax): copies of a worn element
    that begin or end with their contig, so that both walks meet a contig end, between contigs of unique sequence"""
    rng = np.random.default_rng(1804)
    X, w, q0 = _worn_element(rng, 1200, 500)
    contigs = []
    for c in range(120):
        if c % 10 == 3:
            p = X[int(rng.integers(0, 400)):1200 - int(rng.integers(0, 200))]
            contigs.append(revcomp(p) if c % 20 == 3 else p)
        else:
            contigs.append(rand_seq(rng, int(rng.integers(60, 400))))
    cands = []
    for j, t in enumerate((0, 7, 16, 100, 333, 400, q0 + 10)):
        q = w[10 + q0 - min(t, q0 + 10):]
        cands.append(revcomp(q) if j % 2 else q)
    return {"contigs": contigs, "cands": cands, "aligned": True, "alone": []}


_memo = {}


def all_cases():
    """[(name, case)] in a fixed order, built once"""
    if not _memo:
        for fn in (end_lengths, cand_offsets, mixed_batch, many_contigs):
            _memo[fn.__name__] = fn()
        for c in _memo.values():
            assert sum(len(s) for s in c["contigs"]) <= 200_000
    return list(_memo.items())
