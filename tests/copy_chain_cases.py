"""Genomes and candidates for tests/test_gpu_copy_chains.py: the copy finder's path from the sorted hits of a candidate to its
chains (diagonal clusters -> runs -> extreme anchors -> chain filters), at the edges of the cluster rule and of the per-candidate
sort classes.  Seeded, pure numpy / python, in the style of synth_small; at most about 0.5 Mbp per genome.

Constants of the copy finder the cases are built around (hite_amd/csrc/hite_copies.hip)."""
import numpy as np

import casegen

K = 15              # k-mer length of the minimizers
TD = 64             # largest diagonal step inside a cluster
EXT_LONG = 384      # an end of at least this many bases beyond the outermost anchor makes a "long" chain


def minimizer_rank(kmer):
    """the value the copy finder orders the k-mers of a window by: a 32-bit mix of the smaller of the k-mer's and its reverse
    complement's 2-bit codes (first base in the lowest bits), without its lowest bit (hs_from_code, lowbias32)"""
    x = sum(casegen.BASES.index(ch) << (2 * i) for i, ch in enumerate(kmer))
    rc = sum((3 - casegen.BASES.index(ch)) << (2 * i) for i, ch in enumerate(reversed(kmer)))
    h = min(x, rc)
    h ^= h >> 16
    h = (h * 0x7feb352d) & 0xffffffff
    h ^= h >> 15
    h = (h * 0x846ca68b) & 0xffffffff
    h ^= h >> 16
    return h >> 1


class _Genome:
    def __init__(self, rng, lens):
        self.rng = rng
        self.ch = [list(casegen.rand_seq(rng, n)) for n in lens]
        self.used = [np.zeros(n, dtype=bool) for n in lens]

    def place(self, s, margin=80):
        """writes s at a free random place; -> (contig, 0-based position)"""
        rng = self.rng
        for _try in range(200):
            ci = int(rng.integers(0, len(self.ch)))
            n = len(self.ch[ci])
            pos = int(rng.integers(margin, n - len(s) - margin))
            if not self.used[ci][pos - margin:pos + len(s) + margin].any():
                self.used[ci][pos - margin:pos + len(s) + margin] = True
                self.ch[ci][pos:pos + len(s)] = list(s)
                return ci, pos
        raise AssertionError("genome too full")

    def free_stretch(self, n, margin=80):
        """a random stretch of n untouched bases, reserved; -> (contig, position, sequence)"""
        rng = self.rng
        for _try in range(200):
            ci = int(rng.integers(0, len(self.ch)))
            pos = int(rng.integers(margin, len(self.ch[ci]) - n - margin))
            if not self.used[ci][pos - margin:pos + n + margin].any():
                self.used[ci][pos - margin:pos + n + margin] = True
                return ci, pos, "".join(self.ch[ci][pos:pos + n])
        raise AssertionError("genome too full")

    def contigs(self):
        return ["".join(c) for c in self.ch]


def _plant_family(G, rng, cons, ncopy, div):
    for k in range(ncopy):
        s = casegen.mutate(rng, cons, div if k else 0.0)
        G.place(casegen.revcomp(s) if rng.integers(0, 2) else s)


def sort_classes(seed=5, copies=(5, 10, 20, 40)):
    """families of a 1.5 kb element with 5 / 10 / 20 / 40 copies (about 270 minimizers x copies hits: one candidate per class of the
    per-candidate sort, the global one included), and the candidates nobody sorts or that sort two or three hits: no valid k-mer,
    and genome snippets of 15 .. 75 bases from untouched sequence (a candidate has one window per 10 k-mers, or one in all when it has
    fewer: one minimizer that occurs once, then runs of exactly 2 and 3 hits and more as the snippets grow)"""
    rng = np.random.default_rng(seed)
    G = _Genome(rng, [150_000, 150_000, 120_000])
    cands = []
    for n in copies:
        cons = casegen.rand_seq(rng, 1500)
        _plant_family(G, rng, cons, n, 0.01)
        cands.append(cons)
    n_fam = len(cands)
    cands += ["ACGT" * 3, "N" * 100, "ACGTN" * 20]
    snip = []
    for L in range(K, 76):
        _ci, _pos, s = G.free_stretch(L)
        snip.append(casegen.revcomp(s) if L % 2 else s)
    return {"contigs": G.contigs(), "cands": cands + snip, "n_fam": n_fam, "first_snippet": len(cands)}


def cluster_edges(seed=6):
    """one 1.5 kb element; its copies carry ONE deletion or insertion between two anchor blocks, of TD - 1, TD and TD + 1 bases: the
    two blocks' diagonals differ by exactly that much, so TD joins them into one cluster and TD + 1 does not.  One more copy is split
    over a contig end: its halves have the same diagonal in the concatenated genome, and only the contig test cuts the run."""
    rng = np.random.default_rng(seed)
    cons = casegen.rand_seq(rng, 1500)
    head, tail = cons[:700], cons[700:]
    lens = [90_000, 90_000, 90_000]
    G = _Genome(rng, lens)
    # the split copy: contig 0 ends with the first 700 bases, contig 1 begins with the rest
    G.ch[0][lens[0] - len(head):] = list(head)
    G.used[0][lens[0] - len(head) - 200:] = True
    G.ch[1][:len(tail)] = list(tail)
    G.used[1][:len(tail) + 200] = True
    G.place(cons)
    for d in (TD - 1, TD, TD + 1):
        for minus in (False, True):
            dele = cons[:700] + cons[700 + d:]
            ins = cons[:700] + casegen.rand_seq(rng, d) + cons[700:]
            for s in (dele, ins):
                G.place(casegen.revcomp(s) if minus else s)
    return {"contigs": G.contigs(), "cands": [cons, casegen.revcomp(cons)]}


def one_cluster_and_singletons(seed=7):
    """a candidate that IS the only copy of its element (its whole range of hits is one diagonal: one cluster), and a candidate
    whose hits are all singletons: 15-base snippets (ONE k-mer each) of far-apart genome places on either strand, in shuffled order,
    so that no two hits share a strand and a diagonal within TD, with one base between them that keeps the k-mers across a border off
    both neighbours' diagonals.  A snippet gives a hit when its k-mer is a minimizer of the genome
    AND of the candidate: the k-mers taken are the smallest of the 19 around them in the genome, from the lowest fortieth of the hash
    range (the smallest of the candidate's 19 around them with probability 0.6)"""
    rng = np.random.default_rng(seed)
    G = _Genome(rng, [160_000, 160_000])
    _ci, _pos, single = G.free_stretch(1500)
    parts = []
    order = rng.permutation(110)
    for i in order:
        ci, lo = int(i) % 2, 3000 + 2800 * (int(i) // 2)
        contig = "".join(G.ch[ci][lo - 20:lo + 700])
        rank = [minimizer_rank(contig[p:p + K]) for p in range(len(contig) - K + 1)]
        for p in range(9, len(rank) - 9):
            if rank[p] < (1 << 31) // 40 and rank[p] == min(rank[p - 9:p + 10]) and not G.used[ci][lo - 20 + p:lo - 20 + p + K].any():
                s, before, after = contig[p:p + K], contig[p - 1], contig[p + K]
                if rng.integers(0, 2):
                    s, before, after = casegen.revcomp(s), casegen.revcomp(after), casegen.revcomp(before)
                parts.append((s, before, after))
                break
    # one base between two snippets, unlike the base the genome has behind the first and unlike the one it has in front of the
    # second: a k-mer that straddles a border then differs from the genome on either snippet's diagonal
    cand = ""
    for k, (s, _before, after) in enumerate(parts):
        nxt = parts[k + 1][1] if k + 1 < len(parts) else after
        cand += s + next(b for b in casegen.BASES if b != after and b != nxt)
    return {"contigs": G.contigs(), "cands": [single, cand]}


def long_end(seed=8, step=14):
    """a 1.6 kb element with several copies; the candidate's first 400 bases carry a substitution every `step` bases (no 15-mer
    survives, the end extension still aligns through them): its chains have >= EXT_LONG bases beyond the outermost anchor on one
    side -- they are listed from the front of the chain table -- while the intact candidate's chains are listed from the back"""
    rng = np.random.default_rng(seed)
    cons = casegen.rand_seq(rng, 1600)
    G = _Genome(rng, [120_000, 120_000])
    _plant_family(G, rng, cons, 6, 0.0)
    worn = list(cons)
    for i in range(3, 400, step):
        worn[i] = casegen.BASES[(casegen.BASES.index(worn[i]) + 1 + int(rng.integers(0, 3))) % 4]
    worn = "".join(worn)
    return {"contigs": G.contigs(), "cands": [worn, casegen.revcomp(worn), cons]}


def low_complexity_control():
    """synth_small seed 11 with low-complexity candidates beside its own"""
    import synth_small

    g = synth_small.make(11, n_fam=8)
    extra = ["A" * 40, "AT" * 40, "ACGT" * 3, "AAC" * 30, "G" * 15 + "C" * 15, g["contigs"][0][5000:5400]]
    return {"contigs": g["contigs"], "cands": list(g["cands"]) + extra}


def all_cases():
    """[(label, case)] in a fixed order: the child process of the test runs the same list"""
    return [("classes", sort_classes()), ("edges", cluster_edges()), ("one-and-singletons", one_cluster_and_singletons()),
            ("long-end", long_end()), ("low-complexity", low_complexity_control())]
