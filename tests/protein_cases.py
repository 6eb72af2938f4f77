"""Case builders shared by the tests of the translated protein search (tests/test_protein_host.py, tests/test_gpu_protein.py) and
by tools/protein_bench.py: random proteins, back-translation with random codons, residue divergence, reverse complement."""
import protein_twin as T

STD = T.LETTERS[:20]
CODONS_OF = {}
for _cod, _aa in T.CODON.items():
    CODONS_OF.setdefault(_aa, []).append(_cod)
for _v in CODONS_OF.values():
    _v.sort()


def rand_protein(rng, n):
    return "".join(STD[k] for k in rng.integers(0, 20, n))


def rand_dna(rng, n):
    return "".join("ACGT"[k] for k in rng.integers(0, 4, n))


def back_translate(rng, prot):
    """random codon per residue (X -> NNN)"""
    return "".join(CODONS_OF[a][int(rng.integers(0, len(CODONS_OF[a])))] if a in CODONS_OF else "NNN" for a in prot)


def diverge(rng, prot, frac):
    """every residue replaced with probability frac by another standard residue"""
    out = []
    for a in prot:
        if rng.random() < frac:
            b = a
            while b == a:
                b = STD[int(rng.integers(0, 20))]
            a = b
        out.append(a)
    return "".join(out)


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGTacgt", "TGCAtgca"))
