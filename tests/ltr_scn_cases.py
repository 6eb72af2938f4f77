"""TEST INFRASTRUCTURE: what the tests of FiLTR's steps 1 and 2 share (tests/test_ltr_scn_rules.py on the CPU,
tests/test_gpu_ltr_scn_filter.py on the device): the plan and seed of the planted genome -- chosen so that every planted element gets
its planted decision through the twin, which tests/test_ltr_scn_rules.py checks on the CPU -- the golden fixture and its tables."""
import gzip
import hashlib
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PLAN = [("clean", 8), ("recomb", 4), ("nested", 4), ("overhang", 4), ("shifted", 4), ("dirty", 3), ("dup", 2)]
SEED = 2


def load_fixture():
    with gzip.open(os.path.join(ROOT, "tests", "golden", "ltr_scn_filter.json.gz")) as f:
        return json.loads(f.read().decode())


def pair_key(seqs, pair, diag_min):
    """the key of a search in the fixture's tables: the SHA-1 of the two intervals and diag_min"""
    a, a0, a1, b, b0, b1 = pair
    return (hashlib.sha1(seqs[a][a0:a1].encode()).hexdigest(), hashlib.sha1(seqs[b][b0:b1].encode()).hexdigest(), diag_min)


def table_of(entries):
    return {(e["q"], e["s"], e["diag_min"]): [tuple(h) for h in e["hsps"]] for e in entries}


def table_hsps(entries, used=None):
    """a stand-in for Context.pair_hsps that answers from a table of the fixture"""
    by_key = table_of(entries)

    def hsps(seqs, pairs, diag_min=None):
        keys = [pair_key(seqs, p, diag_min) for p in pairs]
        if used is not None:
            used.update(keys)
        return [by_key[k] for k in keys]
    return hsps


def write_inputs(d, contigs, scn):
    scn_path, ref_path = os.path.join(str(d), "in.scn"), os.path.join(str(d), "ref.fa")
    with open(scn_path, "w") as f:
        f.write(scn)
    with open(ref_path, "w") as f:
        for name, seq in contigs.items():
            f.write(">%s\n%s\n" % (name, seq))
    return scn_path, ref_path
