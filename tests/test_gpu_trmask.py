"""The tandem-repeat masker on the device (hite_trmask.hip) at the edges of its periods, tiles and contigs, and as a stage: HIP == the twin
(oracle/hite_oracle_trf.c, through test_trmask.twin_mask) bit for bit, everywhere.  The inputs are those of tests/trmask_cases.py, which
the `tr_seed` block built for the host passes as well (test_host_compiled.py): a disagreement here alone lies in what only the device
has -- the LDS tile and its barriers, the seed list and tr_extend_kernel, atomicOr, tr_apply_kernel, the launch geometry."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import casegen  # noqa: E402
import trmask_cases as TC  # noqa: E402
from test_trmask import twin_mask  # noqa: E402

pytestmark = pytest.mark.gpu

_TWIN = {}


def twin(contigs, P):
    """the twin's mask, computed once per (genome, max_period) and left unchanged"""
    key = (tuple(contigs), P)
    if key not in _TWIN:
        _TWIN[key] = twin_mask(contigs, P)
        _TWIN[key].setflags(write=False)
    return _TWIN[key]


@pytest.fixture(scope="module")
def ctx():
    import hite_amd

    c = hite_amd.Context(0)
    yield c
    c.close()


def gpu_mask(ctx, contigs, P):
    ctx.genome_pack(contigs)            # (the masker works in place: every case packs afresh)
    return ctx.tr_mask(P)


def check(got, exp):
    assert got.shape == exp.shape
    assert np.array_equal(got, exp), (int(got.sum()), int(exp.sum()), np.flatnonzero(got != exp)[:10].tolist())


def with_n(contigs, mask):
    """the contigs with the masked bases (bool array over their concatenation) written as N"""
    out, at = [], 0
    for c in contigs:
        b = np.frombuffer(c.encode(), dtype=np.uint8).copy()
        b[mask[at:at + len(c)]] = ord("N")
        out.append(b.tobytes().decode())
        at += len(c)
    return out


# ---- a. max_period on both sides of every border of the scan's groups and strides -------------------------------------------------------
@pytest.mark.parametrize("P", TC.PERIODS)
def test_period_sweep(ctx, P):
    contigs = TC.period_genome()
    exp = twin(contigs, P)
    assert int(exp.sum()) == TC.TWIN_MASKED[P]
    check(gpu_mask(ctx, contigs, P), exp)


# ---- b. arrays across tile borders and reseed points, contig ends beside them --------------------------------------------------------
@pytest.mark.parametrize("label,contigs,P,count", TC.border_cases(), ids=[c[0] for c in TC.border_cases()])
def test_tile_and_contig_borders(ctx, label, contigs, P, count):
    exp = twin(contigs, P)
    assert int(exp.sum()) == count
    check(gpu_mask(ctx, contigs, P), exp)


@pytest.mark.parametrize("P", TC.BLOCK1_PERIODS)
def test_leftmost_seed_in_second_block(ctx, P):
    """periods 16 .. 31 of arrays whose leftmost seed is the second 8-block of its word (trmask_cases.block1_genome)"""
    contigs = [TC.block1_genome()]
    exp = twin(contigs, P)
    assert int(exp.sum()) == TC.BLOCK1_TWIN_MASKED[P]
    for a, p in TC.BLOCK1_ARRAYS:
        assert exp[a:a + 3 * p + 8].all()
    check(gpu_mask(ctx, contigs, P), exp)


# ---- c. genomes shorter than a block, a word, a tile; uniform arrays longer than one extension -----------------------------------------
@pytest.mark.parametrize("seq", TC.TINY, ids=[TC.tiny_label(s) for s in TC.TINY])
def test_degenerate_genomes(ctx, seq):
    for P in TC.TINY_PERIODS:
        exp = twin([seq], P)
        if P == 500 and TC.tiny_expect_500(seq) is not None:
            assert int(exp.sum()) == TC.tiny_expect_500(seq)
        check(gpu_mask(ctx, [seq], P), exp)


def test_equal_units_do_not_join_across_contig_borders(ctx):
    """five of the degenerate genomes as contigs of one: poly-A ends where poly-A begins, twice"""
    contigs = ["ACG" * 11, "A" * 33, "A" * 16, "A" * 17, "AC" * 20]
    assert all(c in TC.TINY for c in contigs)
    off = np.concatenate([[0], np.cumsum([len(c) for c in contigs])])
    exp = twin(contigs, 500)
    assert exp[off[0]:off[1]].all() and exp[off[1]:off[2]].all()          # the ACG array; 33 A are an array on their own
    assert exp[off[2]:off[4]].sum() == 0                                  # 16 A and 17 A are too short each: they join neither the 33 A
    assert exp[off[4]:off[5]].all()                                       # before them nor each other (33 A together would be masked)
    for P in TC.TINY_PERIODS:
        check(gpu_mask(ctx, contigs, P), twin(contigs, P))


# ---- d. a genome that already carries a mask -----------------------------------------------------------------------------------------------
def premask_intervals():
    """-> [(contig, start1, end1)], 1-based inclusive as hite_genome_mask takes them, chosen from the planted arrays"""
    _contigs, planted = TC.period_case()
    out = []

    def array(k, p):                 # the k-th planted array, which has period p
        assert planted[k][2] == p
        return planted[k][0], planted[k][1]

    def add(a, b):                   # positions [a, b) of the planted sequence, inside one contig
        (c, x), (c2, y) = TC.period_locate(a), TC.period_locate(b - 1)
        assert c == c2
        out.append((c, x + 1, y + 1))

    a, b = array(0, 33)
    add((a + b) // 2 - 10, (a + b) // 2 + 10)                   # cuts an array in half
    a, b = array(1, 48)
    add(a + 466, a + 467)                                       # one base inside an array
    a, b = array(18, 77)
    assert planted[18][4] == 0 and planted[18][5] == 0
    add(a + 3 * 77, a + 4 * 77)                                 # exactly one whole copy (the array has neither substitutions nor indels)
    add(2000, 2100)                                             # background
    add(8950, 9000)                                             # up to the end of the first contig
    a, b = array(19, 500)
    add(a + 500, b)                                             # the second of two copies: no array is left
    a, b = array(7, 1)
    add(a + 24, a + 25)                                         # one base of a homopolymer run
    add(9770, 9777)                                             # up to the N run
    a, b = array(9, 120)
    add(a + 517, a + 577)
    a, b = array(14, 21)
    add(a, b)                                                   # a whole array
    add(35000, 35010)                                           # background of the third contig
    out.append((1, 1, 10))                                      # from the start of the second contig
    out.append((3, 5, 8))                                       # inside a short contig that is an array itself
    out.append((4, 30, 100))                                    # runs past the end of its contig: clamped like a python slice
    return out


def test_genome_that_already_carries_a_mask(ctx):
    contigs = TC.period_genome()
    masked = [bytearray(c.encode()) for c in contigs]
    iv = premask_intervals()
    for c, s1, e1 in iv:
        masked[c][s1 - 1:e1] = b"N" * len(masked[c][s1 - 1:e1])
    masked = [bytes(m).decode() for m in masked]
    assert [len(m) for m in masked] == [len(c) for c in contigs]
    exp = twin(masked, 500)
    plain = twin(contigs, 500)
    assert (exp != plain).sum() > 500 and exp.sum() > 3000          # the intervals hit the arrays, and most arrays are still there
    ctx.genome_pack(contigs)
    ctx.genome_mask([i[0] for i in iv], [i[1] for i in iv], [i[2] for i in iv])
    check(ctx.tr_mask(500), exp)


# ---- e. a second call; the count without the bit map -----------------------------------------------------------------------------------------
def test_second_call_and_count_without_bit_map(ctx):
    contigs = TC.period_genome()
    ctx.genome_pack(contigs)
    first = ctx.tr_mask(500)
    check(first, twin(contigs, 500))
    second = ctx.tr_mask(500)
    check(second, twin(with_n(contigs, first), 500))
    ctx.genome_pack(contigs)
    assert ctx.tr_mask_dev(500) == int(first.sum()) == TC.TWIN_MASKED[500]      # mask_bits_host == NULL, as the benchmark calls it


# ---- f. later stages read N where the masker masked -------------------------------------------------------------------------------------------
def test_later_stages_see_n(ctx):
    contigs = TC.period_genome()
    exp = with_n(contigs, twin(contigs, 500))
    ctx.genome_pack(contigs)
    assert ctx.tr_mask_dev(500) == TC.TWIN_MASKED[500]
    flank = 50
    rows = []                                       # (contig, window [lo, hi) inside it): windows of 200 .. 400 bases tile the contig
    lens = [200, 257, 301, 333, 399, 400, 216, 384]
    for c in range(3):
        L, lo, covered = len(contigs[c]), 0, np.zeros(len(contigs[c]), dtype=bool)
        while lo < L:
            hi = min(L, lo + lens[len(rows) % len(lens)])
            lo = min(lo, hi - 200)                  # (the last one reaches back)
            rows.append((c, lo, hi))
            covered[lo:hi] = True
            lo = hi
        assert covered.all()
    n = len(rows)
    cid = [r[0] for r in rows] * 2
    s1 = [r[1] + flank + 1 for r in rows] * 2
    e1 = [r[2] - flank for r in rows] * 2
    minus = [0] * n + [1] * n
    wins, _trunc = ctx.flank_gather(cid, s1, e1, minus, flank=flank)
    n_seen = 0
    for k, w in enumerate(wins):
        c, lo, hi = rows[k % n]
        want = exp[c][lo:hi]
        assert w is not None and w.decode() == (casegen.revcomp(want) if minus[k] else want), (k, c, lo, hi)
        if not minus[k]:
            n_seen += w.count(b"N")
    n_twin = int(twin(contigs, 500)[:sum(len(c) for c in contigs[:3])].sum())
    assert n_twin > 6000 and n_seen >= n_twin


# ---- g. seeds extended on the spot (no seed list) ---------------------------------------------------------------------------------------------
def test_on_the_spot_extension_path(ctx, tmp_path):
    """HITE_TR_DEFER=0 in one fresh child process (tests/_trmask_child.py): its masks == the twin == the default path's"""
    import _trmask_child

    out = tmp_path / "masks.json"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_trmask_child.py"), str(out)], env={**os.environ, "HITE_TR_DEFER": "0"},
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    got = json.loads(out.read_text())
    cases = _trmask_child.cases()
    assert sorted(got) == sorted(c[0] for c in cases) and len(cases) == 7
    for label, contigs, P in cases:
        G, hexed = got[label]
        m = np.unpackbits(np.frombuffer(bytes.fromhex(hexed), dtype=np.uint8))[:G].astype(bool)
        check(m, twin(contigs, P))
        check(m, gpu_mask(ctx, contigs, P))
