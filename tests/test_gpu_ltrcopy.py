"""GPU: the full-length copy support (hite_amd/csrc/hite_ltrcopy.hip; Context.ltr_copy_support_records and Context.ltr_copy_support)
against tests/ltrcopy_twin.py for exact equality, copy for copy, with the statistics of every run: the crafted tables of
tests/ltrcopy_cases.py (elements of 0, 1, 63, 64, 65 and 300 records, the coverage bound, the buckets at a multiple of 100 000, the
order of equally long copies, nesting on one contig and on two), the capacity protocol, refused arguments, and the fused entry on a
genome with a family of 300 short copies and a family of long elements truncated below and above the bound, on both strands.
The records carry no strand (the rule reads none): the minus-strand copies are those of the fused test."""
import functools

import numpy as np
import pytest

import ltrcopy_cases as LC
import ltrcopy_twin as LT

pytestmark = pytest.mark.gpu
HITE_EINVAL, HITE_ECAP = -1, -4


@pytest.fixture(scope="module")
def ctx():
    import hite_amd

    c = hite_amd.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("case", LC.crafted(), ids=lambda c: c["label"])
def test_records_vs_twin(ctx, case):
    st, gst = {}, {}
    exp = LT.support_records(case["el_len"], case["records"], case["std"], case["contig_len"], stats=st, **case["kw"])
    got = ctx.ltr_copy_support_records(case["el_len"], case["records"], case["std"], case["contig_len"], stats=gst, **case["kw"])
    bad = [k for k in range(len(exp)) if got[k] != exp[k]]
    assert len(got) == len(exp) and not bad, (bad[:5], got[bad[0]], exp[bad[0]])
    assert gst == st and (case["stats"] is None or gst == case["stats"])


def test_other_thresholds_and_segments(ctx):
    """the same table under a looser coverage, a tighter overlap and segments of 10 000 bases: other records pass, other buckets"""
    c = LC.record_counts()
    seen = set()
    for kw in (dict(full_length_coverage=0.95), dict(overlap_threshold=0.99), dict(segment_len=10_000), dict(full_length_coverage=1.0, overlap_threshold=1.0)):
        st, gst = {}, {}
        exp = LT.support_records(c["el_len"], c["records"], c["std"], c["contig_len"], stats=st, **kw)
        assert ctx.ltr_copy_support_records(c["el_len"], c["records"], c["std"], c["contig_len"], stats=gst, **kw) == exp and gst == st
        seen.add((st["covered"], st["matched"], st["kept"]))
    assert len(seen) == 4


def test_capacity(ctx):
    """too little room: HITE_ECAP with the number of copies, then the same call with exactly that room"""
    import hite_amd

    c = LC.record_counts()
    st = {}
    exp = LT.support_records(c["el_len"], c["records"], c["std"], c["contig_len"], stats=st)
    for cap in (0, st["kept"] - 1):
        gst = {}
        with pytest.raises(hite_amd.HiteError) as err:
            ctx.ltr_copy_support_records(c["el_len"], c["records"], c["std"], c["contig_len"], cap=cap, stats=gst)
        assert err.value.code == HITE_ECAP and err.value.n_out == st["kept"] and gst == st
    gst = {}
    assert ctx.ltr_copy_support_records(c["el_len"], c["records"], c["std"], c["contig_len"], cap=st["kept"], stats=gst) == exp and gst == st


def test_empty_and_refused(ctx):
    import hite_amd

    assert ctx.ltr_copy_support_records([], [], [], [1000]) == []
    assert ctx.ltr_copy_support_records([500, 600], [[], []], [(0, 10, 510)], [1000]) == [[], []]
    st = {}
    assert ctx.ltr_copy_support_records([500], [[(0, 11, 510, 0)]], [], [1000], stats=st) == [[]] and st == dict(records=1, covered=1, matched=0, kept=0)
    c = LC.too_many()
    bad = [(c["el_len"], c["records"], c["std"], c["contig_len"], {}),                              # 301 records
           ([500], [[(1, 11, 510, 0)]], [(0, 10, 510)], [1000], {}),                                 # a contig the genome does not have
           ([500], [[(0, 11, 510, 0)]], [(3, 10, 510)], [1000], {}),
           ([500], [[(0, 11, 510, 0)]], [(0, -1, 510)], [1000], {}),
           ([500], [[(0, 11, 510, 0)]], [(0, 10, 510)], [1000], dict(segment_len=0)),
           ([500], [[(0, 11, 510, 0)]], [(0, 10, 510)], [1000], dict(overlap_threshold=1.5)),
           ([500], [[(0, 11, 510, 0)]], [(0, 10, 510)], [1000], dict(full_length_coverage=float("nan")))]
    for el_len, records, std, clen, kw in bad:
        with pytest.raises(hite_amd.HiteError) as err:
            ctx.ltr_copy_support_records(el_len, records, std, clen, **kw)
        assert err.value.code == HITE_EINVAL
    # the context is usable afterwards
    assert ctx.ltr_copy_support_records([500], [[(0, 11, 510, 0)]], [(0, 10, 510)], [1000]) == [[(0, 11, 510)]]


COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _mutate(rng, seq, div):
    s = bytearray(seq)
    for p in rng.choice(len(s), size=int(len(s) * div), replace=False):
        s[p] = ord("ACGT"[("ACGT".index(chr(s[p])) + 1 + int(rng.integers(0, 3))) % 4])
    return bytes(s)


@functools.lru_cache(maxsize=None)
def fused_genome():
    """two contigs of about 100 kb: 300 copies of a 400-base element (1 % apart, a third of them on the minus strand), and an 8 kb
    element whole, on the minus strand, and cut at its right end to 99, 98.5, 98 and 97 %; the candidate lines are the places of the
    copies, but for every seventh short copy; + the twin's result"""
    rng = np.random.default_rng(17)
    rand = lambda n: bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n))  # noqa: E731
    short, long_ = rand(400), rand(8000)
    contigs, std = [bytearray(), bytearray()], []
    pieces = [(short, k % 3 == 0, k % 7 != 0) for k in range(300)]
    cuts = [8000, 8000, 7920, 7880, 7840, 7760]
    for k, n in enumerate(cuts):
        pieces.insert(40 + 45 * k, (long_[:n], k == 1, True))
    for k, (seq, minus, line) in enumerate(pieces):
        g = contigs[k % 2]
        g += rand(int(rng.integers(150, 260)))
        body = _mutate(rng, seq, 0.01)
        if minus:
            body = body.translate(COMP)[::-1]
        if line:
            std.append((k % 2, len(g), len(g) + len(body)))
        g += body
    for g in contigs:
        g += rand(300)
    contigs = [bytes(g).decode() for g in contigs]
    elements = [short.decode(), long_.decode()]
    st = {}
    exp = LT.support(contigs, elements, std, stats=st)
    return contigs, elements, std, exp, st


def test_fused_vs_twin(ctx):
    contigs, elements, std, exp, st = fused_genome()
    assert 190_000 < sum(len(c) for c in contigs) < 260_000
    ctx.genome_pack(contigs)
    for mode in (False, None):          # whole-candidate intervals set on the context: the call runs on aligned ones and puts the setting back
        ctx.copy_config(mode)
        before = ctx.find_copies(elements[:1], clips=True)
        gst = {}
        got = ctx.ltr_copy_support(elements, std, stats=gst)
        assert got == exp and gst == st
        assert ctx.find_copies(elements[:1], clips=True) == before
        assert all(r[5] == 0 for r in before[0]) == (mode is False)
    # what the genome was built for: the short family fills the finder's cap, the lines left out take their copies with them, the
    # long element keeps the whole copies and the cuts at or above the bound
    assert st["records"] >= 300 and st["covered"] > st["matched"] >= 200
    assert 200 <= len(exp[0]) <= 258 and len({r[0] for r in exp[0]}) == 2
    lens = sorted(r[2] - r[1] + 1 for r in exp[1])
    assert len(lens) in (3, 4) and lens[0] >= 7870 and lens[-1] >= 7990
