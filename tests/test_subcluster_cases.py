"""CPU-only: the sub-clustering of an alignment (include/hite_gpu.h, hite_msa_subcluster) away from the device --
  - the twin (tests/subcluster_twin.py, written from the definition) against util.ninja_stand_in, the statement the product ran so far,
    and against literal expectations;
  - the chunked form the kernels run (phase A against the old leaders, match bits inside the chunk, one ordered pass), written out in
    Python in the twin's file, against the twin at chunk sizes 1, 3 and 8;
  - the per-pair count of hite_amd/csrc/hite_subcluster.hip (the block between `// >>> subcluster_pair` and `// <<< subcluster_pair`)
    compiled for the HOST as tests/test_host_compiled_identity.py does for ident_cell, inside a host copy of the wavefront's loop
    (head bytes, whole 16-byte words dealt to the lanes, tail bytes), against the twin's (diff, n) on every pair of the small cases;
  - the switch of the host layer (util._generate_cons_batch) with every device stage answered by its twin.
What only the device has -- the launches, LDS, the shuffles, the batches -- is left to tests/test_gpu_subcluster.py."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import subcluster_cases as SC  # noqa: E402
import subcluster_twin as T  # noqa: E402


def _all_cases():
    return SC.small_cases() + [("families", SC.family_batch(), 0.2)]


def test_twin_is_the_stand_in():
    from hite_amd import util

    assert util.NINJA_CUTOFF == 0.2
    n = 0
    for label, als, cutoff in _all_cases() + SC.size_batch():
        assert cutoff == 0.2
        for k, al in enumerate(als):
            assert T.subcluster(al, cutoff) == util.ninja_stand_in(T.as_matrix(al)), (label, k)
            n += 1
    assert n > 550


def test_literal_expectations():
    seen = 0
    for label, als, cutoff in SC.small_cases():
        for table in (SC.DEGENERATE_EXPECT, SC.ORDER_EXPECT, SC.BYTES_EXPECT):
            if label in table:
                assert [T.subcluster(al, cutoff) for al in als] == table[label], label
                seen += 1
    assert seen == len(SC.DEGENERATE_EXPECT) + len(SC.ORDER_EXPECT) + len(SC.BYTES_EXPECT)
    # the leader counts: unrelated rows are leaders, every copy joins the row it was copied from
    for label, als, cutoff in SC.leader_counts():
        R = int(label.split("-")[1])
        got = T.subcluster(als[0], cutoff)
        assert len(got) == R and sorted(len(g) for g in got)[-1] >= 3, label
        extra = [g for g in got if len(g) > 1]
        assert [g[0] for g in extra] == sorted({0, min(63, R - 1), min(64, R - 1), R - 1}), label
    # the threshold: diff = n // 5 joins, n // 5 + 1 does not, whatever the columns of gaps
    for al, n in zip(SC.threshold()[0][1], SC.THRESHOLD_N):
        assert T.pair_counts(al[0], al[1]) == (n // 5, n) and T.pair_counts(al[0], al[2]) == (n // 5 + 1, n)
        assert al.shape[1] > n or n == 65535
        assert T.subcluster(al, 0.2) == [[0, 1], [2]]
    # the tails: n = 5k against row 0, diff = k or k + 1
    for al in SC.tails()[0][1]:
        k = al.shape[1] // 5
        for r in range(1, 9):
            d, n = T.pair_counts(al[0], al[r])
            assert n == (5 * k if k else al.shape[1]) and d <= k + 1, (al.shape, r, d, n)
        if k >= 1:
            assert {T.pair_counts(al[0], al[r])[0] for r in range(1, 9)} == {k, k + 1}


def test_chunk_boundary_cases_hold_what_they_claim():
    B = SC.CHUNK
    als = SC.chunk_boundary()[0][1]
    assert [a.shape[0] for a in als] == [B - 1, B, B + 1, 2 * B + 1]
    for al in als:
        R = al.shape[0]
        sub, n_sub = T.sub_of_row(al, 0.2)
        lead = {}
        for r, k in enumerate(sub):
            lead.setdefault(k, r)
        is_leader = [lead[sub[r]] == r for r in range(R)]
        m = lambda a, b: T.matches(*T.pair_counts(al[a], al[b]), 0.2)  # noqa: E731
        assert is_leader[0] and sub[1] == sub[0]                               # a later row of the chunk joins a leader born in it
        assert sub[3] == sub[2] and is_leader[4] and m(4, 3) and not m(4, 2)     # matches a non-leader only: founds
        if R > B:
            assert sub[B - 1] == sub[B - 2] and is_leader[B] and m(B, B - 1)     # ... across the chunk border
        if R > B + 5:
            assert is_leader[5] and is_leader[B + 2] and m(B + 5, B + 2) and sub[B + 5] == sub[5]   # old leader before the new one
        assert sub[R - 1] == 0 or R - 1 in (B - 1, B)


@pytest.mark.parametrize("B", [1, 3, 8])
def test_chunked_form_is_the_twin(B):
    for label, als, cutoff in _all_cases():
        if label.startswith("leaders-") and int(label.split("-")[1]) > 257:
            continue            # (the Python pair loop of the chunked form is slow: the device runs this one)
        for k, al in enumerate(als):
            if T.as_matrix(al).shape[1] > 2000:
                continue
            assert T.chunked(al, cutoff, B) == T.subcluster(al, cutoff), (label, k, B)
    for cutoff in (0.0, 0.5, 1.0):
        for k, al in enumerate(SC.family_batch(60, seed=77)):
            assert T.chunked(al, cutoff, B) == T.subcluster(al, cutoff), (cutoff, k, B)


# ---- the per-pair count of the kernel, compiled for the host --------------------------------------------------------------------
PRELUDE = r"""
#include <stdint.h>
#include <stddef.h>
#define __device__
#define __forceinline__ inline
"""

WRAPPER = r"""
// the wavefront's loop of sub_pair_match with `lanes` workers run one after the other (no early exit: the counts are compared)
static void host_pair(const uint8_t *x, const uint8_t *y, int C, int lanes, int32_t *out) {
    int head, nw, diff = 0, n = 0;
    sub_split(x, C, head, nw);
    for (int lane = 0; lane < lanes; lane++) {
        sub_count_ends(x, y, C, head, nw, lane, lanes, diff, n);
        for (int w = lane; w < nw; w += lanes) sub_count16(x + head + (size_t)w * 16, y + head + (size_t)w * 16, diff, n);
    }
    out[0] = diff; out[1] = n;
}
// every pair (i, j < i) of an alignment at `mat`: out[(i * R + j) * 2 ..] = diff, n
extern "C" void host_all_pairs(const uint8_t *mat, int R, int C, int lanes, int32_t *out) {
    for (int i = 0; i < R; i++)
        for (int j = 0; j < i; j++) host_pair(mat + (size_t)i * C, mat + (size_t)j * C, C, lanes, out + ((size_t)i * R + j) * 2);
}
extern "C" int host_match(int diff, int n, double cutoff) { return sub_match(diff, n, cutoff) ? 1 : 0; }
"""


@pytest.fixture(scope="module")
def pair_lib(tmp_path_factory):
    src = open(os.path.join(ROOT, "hite_amd", "csrc", "hite_subcluster.hip")).read()
    m = re.search(r"// >>> subcluster_pair.*?\n(.*?)// <<< subcluster_pair", src, re.S)
    assert m
    d = tmp_path_factory.mktemp("subcluster_pair")
    cpp, so = d / "pair.cpp", d / "pair.so"
    cpp.write_text(PRELUDE + m.group(1) + WRAPPER)
    extra = os.environ.get("HITE_HOST_CXXFLAGS", "").split()
    subprocess.run(["g++", "-O2", "-shared", "-fPIC"] + extra + ["-o", str(so), str(cpp)], check=True)
    lib = C.CDLL(str(so))
    lib.host_match.argtypes = [C.c_int, C.c_int, C.c_double]
    return lib


def _twin_counts(m):
    R = m.shape[0]
    out = np.zeros((R, R, 2), dtype=np.int32)
    for i in range(1, R):
        out[i, :i, 0] = (m[:i] != m[i]).sum(axis=1)
        out[i, :i, 1] = ((m[:i] != 45) | (m[i] != 45)).sum(axis=1)
    return out


def test_pair_count_compiled_for_the_host(pair_lib):
    """the alignments of a case are packed back to back behind `shift` bytes, as the device holds a batch: rows start at every
    offset modulo 16"""
    pairs = 0
    for label, als, _cutoff in SC.small_cases():
        mats = [T.as_matrix(al) for al in als]
        mats = [m for m in mats if m.size]
        for shift, lanes in ((0, 64), (5, 1), (11, 7)):
            if lanes != 64 and sum(m.size for m in mats) > 200000:
                continue
            buf = np.concatenate([np.full(shift, 45, np.uint8)] + [m.reshape(-1) for m in mats] + [np.full(16, 45, np.uint8)]) if mats else None
            at = shift
            for k, m in enumerate(mats):
                R, Cc = m.shape
                got = np.zeros((R, R, 2), dtype=np.int32)
                pair_lib.host_all_pairs(C.c_void_p(buf.ctypes.data + at), R, Cc, lanes, got.ctypes.data_as(C.c_void_p))
                exp = _twin_counts(m)
                bad = np.argwhere((got != exp).any(axis=2))
                assert len(bad) == 0, (label, k, shift, lanes, bad[:5].tolist())
                at += m.size
                pairs += R * (R - 1) // 2
    assert pairs > 500000


def test_match_compiled_for_the_host(pair_lib):
    """the one binary64 compare: for cutoff 0.2 it is 5 diff <= n"""
    for n in list(range(0, 300)) + [4095, 4096, 20000, 65535]:
        for d in {0, n // 5 - 1, n // 5, n // 5 + 1, n} - {-1}:
            if d <= n:
                assert bool(pair_lib.host_match(d, n, 0.2)) == (n > 0 and 5 * d <= n) == T.matches(d, n, 0.2), (d, n)
    for cutoff in (0.0, 0.5, 1.0):
        for d, n in ((0, 0), (0, 7), (1, 7), (3, 7), (4, 7), (7, 7), (3, 6)):
            assert bool(pair_lib.host_match(d, n, cutoff)) == T.matches(d, n, cutoff)


# ---- the host layer ------------------------------------------------------------------------------------------------------------
def _ctx_classes():
    from oracle_ctx import OracleCtx

    class Refuses(OracleCtx):
        def msa_subcluster(self, alignments, cutoff=0.2):
            raise AssertionError("the switch is off: nothing new may be called on the context")

    class FromTwin(OracleCtx):
        calls = 0

        def msa_subcluster(self, alignments, cutoff=0.2):
            self.calls += 1
            return [T.subcluster(al, cutoff) for al in alignments]

    return Refuses, FromTwin


def test_switch_of_the_host_layer(monkeypatch):
    from hite_amd import util

    monkeypatch.delenv("HITE_SUBCLUSTER", raising=False)
    Refuses, FromTwin = _ctx_classes()
    batch = SC.cons_clusters()
    off = util._generate_cons_batch(Refuses(), batch)
    assert util._generate_cons_batch(Refuses(), batch, subcluster="cpu") == off
    assert sum(len(d) for d in off[:3]) >= 6 and "c1_short" in off[1] and off[3] == dict(batch[3])   # two sub-families each; the dropped member passes
    ctx = FromTwin()
    secs = {}
    on = util._generate_cons_batch(ctx, batch, subcluster="gpu", seconds=secs)
    assert on == off and ctx.calls == 1                    # ONE call for all first alignments
    assert sorted(secs) == ["align_first", "align_second", "consensus", "subcluster"] and all(v >= 0 for v in secs.values())
    monkeypatch.setenv("HITE_SUBCLUSTER", "gpu")
    ctx = FromTwin()
    assert util._generate_cons_batch(ctx, batch) == off and ctx.calls == 1
    with pytest.raises(AssertionError):
        util._generate_cons_batch(Refuses(), batch)
    # a caller's Ninja clusters override the switch: nothing is asked of the context
    ninja = [{0: [n for n, _s in cl]} for cl in batch]
    assert util._generate_cons_batch(Refuses(), batch, ninja) == util._generate_cons_batch(Refuses(), batch, ninja, subcluster="off")


def test_stage_seconds_of_the_library_merge(tmp_path, monkeypatch):
    from hite_amd import util

    monkeypatch.delenv("HITE_SUBCLUSTER", raising=False)
    _Refuses, FromTwin = _ctx_classes()
    recs = [r for cl in SC.cons_clusters(seed=4111) for r in cl]
    outs = []
    for mode in (None, "gpu"):
        lib = str(tmp_path / ("lib_%s.fa" % mode))
        util.store_fasta(dict(recs), lib)
        st = {}
        ctx = FromTwin()
        util.deredundant_for_LTR_v5(lib, str(tmp_path), 1, "terminal", 0.95, 0, ctx=ctx, stages=st, subcluster=mode)
        assert list(st["seconds"]) == ["hits", "stretch", "chain", "cluster", "align_first", "subcluster", "align_second", "consensus",
                                       "redundancy"]
        assert all(isinstance(v, float) and v >= 0 for v in st["seconds"].values()) and st["seconds"]["align_first"] > 0
        assert ctx.calls == (1 if mode == "gpu" else 0)
        outs.append((st["clusters"], util.read_fasta(lib + ".tmp.cons"), util.read_fasta(lib + ".cons")))
    assert outs[0] == outs[1]
