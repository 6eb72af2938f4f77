"""CPU-only: the cell update and the compares of the banded HSP aligner (hite_amd/csrc/hite_hsp.h, the block between `// >>> hsp_cell`
and `// <<< hsp_cell`) compiled for the HOST as tests/test_host_compiled_framecluster.py does for the clustering of frames, inside the
host copy of the strip loop of hsp_align (tests/hsp_host.py), and compared with the twin at the strip-edge lengths the GPU tests run.
What only the device has -- the word table, the votes, the windows, the data-parallel moves, the batches -- is left to
tests/test_gpu_pairhsp.py."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import hsp_host as H  # noqa: E402
import pairhsp_cases as PC  # noqa: E402
import pairhsp_twin as T  # noqa: E402

WRAPPER = r"""
extern "C" int host_hsp(const uint8_t *q, int m, const uint8_t *s, int dlo, int dhi, int r0, int r1, int c0, int c1, int32_t *out) {
    const HspBest best = host_align(q, m, s, dlo, dhi, r0, r1, c0, c1);
    if (best.a == 0) return 0;
    out[0] = hsp_q_start(best.b); out[1] = hsp_q_end(best.e); out[2] = hsp_s_start(best.b); out[3] = hsp_s_end(best.e);
    out[4] = hsp_score(best.a); out[5] = hsp_matches(best.a); out[6] = hsp_columns(best.a);
    return 1;
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return H.compile_host(tmp_path_factory.mktemp("hsp_cell"), "ph", H.blocks("hite_hsp.h", "hsp_cell") + H.HOST_ALIGN + WRAPPER)


def test_the_aligner_is_defined_once():
    """the pair search, the LTR scan and the annotation include hite_hsp.h, and the cell and the strip routine stand nowhere else"""
    csrc = os.path.join(ROOT, "hite_amd", "csrc")
    text = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h", ".inc"))}
    for f in ("hite_pairhsp.hip", "hite_ltrscan.hip", "hite_annotate.hip"):
        assert '#include "hite_hsp.h"' in text[f], f
    for name in ("hsp_cell", "hsp_align"):
        defs = [f for f, t in text.items() for _ in re.finditer(r"^[^\n/]*\b\w+ %s\(" % name, t, re.M)]
        assert defs == ["hite_hsp.h"], (name, defs)
    assert sum(len(re.findall(r"_align\(const uint8_t \*q", t)) for t in text.values()) == 1


def _align(lib):
    def align(q, s, dlo, dhi, r0, r1, c0, c1):
        q, s = T.as_bytes(q), T.as_bytes(s)
        out = np.zeros(7, dtype=np.int32)
        ok = lib.host_hsp(q, len(q), s, dlo, dhi, r0, r1, c0, c1, out.ctypes.data_as(C.c_void_p))
        return tuple(int(x) for x in out) if ok else None
    return align


def _bands(q, s, dm):
    """the bands the definition gives the pair, and one at each end of the diagonals"""
    qc, sc = T.codes(q), T.codes(s)
    lo = T.NO_DIAG_MIN if dm is None else dm
    bands = [T.band_of(b, len(qc), lo) for b in T.windows(T.votes(qc, sc, lo))]
    return bands + [(-(len(qc) - 1) - 5, -(len(qc) - 1) + 186), (len(sc) - 1 - 186, len(sc) + 5), (-3, 0)]


def test_strip_loop_vs_twin_at_the_strip_edges(lib):
    """random and related pairs at lengths around the 64 columns of a strip, in their own bands and in bands at the corners"""
    align = _align(lib)
    grid = [c for c in PC.length_grid() if "unrelated" not in c[0]]
    n = 0
    for label, q, s, dm in grid:
        for dlo, dhi in _bands(q, s, dm):
            assert align(q, s, dlo, dhi, 1, len(q), 1, len(s)) == T.align_c(q, s, dlo, dhi, 1, len(q), 1, len(s)), (label, dlo, dhi)
            n += 1
    assert n >= 3 * len(grid)


def test_rectangles_and_band_edges(lib):
    """sub-rectangles, alignments that run along and across the band's edges, diag_min through a band"""
    align = _align(lib)
    rng = np.random.default_rng(4)
    n_hsp = 0
    for label, q, s, dm in PC.rectangles() + PC.band_edges()[::3] + PC.diag_min_cases()[:6] + PC.ties() + PC.bytes_cases():
        m, n = len(q), len(s)
        for dlo, dhi in _bands(q, s, dm)[:-2]:
            rects = [(1, m, 1, n)]
            for _ in range(3):
                r0, c0 = int(rng.integers(1, m + 1)), int(rng.integers(1, n + 1))
                rects.append((r0, int(rng.integers(r0, m + 1)), c0, int(rng.integers(c0, n + 1))))
            for r in rects:
                got = align(q, s, dlo, dhi, *r)
                assert got == T.align_c(q, s, dlo, dhi, *r), (label, dlo, dhi, r)
                n_hsp += got is not None
    assert n_hsp > 100
