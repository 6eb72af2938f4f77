"""hite_fill_tile.h compiled for the HOST: the phases of the tile form of the sparse fill (ops load, window range into the slot, cells
into the image, image to the output row), run lane by lane over every (row, tile) the way star_fill_tile_kernel runs them, must write
exactly the twin's sparse alignment -- and so must fill_sparse_row (hite_fill.h) on the same ops and layout words.  Inputs: the groups
of star_layout_cases.py and the cases of fill_tile_cases.py at the tile form's own limits, ops and layout words derived from the
twin's alignment.  Windows and output rows sit at every offset within 16 bytes; slot and image are poisoned before every (row, tile);
the bytes around an output row must stay untouched.  No GPU needed."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fill_tile_cases as FC  # noqa: E402
import star_layout_cases as SC  # noqa: E402
from test_host_compiled import _block, _build  # noqa: E402

WRAPPER = r"""
#include <string.h>
alignas(16) static uint8_t g_slot[FT_LDS], g_img[FT_LDS];
extern "C" void host_ft_limits(int *o) { o[0] = FT_T; o[1] = FT_SLOT; o[2] = FT_ROWS; }
// one row, tile by tile; how[t] = 0 the tile form, 1 the row's range did not fit, 2 the tile's columns did not fit
extern "C" int host_fill_tile_row(uint8_t *row, int Cn, const uint8_t *b, int nrow, const uint16_t *rop, const uint32_t *lay, int m, int le,
                                  int centre, int *how) {
    static FtOps L[64];
    static FtV16 v[64][FT_CH];
    for (int P0 = 0, t = 0; P0 <= m; P0 += FT_T, t++) {
        const int pl = min(P0 + FT_T - 1, m);
        int c0, W, qa, len;
        const bool tile_ok = ft_tile_plan(lay[P0], lay[pl < m ? pl + 1 : m], pl == m, Cn, &c0, &W);
        for (int lane = 0; lane < 64; lane++) L[lane] = ft_ops_load(rop, P0 + lane * FT_NP, m, centre != 0, centre != 0);
        const bool ok = ft_row_plan(L[0].oprev, ft_lane_op(L[(pl - P0) / FT_NP], (pl - P0) % FT_NP), P0, pl, m, nrow, centre != 0, &qa, &len);
        if (!ok || !tile_ok) {
            for (int lane = 0; lane < 64; lane++) ft_cells_direct(row, b, nrow, rop, lay, m, le, centre != 0, P0, pl + 1, lane);
            how[t] = tile_ok ? 1 : 2;
            continue;
        }
        how[t] = 0;
        memset(g_slot, 0xee, sizeof g_slot);
        memset(g_img, 0xee, sizeof g_img);
        const int sh = ft_win_shift(b, qa);
        for (int lane = 0; lane < 64; lane++) ft_win_load(v[lane], b, qa, len, lane);
        for (int lane = 0; lane < 64; lane++) ft_win_put(g_slot, v[lane], ft_win_chunks(sh, len), lane);
        for (int lane = 0; lane < 64; lane++) {
            uint32_t w[FT_NP];
            for (int u = 0; u < FT_NP; u++) { const int p = P0 + lane * FT_NP + u; w[u] = p <= m ? lay[p] : 0u; }
            ft_cells(g_img, g_slot, L[lane], w, P0 + lane * FT_NP, m, nrow, le, centre != 0, sh - qa, ft_img_shift(row + c0) - c0);
        }
        for (int lane = 0; lane < 64; lane++) ft_store(row + c0, g_img, W, lane);
    }
    return 0;
}
extern "C" void host_fill_row(uint8_t *row, const uint8_t *b, int nrow, const uint16_t *rop, const uint32_t *lay, int m, int le, int centre) {
    for (int t = 0; t < 64; t++) fill_sparse_row<uint8_t *, 64>(row, b, nrow, rop, lay, m, le, centre != 0, t);
}
"""

u8p = C.POINTER(C.c_uint8)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    csrc = os.path.join(ROOT, "hite_amd", "csrc")
    body = _block(os.path.join(csrc, "hite_fill.h"), "fill_sparse_row") + _block(os.path.join(csrc, "hite_fill_tile.h"), "fill_tile_row")
    return _build(tmp_path_factory.mktemp("fill_tiles"), "fill_tiles", body, WRAPPER)


@pytest.fixture(scope="module")
def limits(lib):
    o = (C.c_int * 3)()
    lib.host_ft_limits(o)
    return (o[0], o[1], o[2], 2)


def _aligned(n, off, fill):
    """n bytes that begin `off` bytes behind a 16-byte boundary, 32 guard bytes on either side: (whole buffer, start index)"""
    buf = np.full(n + 96, fill, np.uint8)
    start = (-buf.ctypes.data) % 16 + 32 + off
    return buf, start


def run_group(lib, d, T, what):
    """every row of a derived alignment through both forms; -> how[r][t] of the tile form"""
    m, Cn, R = d["m"], d["C"], d["R"]
    ntile = m // T + 1
    hows = []
    lay = np.concatenate([d["lay"], np.zeros(16, np.uint32)])
    for r in range(R):
        seq = np.frombuffer(d["rows"][r], np.uint8)
        wbuf, ws = _aligned(len(seq), (5 * r + 3) % 16, 0x23)
        wbuf[ws:ws + len(seq)] = seq
        rbuf = np.concatenate([[0x8000], d["ops"][r], np.zeros(32, np.uint16)]).astype(np.uint16)
        rop = C.cast(rbuf.ctypes.data + 2, C.POINTER(C.c_uint16))
        how = (C.c_int * ntile)()
        for form in ("tile", "row"):
            obuf, os_ = _aligned(Cn, (r * Cn) % 16, 0x2a)
            dst = C.cast(obuf.ctypes.data + os_, u8p)
            b = C.cast(wbuf.ctypes.data + ws, u8p)
            if form == "tile":
                rc = lib.host_fill_tile_row(dst, Cn, b, len(seq), rop, lay.ctypes.data_as(C.POINTER(C.c_uint32)), m, d["le"], int(r == 0), how)
                assert rc == 0, (what, r)
            else:
                lib.host_fill_row(dst, b, len(seq), rop, lay.ctypes.data_as(C.POINTER(C.c_uint32)), m, d["le"], int(r == 0))
            got = obuf[os_:os_ + Cn]
            assert np.array_equal(got, d["exp"][r]), (what, form, r, np.flatnonzero(got != d["exp"][r])[:8].tolist())
            assert (obuf[:os_] == 0x2a).all() and (obuf[os_ + Cn:] == 0x2a).all(), (what, form, r, "wrote outside the row")
        hows.append(list(how))
    return hows


@pytest.mark.parametrize("label", SC.LABELS + ["long"])
def test_layout_cases(lib, limits, label):
    if label == "long":
        fulls = [SC.twin_full(SC.long_group())]
    else:
        SC.check_precondition(label)
        fulls = [f for f, _ in SC.twin(label)]
    for i, full in enumerate(fulls):
        if label == "pads":
            assert not (full & 0x20)[full != SC.GAP].any()
        run_group(lib, FC.derive(full), limits[0], "%s[%d]" % (label, i))


def test_tile_limit_cases(lib, limits):
    T = limits[0]
    seen = {}
    for label in FC.labels(limits):
        gs, ds = FC.case(limits, label)
        seen[label] = [run_group(lib, d, T, "%s[%d]" % (label, i)) for i, d in enumerate(ds)]
    # the far side of the slot is the per-cell path, and only there
    for dd, direct in ((-1, 0), (0, 0), (1, 1)):
        how = seen["slot_%+d" % dd][0]
        assert [h[0] for h in how] == [0, 0, direct, 0, 0, 0] and all(h[1] == 0 for h in how), (dd, how)
    assert all(h == 0 for label, hs in seen.items() if not label.startswith("slot") for g in hs for row in g for h in row)
