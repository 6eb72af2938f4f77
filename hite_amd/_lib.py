"""ctypes binding of libhite_gpu.so (include/hite_gpu.h).  This is the stub a HiTE maintainer
would add next to module/Util.py.  There is NO CPU fallback: if the HIP
library is missing or no GPU is present every call raises."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_HERE, "libhite_gpu.so")

HITE_TE = {"tir": 0, "helitron": 1, "non_ltr": 2}
INFO = {0: "", 1: "nb", 2: "fl1", 3: "EXC"}
HITE_SUBCLUSTER_CHUNK = 64   # include/hite_gpu.h: rows per chunk of hite_msa_subcluster
LTRDEEP_PARAMS, LTRDEEP_ROWS, LTRDEEP_COLS, LTRDEEP_KMER = 40026, 100, 200, 3872   # include/hite_gpu.h: HITE_LTRDEEP_*


class HiteError(RuntimeError):
    pass


class HiteCall(C.Structure):
    _fields_ = [("is_te", C.c_int32), ("info", C.c_int32), ("row_num", C.c_int32), ("bstart", C.c_int32),
                ("bend", C.c_int32), ("cons_len", C.c_int32), ("cons_off", C.c_int64)]


CALL_DTYPE = np.dtype([("is_te", "<i4"), ("info", "<i4"), ("row_num", "<i4"), ("bstart", "<i4"), ("bend", "<i4"),
                       ("cons_len", "<i4"), ("cons_off", "<i8")])
assert CALL_DTYPE.itemsize == 32 and C.sizeof(HiteCall) == 32
# hite_lcv (include/hite_gpu.h): a compiled HelitronScanner pattern; two bits per body position in `body` (A 0 C 1 G 2 T 3) and `care` (3 / 0)
LCV_DTYPE = np.dtype([("body", "<u8"), ("care", "<u8"), ("gap_min", "u1"), ("gap_max", "u1"), ("body_len", "u1"), ("pad", "u1", (5,))])
assert LCV_DTYPE.itemsize == 24
HELITRON_MAX_BODY, HELITRON_MAX_GAP = 32, 63

_lib = None


def load():
    """Load libhite_gpu.so; raises HiteError (never falls back) when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise HiteError("libhite_gpu.so not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                            "(or make -C hite_amd/csrc); there is no CPU fallback")
        lib = C.CDLL(SO_PATH)
        lib.hite_last_error.restype = C.c_char_p
        lib.hite_genome_bases.restype = C.c_int64
        lib.hite_host_free.restype = None
        lib.hite_host_free.argtypes = [C.c_void_p]
        lib.hite_protein_lib_release.restype = None
        lib.hite_protein_lib_release.argtypes = [C.c_void_p]
        lib.hite_ltr_model_release.restype = None
        lib.hite_ltr_model_release.argtypes = [C.c_void_p]
        _lib = lib
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _arr(x, dtype):
    return np.ascontiguousarray(x, dtype=dtype)


def seed_sub_shard(rank, world, s, S):
    """sub-share s of S of the share (rank, world) of the all-vs-all stage (world <= 1: of the whole stage), as the (rank, world)
    pair hite_seed_shard takes.  hite_seed_shard puts the lower edge of rank k at mass 2.0 * k / world in binary64; k / world and
    k S / (world S) are the same rational, so their correctly rounded quotients are the same double and every edge of `world` is an
    edge of world S: the sub-shares rank S .. rank S + S - 1 tile the share exactly, on the device and in the twin."""
    if world <= 1:
        rank, world = 0, 1
    return rank * S + s, world * S


class Context:
    """One per process/GPU.  Owns the resident 2-bit genome and device scratch."""

    def __init__(self, device=0):
        self.lib = load()
        h = C.c_void_p()
        rc = self.lib.hite_ctx_create(int(device), C.byref(h))
        if rc != 0:
            raise HiteError("hite_ctx_create(device=%d) failed: %d (no usable GPU?)" % (device, rc))
        self.h = h
        self.device = device

    def copy_config(self, aligned_interval):
        """which interval the copy records of THIS context carry (include/hite_gpu.h hite_copy_config_ctx): True = the aligned interval
        as get_copies_minimap2 reports it (Util.py:8026; the default), False = the whole candidate (rounds 2-4), None = follow the
        process-wide setting again (hite_copy_config; HITE_COPY_INTERVAL = aligned | whole, else the default)"""
        self._check(self.lib.hite_copy_config_ctx(self.h, -1 if aligned_interval is None else int(bool(aligned_interval))), "hite_copy_config_ctx")

    def fill_config(self, tiles):
        """which form of the sparse fill THIS context runs (include/hite_gpu.h hite_fill_config_ctx): True = tiles of positions built in
        LDS (the default), False = the per-cell form, None = follow the process default again (HITE_FILL_TILES=0: the per-cell form).
        Both write the same bytes."""
        self._check(self.lib.hite_fill_config_ctx(self.h, -1 if tiles is None else int(bool(tiles))), "hite_fill_config_ctx")

    def gather_config(self, chunks):
        """which form of the fine stage's window gather THIS context runs (include/hite_gpu.h hite_gather_config_ctx): True = in chunks of
        the destination (the default), False = a wavefront per row, None = follow the process default again (HITE_GATHER_CHUNKS=0: per
        row).  Both write the same window bytes."""
        self._check(self.lib.hite_gather_config_ctx(self.h, -1 if chunks is None else int(bool(chunks))), "hite_gather_config_ctx")

    def gather_mode(self):
        """the form of the window gather the next call of this context runs: True = chunks, False = a wavefront per row"""
        m = self.lib.hite_gather_mode_ctx(self.h)
        if m < 0:
            raise HiteError("hite_gather_mode_ctx failed: %d" % m)
        return bool(m)

    def fallback_overlap(self, mode):
        """whether the star alignment of THIS context runs its fall-back alignment beside the layout of the candidates the fall-back does
        not touch (include/hite_gpu.h hite_fallback_overlap_ctx): True / 1 = beside (the default), False / 0 = one after the other,
        None / -1 = follow the process default again (HITE_FALLBACK_OVERLAP=0: one after the other).  Both give the same bytes."""
        self._check(self.lib.hite_fallback_overlap_ctx(self.h, -1 if mode is None or int(mode) < 0 else int(bool(mode))), "hite_fallback_overlap_ctx")

    def wide_tb_runs(self, mode):
        """which form of the fall-back alignment's traceback THIS context runs (include/hite_gpu.h hite_wide_tb_runs_ctx): True / 1 = by
        runs of up to 64 path steps per trip (the default), False / 0 = a column per step, None / -1 = follow the process default again
        (HITE_WIDE_TB_RUNS=0: a column per step).  Both write the same bytes."""
        self._check(self.lib.hite_wide_tb_runs_ctx(self.h, -1 if mode is None or int(mode) < 0 else int(bool(mode))), "hite_wide_tb_runs_ctx")

    def fill_tile_limits(self):
        """(positions of a tile, window-range bytes that fit the LDS slot, rows of a workgroup per trip, row slices) of the tile form"""
        out = (C.c_int32 * 4)()
        self._check(self.lib.hite_fill_tile_limits(out), "hite_fill_tile_limits")
        return tuple(out)

    def release_copy_index(self):
        """drops the minimizer index of the packed genome (device memory is freed); the next copy / seeding call rebuilds it"""
        if getattr(self, "_copy_state", None) is not None and getattr(self, "h", None):
            self.lib.hite_copy_index_release(self._copy_state)
        self._copy_state = None

    def close(self):
        self.release_copy_index()
        for lib in list(getattr(self, "_prot_libs", ())) + list(getattr(self, "_ltr_models", ())):      # before the context, like the copy-finder state
            lib.release()
        if getattr(self, "_pipe_state", None) is not None and getattr(self, "h", None):
            self.lib.hite_pipeline_release(self._pipe_state)
            self._pipe_state = C.c_void_p(None)
        if getattr(self, "h", None):
            self.lib.hite_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            msg = self.lib.hite_last_error(self.h)
            raise HiteError("%s failed: %d %s" % (what, rc, (msg or b"").decode(errors="replace")))

    # ---- genome ---------------------------------------------------------------------------
    def genome_pack(self, seqs):
        """seqs: list of str/bytes contigs (upper-case)."""
        bs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
        off = np.zeros(len(bs) + 1, dtype=np.int64)
        np.cumsum([len(b) for b in bs], out=off[1:])
        buf = np.frombuffer(b"".join(bs), dtype=np.uint8)
        self._check(self.lib.hite_genome_pack(self.h, _p(buf), _p(off), len(bs)), "hite_genome_pack")
        self.contig_len = np.diff(off)

    def set_contig_order(self, names):
        """contig names (in packing order) -> the byte order of "<name>:" that breaks length ties between alignment rows
        (tools/ready_for_MSA.sh); None clears it (contigs then compare by index)"""
        if names is None:
            self._check(self.lib.hite_set_contig_order(self.h, None, 0), "hite_set_contig_order")
            return
        keyed = sorted(range(len(names)), key=lambda i: (names[i] + ":").encode())
        rank = np.zeros(len(names), dtype=np.int32)
        rank[keyed] = np.arange(len(names), dtype=np.int32)
        self._check(self.lib.hite_set_contig_order(self.h, _p(rank), len(names)), "hite_set_contig_order")

    def genome_pack_dev(self, d_ptr, contig_off, stream=0):
        off = _arr(contig_off, np.int64)
        self._check(self.lib.hite_genome_pack_dev(self.h, C.c_void_p(d_ptr), _p(off), len(off) - 1, C.c_void_p(stream)),
                    "hite_genome_pack_dev")
        self.contig_len = np.diff(off)

    # ---- flank windows --------------------------------------------------------------------
    def flank_gather(self, contig, start1, end1, minus, flank=50):
        """-> (windows: list[bytes|None], trunc: list[bytes|None]) following Util.py:8095-8124"""
        n = len(contig)
        contig = _arr(contig, np.int32)
        start1 = _arr(start1, np.int64)
        end1 = _arr(end1, np.int64)
        minus = _arr(minus, np.uint8)
        ln = np.zeros(n, dtype=np.int64)
        tl = np.zeros(n, dtype=np.int64)
        self._check(self.lib.hite_flank_sizes(self.h, C.c_int64(n), _p(contig), _p(start1), _p(end1), int(flank), _p(ln), _p(tl)),
                    "hite_flank_sizes")
        pad = (ln + 15) // 16 * 16
        off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(pad, out=off[1:])
        tpad = (tl + 15) // 16 * 16
        toff = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(tpad, out=toff[1:])
        out = np.zeros(int(off[-1]) + 16, dtype=np.uint8)
        tout = np.zeros(int(toff[-1]) + 16, dtype=np.uint8)
        self._check(self.lib.hite_flank_gather(self.h, C.c_int64(n), _p(contig), _p(start1), _p(end1), _p(minus), int(flank),
                                               _p(off), _p(out), _p(toff), _p(tout)), "hite_flank_gather")
        wins = [out[off[i]:off[i] + ln[i]].tobytes() if ln[i] else None for i in range(n)]
        tr = [tout[toff[i]:toff[i] + tl[i]].tobytes() if tl[i] else None for i in range(n)]
        return wins, tr

    # ---- alignments -----------------------------------------------------------------------
    @staticmethod
    def pack_msas(msas):
        """msas: list of 2-D uint8 arrays -> (bytes, msa_off, rows, cols)"""
        rows = np.array([m.shape[0] for m in msas], dtype=np.int32)
        cols = np.array([m.shape[1] for m in msas], dtype=np.int32)
        sizes = rows.astype(np.int64) * cols
        pad = (sizes + 15) // 16 * 16
        off = np.zeros(len(msas) + 1, dtype=np.int64)
        np.cumsum(pad, out=off[1:])
        buf = np.full(int(off[-1]) + 16, ord("-"), dtype=np.uint8)
        for i, m in enumerate(msas):
            buf[off[i]:off[i] + sizes[i]] = np.ascontiguousarray(m, dtype=np.uint8).reshape(-1)
        return buf, off[:-1].copy(), rows, cols

    def sparse_cols(self, msas):
        buf, off, rows, cols = self.pack_msas(msas)
        out = np.zeros_like(buf)
        nc = np.zeros(len(msas), dtype=np.int32)
        self._check(self.lib.hite_sparse_cols(self.h, len(msas), _p(buf), _p(off), _p(rows), _p(cols), _p(out), _p(nc)),
                    "hite_sparse_cols")
        return [out[off[i]:off[i] + int(rows[i]) * int(nc[i])].reshape(int(rows[i]), int(nc[i])).copy() for i in range(len(msas))]

    def column_vote(self, msas):
        buf, off, rows, cols = self.pack_msas(msas)
        coff = np.zeros(len(msas) + 1, dtype=np.int64)
        np.cumsum(cols, out=coff[1:])
        counts = np.zeros((int(coff[-1]), 6), dtype=np.int32)
        self._check(self.lib.hite_column_vote(self.h, len(msas), _p(buf), _p(off), _p(rows), _p(cols), _p(coff), _p(counts)),
                    "hite_column_vote")
        return [counts[coff[i]:coff[i + 1]] for i in range(len(msas))]

    def boundary_search(self, msas, pos, side, thr, variant=3, int_thr=None, out_thr=None, win_in=20, win_out=10):
        buf, off, rows, cols = self.pack_msas(msas)
        n = len(msas)
        pos = _arr(pos, np.int32)
        side = _arr([0 if s in (0, "start") else 1 for s in side], np.int32)
        thr = _arr(thr, np.float64)
        it = _arr(int_thr, np.float64) if int_thr is not None else None
        ot = _arr(out_thr, np.float64) if out_thr is not None else None
        b = np.zeros(n, dtype=np.int32)
        v = np.zeros(n, dtype=np.int32)
        self._check(self.lib.hite_boundary_search(self.h, n, _p(buf), _p(off), _p(rows), _p(cols), _p(pos), _p(side), _p(thr),
                                                  _p(it), _p(ot), int(variant), win_in, win_out, _p(b), _p(v)),
                    "hite_boundary_search")
        return b, v

    def judge(self, te_type, msas, cands, plant=1):
        """-> list of (is_TE, info, cons, row_num, bstart, bend) -- the tuple judge_boundary_v5/v6/v9 return"""
        buf, off, rows, cols = self.pack_msas(msas)
        n = len(msas)
        cb = [c.encode() if isinstance(c, str) else bytes(c) for c in cands]
        coff = np.zeros(n + 1, dtype=np.int64)
        np.cumsum([len(c) for c in cb], out=coff[1:])
        cbuf = np.frombuffer(b"".join(cb) + b"\0" * 16, dtype=np.uint8)
        calls = np.zeros(n, dtype=CALL_DTYPE)
        cons = np.zeros(int(cols.astype(np.int64).sum()) + 8 * n + 16, dtype=np.uint8)
        self._check(self.lib.hite_judge(self.h, HITE_TE[te_type], int(plant), n, _p(buf), _p(off), _p(rows), _p(cols),
                                        _p(cbuf), _p(coff), _p(calls), _p(cons)), "hite_judge")
        out = []
        for i in range(n):
            c = calls[i]
            s = cons[c["cons_off"]:c["cons_off"] + c["cons_len"]].tobytes().decode() if c["is_te"] else ""
            out.append((bool(c["is_te"]), INFO[int(c["info"])], s, int(c["row_num"]), int(c["bstart"]), int(c["bend"])))
        return out

    def tsd_search(self, rows_, bstart, bend, plant=1):
        rb = [r.encode() if isinstance(r, str) else bytes(r) for r in rows_]
        n = len(rb)
        off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum([len(r) for r in rb], out=off[1:])
        buf = np.frombuffer(b"".join(rb) + b"\0" * 16, dtype=np.uint8)
        ln = np.zeros(n, dtype=np.int32)
        lo = np.zeros((n, 16), dtype=np.uint8)
        ro = np.zeros((n, 16), dtype=np.uint8)
        self._check(self.lib.hite_tsd_search(self.h, n, _p(buf), _p(off), _p(_arr(bstart, np.int32)), _p(_arr(bend, np.int32)),
                                             int(plant), _p(ln), _p(lo), _p(ro)), "hite_tsd_search")
        return [(lo[i, :max(ln[i], 0)].tobytes().decode(), ro[i, :max(ln[i], 0)].tobytes().decode(), int(ln[i])) for i in range(n)]

    # ---- star alignment (stage where the reference calls mafft) -------------------------------
    def align_config(self, exact_cap):
        """exact_cap: 0 = fast (band of 128 centre rows only); 8 / 16 / 32 = widest band (x 32 rows) tried for an optimality
        certificate (default 8 or $HITE_ALIGN_EXACT)"""
        self._check(self.lib.hite_align_config(self.h, int(exact_cap)), "hite_align_config")

    def align_lanes(self, min_cols):
        """which pairs the lane-parallel kernels take (hite_align_lanes): -1 = by the size of the call (default or
        $HITE_ALIGN_LANES), >= 0 = pairs of at least this many columns (0: all), -2 = none.  Never changes a result."""
        self._check(self.lib.hite_align_lanes(self.h, int(min_cols)), "hite_align_lanes")

    def align_stats(self, reset=False):
        """-> dict(pairs, certified, wide, fallback, dropped, cost, columns, exact_cap) accumulated since the last reset"""
        o = np.zeros(8, dtype=np.int64)
        self._check(self.lib.hite_align_stats(self.h, _p(o), 1 if reset else 0), "hite_align_stats")
        return dict(zip(("pairs", "certified", "wide", "fallback", "dropped", "cost", "columns", "exact_cap"), (int(x) for x in o)))

    def star_msa(self, groups, sparse=False, info=False):
        """groups: list of lists of windows (bytes/str), first window of each group = centre.
        -> list of 2-D uint8 alignments (None where the alignment failed); rows that cannot be aligned are dropped.
        sparse=True: the fused path, sparse columns (remove_sparse_col_in_align_file) already removed.
        info=True: also, per group, an int32 array (windows x 5): cost U, certified, status, k*, band words (| 0x100 fall-back)."""
        flat = [w.encode() if isinstance(w, str) else bytes(w) for g in groups for w in g]
        n = len(groups)
        row_first = np.zeros(n + 1, dtype=np.int32)
        np.cumsum([len(g) for g in groups], out=row_first[1:])
        off = np.zeros(len(flat) + 1, dtype=np.int64)
        np.cumsum([len(w) for w in flat], out=off[1:])
        buf = np.frombuffer(b"".join(flat) + b"\0" * 16, dtype=np.uint8)
        cols = np.zeros(n, dtype=np.int32)
        rows = np.zeros(n, dtype=np.int32)
        inf = np.zeros((len(flat), 5), dtype=np.int32)
        moff = np.zeros(max(n, 1), dtype=np.int64)
        if n == 0:
            return ([], []) if info else []
        # ONE call: the library allocates the result (the sizes-then-fill protocol of hite_star_msa ran the alignment twice)
        ptr = C.POINTER(C.c_uint8)()
        nbytes = C.c_int64(0)
        self._check(self.lib.hite_star_msa_once(self.h, n, _p(buf), _p(off), _p(row_first), 1 if sparse else 0, _p(cols), _p(rows),
                                                _p(inf) if info else None, C.byref(ptr), _p(moff), C.byref(nbytes)), "hite_star_msa_once")
        try:
            out = np.ctypeslib.as_array(ptr, shape=(max(int(nbytes.value), 1),)).copy() if nbytes.value > 0 else np.zeros(1, dtype=np.uint8)
        finally:
            self.lib.hite_host_free(C.cast(ptr, C.c_void_p))
        res = []
        for i in range(n):
            if cols[i] <= 0:
                res.append(None)
            else:
                res.append(out[moff[i]:moff[i] + int(rows[i]) * cols[i]].reshape(int(rows[i]), int(cols[i])).copy())
        if info:
            return res, [inf[row_first[i]:row_first[i + 1]].copy() for i in range(n)]
        return res

    # ---- the fine stage in one call (body of flank_region_align_v5 after copy finding) -----------
    def flank_region_align(self, te_type, cands, copies, plant=1, flank=50):
        """cands: list of candidate sequences; copies: list (per candidate) of
        (contig_index, start1, end1, minus) tuples.  Needs genome_pack() first.
        Tuples as find_copies(..., clips=True) returns them -- (contig, start1, end1, minus, anchors, clip) -- hand their clip
        words on (hite_flank_region_align_clip: rows padded by the clipped candidate bases); shorter tuples: no pads.
        -> (list of (is_TE, info, cons, row_num, bstart, bend), stats)"""
        n = len(cands)
        cb = [c.encode() if isinstance(c, str) else bytes(c) for c in cands]
        coff = np.zeros(n + 1, dtype=np.int64)
        np.cumsum([len(c) for c in cb], out=coff[1:])
        cbuf = np.frombuffer(b"".join(cb) + b"\0" * 16, dtype=np.uint8)
        cf = np.zeros(n + 1, dtype=np.int32)
        np.cumsum([len(c) for c in copies], out=cf[1:])
        flat = [t for c in copies for t in c]
        contig = _arr([t[0] for t in flat], np.int32)
        s1 = _arr([t[1] for t in flat], np.int64)
        e1 = _arr([t[2] for t in flat], np.int64)
        mn = _arr([t[3] for t in flat], np.uint8)
        # the clip words travel as the 6th field of the tuples (find_copies(clips=True)); tuples WITHOUT it -- the reference's own
        # (chr, start, end, length, strand) records -- get theirs estimated by the library (hite_clip_probe's rule)
        has = [len(t) > 5 for t in flat]
        if any(has) and not all(has):
            raise ValueError("flank_region_align: copy tuples with and without a clip field in one table")
        clip = _arr([t[5] for t in flat], np.uint32) if flat and all(has) else None
        calls = np.zeros(n, dtype=CALL_DTYPE)
        cap = int(coff[-1]) + (2 * flank + 64) * n + 4096
        stats = np.zeros(12, dtype=np.int64)
        for _attempt in range(2):
            cons = np.zeros(cap + 16, dtype=np.uint8)
            rc = self.lib.hite_flank_region_align_clip(self.h, HITE_TE[te_type], int(plant), n, _p(cbuf), _p(coff), _p(cf),
                                                       C.c_int64(len(flat)), _p(contig), _p(s1), _p(e1), _p(mn),
                                                       _p(clip) if clip is not None else None, int(flank),
                                                       _p(calls), _p(cons), C.c_int64(cap), _p(stats))
            if rc == -4 and stats[10] > cap:     # HITE_ECAP: the consensus pool was too small; stats[10] says how much is needed
                cap = int(stats[10]) + 4096
                continue
            break
        self._check(rc, "hite_flank_region_align")
        out = []
        for i in range(n):
            c = calls[i]
            s = cons[c["cons_off"]:c["cons_off"] + c["cons_len"]].tobytes().decode() if c["is_te"] else ""
            out.append((bool(c["is_te"]), INFO[int(c["info"])], s, int(c["row_num"]), int(c["bstart"]), int(c["bend"])))
        return out, stats

    def clip_probe(self, cands, copies):
        """the clip words hite_flank_region_align estimates for a table without them (hite_clip_probe): copies as for
        flank_region_align -> per candidate list of words (left | right << 16, in the orientation of the genome)"""
        n = len(cands)
        cb = [c.encode() if isinstance(c, str) else bytes(c) for c in cands]
        coff = np.zeros(n + 1, dtype=np.int64)
        np.cumsum([len(c) for c in cb], out=coff[1:])
        cbuf = np.frombuffer(b"".join(cb) + b"\0" * 16, dtype=np.uint8)
        cf = np.zeros(n + 1, dtype=np.int32)
        np.cumsum([len(c) for c in copies], out=cf[1:])
        flat = [t for c in copies for t in c]
        out = np.zeros(len(flat) + 1, dtype=np.uint32)
        self._check(self.lib.hite_clip_probe(self.h, n, _p(cbuf), _p(coff), _p(cf), C.c_int64(len(flat)), _p(_arr([t[0] for t in flat], np.int32)),
                                             _p(_arr([t[1] for t in flat], np.int64)), _p(_arr([t[2] for t in flat], np.int64)),
                                             _p(_arr([t[3] for t in flat], np.uint8)), _p(out)), "hite_clip_probe")
        return [[int(x) for x in out[cf[i]:cf[i + 1]]] for i in range(n)]

    def fine_rows(self, cands, copies, flank=50, rows_pass=0):
        """the rows one pass of the fine stage hands to the alignment (hite_fine_rows: the stage's own row selection and window
        gather): cands / copies as for flank_region_align (6-tuples carry their clip words, shorter ones are probed); rows_pass
        0 = pass A, 1 = pass B as if every first500 + last500 form had passed
        -> (per candidate list of (copy_index_within_candidate, window_bytes, trunc), totals = [rows, window bytes, longest row, 0])"""
        n = len(cands)
        cb = [c.encode() if isinstance(c, str) else bytes(c) for c in cands]
        coff = np.zeros(n + 1, dtype=np.int64)
        np.cumsum([len(c) for c in cb], out=coff[1:])
        cbuf = np.frombuffer(b"".join(cb) + b"\0" * 16, dtype=np.uint8)
        cf = np.zeros(n + 1, dtype=np.int32)
        np.cumsum([len(c) for c in copies], out=cf[1:])
        flat = [t for c in copies for t in c]
        has = [len(t) > 5 for t in flat]
        if any(has) and not all(has):
            raise ValueError("fine_rows: copy tuples with and without a clip field in one table")
        clip = _arr([t[5] for t in flat], np.uint32) if flat and all(has) else None
        args = (_p(_arr([t[0] for t in flat], np.int32)), _p(_arr([t[1] for t in flat], np.int64)), _p(_arr([t[2] for t in flat], np.int64)),
                _p(_arr([t[3] for t in flat], np.uint8)))
        nrows = np.zeros(n + 1, dtype=np.int32)
        totals = np.zeros(4, dtype=np.int64)
        row_cap = win_cap = 0
        for _attempt in range(2):
            row_copy = np.zeros(row_cap + 1, dtype=np.int32)
            row_len = np.zeros(row_cap + 1, dtype=np.int32)
            row_trunc = np.zeros(row_cap + 1, dtype=np.uint8)
            win_off = np.zeros(row_cap + 2, dtype=np.int64)
            win = np.zeros(win_cap + 16, dtype=np.uint8)
            rc = self.lib.hite_fine_rows(self.h, n, _p(cbuf), _p(coff), _p(cf), C.c_int64(len(flat)), *args,
                                         _p(clip) if clip is not None else None, int(flank), int(rows_pass), _p(nrows), C.c_int64(row_cap),
                                         _p(row_copy), _p(row_len), _p(row_trunc), _p(win_off), C.c_int64(win_cap), _p(win), _p(totals))
            if rc == -4 and (totals[0] > row_cap or totals[1] > win_cap):      # HITE_ECAP: totals say what is needed
                row_cap, win_cap = int(totals[0]), int(totals[1])
                continue
            break
        self._check(rc, "hite_fine_rows")
        out, r = [], 0
        for i in range(n):
            rows = []
            for _k in range(int(nrows[i])):
                o = int(win_off[r])
                rows.append((int(row_copy[r]) - int(cf[i]), win[o:o + int(row_len[r])].tobytes(), bool(row_trunc[r])))
                r += 1
            out.append(rows)
        assert r == int(totals[0]) and int(win_off[r]) == int(totals[1])
        return out, [int(x) for x in totals]

    # device-resident variant: every argument is a raw device pointer (e.g. torch tensor .data_ptr())
    def flank_region_align_dev(self, te_type, plant, n_cand, d_cand, d_cand_off, d_copy_first, n_copies, d_contig, d_start1,
                               d_end1, d_minus, flank, d_calls, d_cons, cons_cap, stream=0, d_clip=0):
        """d_clip: device pointer of the records' clip words (copy_clips_dev()), 0: the library estimates them (hite_clip_probe's rule)"""
        if not hasattr(self, "_pipe_state"):
            self._pipe_state = C.c_void_p(None)
        stats = np.zeros(12, dtype=np.int64)
        v = C.c_void_p
        rc = self.lib.hite_flank_region_align_clip_dev(self.h, C.byref(self._pipe_state), HITE_TE[te_type], int(plant), int(n_cand),
                                                       v(d_cand), v(d_cand_off), v(d_copy_first), C.c_int64(n_copies), v(d_contig),
                                                       v(d_start1), v(d_end1), v(d_minus), v(d_clip or None), int(flank), v(d_calls),
                                                       v(d_cons), C.c_int64(cons_cap), _p(stats), v(stream))
        self._check(rc, "hite_flank_region_align_clip_dev")
        return stats

    def profile(self, on=None, reset=False):
        """per-stage HIP-event timings recorded by the library on its launch stream"""
        if reset:
            self.lib.hite_profile_reset(self.h)
        if on is not None:
            self.lib.hite_profile_enable(self.h, 1 if on else 0)
        out = {}
        name = C.create_string_buffer(32)
        ms = C.c_double(0)
        cnt = C.c_int64(0)
        for i in range(self.lib.hite_profile_count(self.h)):
            if self.lib.hite_profile_get(self.h, i, name, C.byref(ms), C.byref(cnt)) == 0:
                out[name.value.decode()] = (ms.value, cnt.value)
        return out

    # ---- k-mer TSD seed matching (search_confident_tir_v4, Util.py:7734) -----------------------------
    def tsd_kmer(self, seqs, flank=50, plant=1):
        """-> per candidate list of (tsd_len, tir_start, tir_end, distance), canonical order, <= 100"""
        sb = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
        n = len(sb)
        off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum([len(s) for s in sb], out=off[1:])
        buf = np.frombuffer(b"".join(sb) + b"\0" * 16, dtype=np.uint8)
        rec = np.zeros((n, 100, 4), dtype=np.int32)
        cnt = np.zeros(n, dtype=np.int32)
        self._check(self.lib.hite_tsd_kmer(self.h, n, _p(buf), _p(off), int(flank), int(plant), _p(rec), _p(cnt)), "hite_tsd_kmer")
        return [[tuple(int(x) for x in rec[i, j]) for j in range(max(cnt[i], 0))] for i in range(n)]

    # ---- merge of the call records on a caller-owned RCCL communicator (no reference counterpart) ------------
    def allgather_records(self, nccl_comm, d_send, d_recv, bytes_per_rank, stream=None):
        """one ncclAllGather of bytes_per_rank bytes per rank (device pointers; nccl_comm = the caller's ncclComm_t as an int / c_void_p)"""
        self._check(self.lib.hite_allgather_records(self.h, C.c_void_p(nccl_comm), C.c_void_p(d_send), C.c_void_p(d_recv), C.c_int64(bytes_per_rank),
                                                    C.c_void_p(stream or 0)), "hite_allgather_records")

    # ---- terminal inverted repeats (run_itrsearch, Util.py:216: tools/itrsearch -i 0.7 -l 7) --------------------
    def itr_search(self, seqs, end_len=40, min_identity=0.7, min_len=7, match=10, mismatch=16, gap_open=32, gap_extend=32):
        """-> int32 [n, 8]: score, end1, end2, equal bases, aligned columns, found, "Length itr=", flags.  end_len > 0: the record
        is s[:end_len] + s[-end_len:] (search_confident_tir_batch_v1, Util.py:6564); end_len = 0: the whole sequence (remove_no_tirs)"""
        sb = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
        n = len(sb)
        out = np.zeros((n, 8), dtype=np.int32)
        if n == 0:
            return out
        off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum([len(s) for s in sb], out=off[1:])
        buf = np.frombuffer(b"".join(sb) + b"\0" * 16, dtype=np.uint8)
        self._check(self.lib.hite_itr_search(self.h, C.c_int64(n), _p(buf), _p(off), int(end_len), C.c_double(min_identity), int(min_len),
                                             int(match), int(mismatch), int(gap_open), int(gap_extend), _p(out)), "hite_itr_search")
        return out

    def itr_limits(self):
        """(cap on h, largest h with the traceback store in LDS, sequences per workgroup, grid cap on the LDS path, grid cap on the
        HBM path, columns of a strip) of itr_search_kernel"""
        out = (C.c_int32 * 6)()
        self._check(self.lib.hite_itr_limits(out), "hite_itr_limits")
        return tuple(out)

    # ---- pairwise identity (the -c / -A of cd-hit-est -aS 0.95 -aL 0.95 -c <c> -G 0 -g 1 -A 80) ---------------------------
    def pair_identity(self, seqs, pairs, band=32):
        """seqs: str / bytes; pairs: rows (a_id, a_start, a_end, b_id, b_start, b_end, strand), intervals 0-based and half-open, the
        second one reverse-complemented when strand != 0 -> int32 [n_pair, 2]: (cost, matches) of the banded edit alignment that
        include/hite_gpu.h defines ("pairwise identity"); (-1, 0) for a pair beyond a limit or outside its sequences.  The identity is
        matches / (cost + matches)."""
        pr = np.asarray(pairs, dtype=np.int64).reshape(-1, 7)
        n = len(pr)
        out = np.zeros((n, 2), dtype=np.int32)
        if n == 0:
            return out
        buf, off = self._csr(seqs)
        cost, mat = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        ai, bi = _arr(pr[:, 0], np.int32), _arr(pr[:, 3], np.int32)
        if (ai != pr[:, 0]).any() or (bi != pr[:, 3]).any():
            raise HiteError("pair_identity: a sequence id does not fit 32 bits")
        self._check(self.lib.hite_pair_identity(self.h, C.c_int64(len(off) - 1), _p(buf), _p(off), C.c_int64(n), _p(ai), _p(_arr(pr[:, 1], np.int64)),
                                                _p(_arr(pr[:, 2], np.int64)), _p(bi), _p(_arr(pr[:, 4], np.int64)), _p(_arr(pr[:, 5], np.int64)),
                                                _p(_arr(pr[:, 6] != 0, np.uint8)), C.c_int32(int(band)), _p(cost), _p(mat)), "hite_pair_identity")
        out[:, 0], out[:, 1] = cost, mat
        return out

    # ---- local alignments of pairs of intervals (the `blastn -query .. -subject .. -outfmt 6` of FiLTR's steps 1 and 2) -----
    def pair_hsps(self, seqs, pairs, diag_min=None):
        """seqs: str / bytes; pairs: rows (a_id, a_start, a_end, b_id, b_start, b_end), intervals 0-based and half-open -> per pair
        None (beyond HITE_PAIRHSP_MAX_LEN, empty, or outside its sequences) or the list of its HSPs, each the 7-tuple (q_start, q_end,
        s_start, s_end, score, matches, columns) with 1-based inclusive coordinates inside the intervals, in the order
        include/hite_gpu.h defines ("local alignments of pairs of intervals"; hite_pair_hsps).  Plus strand only; diag_min: only
        word hits and cells with s - q >= diag_min count (None: no limit)."""
        pr = np.asarray(pairs, dtype=np.int64).reshape(-1, 6)
        n = len(pr)
        if n == 0:
            self._check(self.lib.hite_pair_hsps(self.h, C.c_int64(0), None, None, C.c_int64(0), None, None, None, None, None, None, C.c_int32(0),
                                                C.c_int64(0), None, None, None, None), "hite_pair_hsps")
            return []
        buf, off = self._csr(seqs)
        ai, bi = _arr(pr[:, 0], np.int32), _arr(pr[:, 3], np.int32)
        if (ai != pr[:, 0]).any() or (bi != pr[:, 3]).any():
            raise HiteError("pair_hsps: a sequence id does not fit 32 bits")
        cols = [_arr(pr[:, k], np.int64) for k in (1, 2, 4, 5)]
        dm = -2 ** 31 if diag_min is None else int(diag_min)
        status, first, n_out = np.zeros(n, dtype=np.int32), np.zeros(n + 1, dtype=np.int64), C.c_int64(0)
        cap = 2 * n + 16
        while True:
            recs = np.zeros((cap, 7), dtype=np.int32)
            rc = self.lib.hite_pair_hsps(self.h, C.c_int64(len(off) - 1), _p(buf), _p(off), C.c_int64(n), _p(ai), _p(cols[0]), _p(cols[1]), _p(bi),
                                         _p(cols[2]), _p(cols[3]), C.c_int32(dm), C.c_int64(cap), _p(status), _p(first), _p(recs), C.byref(n_out))
            if rc == -4 and n_out.value > cap:       # HITE_ECAP: now the room is known
                cap = n_out.value
                continue
            self._check(rc, "hite_pair_hsps")
            break
        rows, at = recs[:n_out.value].tolist(), first.tolist()
        return [None if status[p] < 0 else [tuple(r) for r in rows[at[p]:at[p + 1]]] for p in range(n)]

    # ---- LTR candidate scan (where FiLTR runs LtrDetector, HiTE's other branch gt ltrharvest + LTR_FINDER) -------------------
    LTR_SCAN_STATS = ("words", "hits", "runs", "runs_span", "alignments", "redos", "no_hsp", "drop_ltr", "drop_len", "drop_overlap",
                      "drop_identity", "records")

    def ltr_scan(self, seqs, min_len=400, max_len=22000, min_ltr=100, max_ltr=6000, identity=85, stats=None, cap=1 << 14):
        """seqs: str / bytes -> int32 [n, 8]: (seq, ls, le, rs, re, score, matches, columns) of the LTR candidate scan that
        include/hite_gpu.h defines ("LTR candidate scan"; hite_ltr_scan): [ls, le) and [rs, re) are the two terminals, 0-based and
        half-open on the plus strand, ordered by (seq, ls, re, le, rs).  The defaults are LtrDetector's.  A result beyond `cap`
        records is asked again with the room it reported.  stats (a dict): the counters of this call (LTR_SCAN_STATS)."""
        buf, off = self._csr(seqs)
        room = int(cap)
        while True:
            recs = np.zeros((max(room, 1), 8), dtype=np.int32)
            n_out = C.c_int64(0)
            st = np.zeros(len(self.LTR_SCAN_STATS), dtype=np.int64)
            rc = self.lib.hite_ltr_scan(self.h, C.c_int64(len(off) - 1), _p(buf), _p(off), C.c_int32(int(min_len)), C.c_int32(int(max_len)),
                                        C.c_int32(int(min_ltr)), C.c_int32(int(max_ltr)), C.c_int32(int(identity)), C.c_int64(room), _p(recs),
                                        C.byref(n_out), _p(st))
            if rc == -4 and n_out.value > room:       # HITE_ECAP: now the room is known
                room = n_out.value
                continue
            self._check(rc, "hite_ltr_scan")
            break
        if stats is not None:
            stats.update(zip(self.LTR_SCAN_STATS, (int(v) for v in st)))
        return np.ascontiguousarray(recs[:n_out.value])

    # ---- genome annotation (where HiTE ends with RepeatMasker: annotate_genome.py:17, pan_annotate_genome.py:27) --------------
    ANNOTATE_STATS = ("table", "silenced", "too_long", "hits", "runs", "alignments", "redos", "no_hsp", "hsps", "duplicates", "dominated",
                      "records")

    def annotate(self, seqs, lib, piece_len=0, cap=None, stats=None):
        """seqs, lib: str / bytes (the genome's sequences, the library's entries) -> (int32 [n, 10], int8 [n_lib]): the records (seq,
        g_start, g_end, lib, strand, q_start, q_end, score, matches, columns) of the annotation that include/hite_gpu.h defines ("genome
        annotation"; hite_annotate) -- intervals 0-based and half-open, g on the plus strand of the sequence, q on the entry's forward
        strand, strand 1: the copy is the entry's reverse complement --, ordered by (seq, g_start, g_end, lib, strand, q_start), and
        per entry 0 or -1 (longer than HITE_ANNOT_MAX_LIB_LEN: not searched).  piece_len 0: HITE_ANNOT_PIECE.  A result beyond `cap`
        records is asked again with the room it reported.  stats (a dict): the counters of this call (ANNOTATE_STATS)."""
        buf, off = self._csr(seqs)
        lbuf, loff = self._csr(lib)
        n_lib = len(loff) - 1
        room = 1 << 14 if cap is None else int(cap)
        status = np.zeros(max(n_lib, 1), dtype=np.int8)
        while True:
            recs = np.zeros((max(room, 1), 10), dtype=np.int32)
            n_out = C.c_int64(0)
            st = np.zeros(len(self.ANNOTATE_STATS), dtype=np.int64)
            rc = self.lib.hite_annotate(self.h, C.c_int64(len(off) - 1), _p(buf), _p(off), C.c_int32(n_lib), _p(lbuf), _p(loff),
                                        C.c_int32(int(piece_len)), C.c_int64(room), _p(recs), C.byref(n_out), _p(status), _p(st))
            if rc == -4 and n_out.value > room:       # HITE_ECAP: now the room is known
                room = n_out.value
                continue
            self._check(rc, "hite_annotate")
            break
        if stats is not None:
            stats.update(zip(self.ANNOTATE_STATS, (int(v) for v in st)))
        return np.ascontiguousarray(recs[:n_out.value]), status[:n_lib].copy()

    # ---- Helitron candidate scan (multi_process_helitronscanner, Util.py:263: HelitronScanner.jar) ---------------------------
    def _helitron_args(self, seqs, head_patterns, tail_patterns):
        buf, off = self._csr(seqs)
        hp, tp = _arr(head_patterns, LCV_DTYPE).reshape(-1), _arr(tail_patterns, LCV_DTYPE).reshape(-1)
        return buf, off, [C.c_int64(len(off) - 1), _p(buf), _p(off), C.c_int32(len(hp)), _p(hp), C.c_int32(len(tp)), _p(tp)], (hp, tp)

    def helitron_scan(self, seqs, head_patterns, tail_patterns, head_threshold=1, tail_threshold=1, len_range=(200, 20000), stats=None,
                      cap=1 << 16):
        """seqs: str / bytes; patterns: LCV_DTYPE records (util.parse_lcvs) -> int32 [n, 6]: (seq, start, end, strand, head score,
        tail score) of the Helitron candidate scan that include/hite_gpu.h defines, ordered by (seq, strand, start, end); start / end
        are 0-based, half-open, on the forward strand.  A result beyond `cap` records is asked again with the room it reported.
        stats (a dict): anchors, heads, tails, pairs of this call."""
        buf, off, args, keep = self._helitron_args(seqs, head_patterns, tail_patterns)
        room = int(cap)
        while True:
            out = np.zeros((5, max(room, 1)), dtype=np.int32)
            strand = np.zeros(max(room, 1), dtype=np.uint8)
            n_out = C.c_int64(0)
            st = np.zeros(4, dtype=np.int64)
            rc = self.lib.hite_helitron_scan(self.h, *args, C.c_int32(int(head_threshold)), C.c_int32(int(tail_threshold)),
                                             C.c_int32(int(len_range[0])), C.c_int32(int(len_range[1])), C.c_int64(out.shape[1]),
                                             _p(out[0]), _p(out[1]), _p(out[2]), _p(strand), _p(out[3]), _p(out[4]), C.byref(n_out), _p(st))
            if rc == -4 and n_out.value > out.shape[1]:       # HITE_ECAP: now the room is known
                room = n_out.value
                continue
            self._check(rc, "hite_helitron_scan")
            break
        k = n_out.value
        if stats is not None:
            stats.update(zip(("anchors", "heads", "tails", "pairs"), (int(v) for v in st)))
        return np.ascontiguousarray(np.stack([out[0, :k], out[1, :k], out[2, :k], strand[:k].astype(np.int32), out[3, :k], out[4, :k]], axis=1))

    def helitron_scores(self, seqs, head_patterns, tail_patterns):
        """-> int32 [4, total bytes]: the head / tail scores of every position (rows: plus heads, plus tails, minus heads, minus tails;
        the minus rows in the coordinates of the reverse complement), sequence k at columns sum(len(seqs[:k])) ..."""
        buf, off, args, keep = self._helitron_args(seqs, head_patterns, tail_patterns)
        out = np.zeros((4, int(off[-1])), dtype=np.int32)
        self._check(self.lib.hite_helitron_scores(self.h, *args, _p(out)), "hite_helitron_scores")
        return out

    # ---- translated protein search (get_domain_info, Util.py:4571: blastx -evalue 1e-20 -outfmt 6) -------------------
    @staticmethod
    def _csr(seqs):
        sb = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
        off = np.zeros(len(sb) + 1, dtype=np.int64)
        np.cumsum([len(s) for s in sb], out=off[1:])
        return np.frombuffer(b"".join(sb) + b"\0" * 16, dtype=np.uint8), off

    def translate6(self, seqs):
        """-> per sequence its six frames (+1 +2 +3 -1 -2 -3) as str: standard code, X for a codon with a non-ACGT base, * for a stop"""
        n = len(seqs)
        if n == 0:
            return []
        buf, off = self._csr(seqs)
        foff = np.zeros(6 * n + 1, dtype=np.int64)
        out = np.zeros(int(off[-1]) * 2 + 16, dtype=np.uint8)       # six frames of L bases hold at most 2 L residues
        self._check(self.lib.hite_translate6(self.h, C.c_int64(n), _p(buf), _p(off), C.c_int64(len(out)), _p(out), _p(foff)), "hite_translate6")
        txt = out.tobytes()
        return [[txt[foff[6 * q + f]:foff[6 * q + f + 1]].decode() for f in range(6)] for q in range(n)]

    def protein_lib(self, proteins):
        """proteins (str / bytes, letters) -> the handle protein_search takes: the seed index of the library on the device.  Released by
        its release(), or by close() before the context."""
        return ProteinLib(self, proteins)

    def protein_search(self, queries, lib, evalue=1e-20, stats=None, batch_bases=1 << 20, cap=1 << 16):
        """the HSPs of `blastx -evalue <evalue> -outfmt 6` by the definition in include/hite_gpu.h -> int32 [n, 10]: query, protein,
        frame (+-1..3), q_start, q_end, s_start, s_end, raw score, identical columns, columns; ordered by (query, score descending,
        protein, frame, q_start, s_start).  The queries go to the library in batches of about batch_bases bases; a batch whose
        HSPs exceed `cap` is asked again with the room it reported.  stats (a dict): seed hits, survivors, tasks are added up."""
        if lib.ctx is not self or lib.h is None:
            raise HiteError("protein_search: the library handle belongs to another context or was released")
        sb = [s.encode() if isinstance(s, str) else bytes(s) for s in queries]
        parts = []
        a = 0
        while a < len(sb):
            b, nb = a, 0
            while b < len(sb) and (b == a or nb + len(sb[b]) <= batch_bases):
                nb += len(sb[b])
                b += 1
            buf, off = self._csr(sb[a:b])
            room = int(cap)
            while True:
                out = np.zeros((10, max(room, 1)), dtype=np.int32)
                n_out = C.c_int64(0)
                st = np.zeros(3, dtype=np.int64)
                rc = self.lib.hite_protein_search(self.h, lib.h, C.c_int64(b - a), _p(buf), _p(off), C.c_double(evalue), C.c_int64(out.shape[1]),
                                                  *[_p(out[k]) for k in range(10)], C.byref(n_out), _p(st))
                if rc == -4 and n_out.value > out.shape[1]:       # HITE_ECAP: now the room is known
                    room = n_out.value
                    continue
                self._check(rc, "hite_protein_search")
                break
            rec = np.ascontiguousarray(out[:, :n_out.value].T)
            rec[:, 0] += a
            parts.append(rec)
            if stats is not None:
                for k, name in enumerate(("hits", "survivors", "tasks")):
                    stats[name] = stats.get(name, 0) + int(st[k])
            a = b
        return np.concatenate(parts) if parts else np.zeros((0, 10), dtype=np.int32)

    def protein_smin(self, m, n, evalue):
        """the smallest raw score whose E-value m n K exp(-lambda S) is <= evalue (host arithmetic of the library)"""
        s = C.c_int32(0)
        self._check(self.lib.hite_protein_smin(C.c_int64(m), C.c_int64(n), C.c_double(evalue), C.byref(s)), "hite_protein_smin")
        return s.value

    # ---- FMEA (get_longest_repeats_v4 + process_all_seqs, Util.py:4122) --------------------------------
    def fmea_chain(self, qseg, sseg, qs, qe, ss, se, seg_chrom, seg_off, skip_gap, max_len):
        """-> (chrom ids, starts, ends) of the longest_repeats keys, in the reference's insertion order"""
        n = len(qseg)
        a = lambda x, t: _arr(x, t)  # noqa: E731
        qseg, sseg = a(qseg, np.int32), a(sseg, np.int32)
        qs, qe, ss, se = a(qs, np.int64), a(qe, np.int64), a(ss, np.int64), a(se, np.int64)
        seg_chrom, seg_off = a(seg_chrom, np.int32), a(seg_off, np.int64)
        cap = max(16, n + 16)
        oc = np.zeros(cap, dtype=np.int32)
        os_ = np.zeros(cap, dtype=np.int64)
        oe = np.zeros(cap, dtype=np.int64)
        nout = C.c_int64(0)
        self._check(self.lib.hite_fmea_chain(self.h, C.c_int64(n), _p(qseg), _p(sseg), _p(qs), _p(qe), _p(ss), _p(se), len(seg_chrom),
                                             _p(seg_chrom), _p(seg_off), C.c_int64(skip_gap), C.c_int64(max_len), C.c_int64(cap),
                                             _p(oc), _p(os_), _p(oe), C.byref(nout)), "hite_fmea_chain")
        k = nout.value
        return oc[:k].copy(), os_[:k].copy(), oe[:k].copy()

    # ---- copy finding (stage where the reference calls minimap2, Util.py:7933) ---------------------------
    FIND_COPIES_BATCH = 1 << 18

    def find_copies_table(self, cands, restricted=False, clips=False):
        """the copy table as arrays: (copy_first int32[n + 1], contig, start1, end1, minus, anchors) -- the copies of candidate c are
        rows copy_first[c] .. copy_first[c + 1]; needs genome_pack() first; at most FIND_COPIES_BATCH candidates.
        clips=True: a 7th array, uint32 per record: the candidate bases the end extensions clipped, left | right << 16 in the
        orientation of the genome (hite_copy_clips) -- zero when the records carry the whole-candidate interval
        (hite_copy_config(0)); flank_region_align pads the rows of the star alignment with them.
        restricted=True: the caller uses the index of this genome for THIS candidate set only (the masking step of stage 3.1):
        hite_find_copies_restricted builds the index from just the genome minimizers the candidates look up -- same table,
        a fraction of the build; any later use of the handle rebuilds the full index by itself."""
        if getattr(self, "_copy_state", None) is None:
            self._copy_state = C.c_void_p(None)
        cb = [c.encode() if isinstance(c, str) else bytes(c) for c in cands]
        n = len(cb)
        if n > self.FIND_COPIES_BATCH:
            raise ValueError("find_copies_table: %d candidates in one call (limit %d)" % (n, self.FIND_COPIES_BATCH))
        off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum([len(c) for c in cb], out=off[1:])
        buf = np.frombuffer(b"".join(cb) + b"\0" * 16, dtype=np.uint8)
        cap = 300 * n + 16
        cf = np.zeros(n + 1, dtype=np.int32)
        ct = np.zeros(cap, dtype=np.int32)
        s1 = np.zeros(cap, dtype=np.int64)
        e1 = np.zeros(cap, dtype=np.int64)
        mn = np.zeros(cap, dtype=np.uint8)
        an = np.zeros(cap, dtype=np.int32)
        nout = C.c_int64(0)
        fn = self.lib.hite_find_copies_restricted if restricted else self.lib.hite_find_copies
        self._check(fn(self.h, C.byref(self._copy_state), n, _p(buf), _p(off), C.c_int64(cap), _p(cf), _p(ct), _p(s1), _p(e1), _p(mn),
                       _p(an), C.byref(nout)), "hite_find_copies_restricted" if restricted else "hite_find_copies")
        k = int(cf[n])
        if clips:
            cl = np.zeros(k + 1, dtype=np.uint32)
            self._check(self.lib.hite_copy_clips(self._copy_state, C.c_int64(k + 1), _p(cl)), "hite_copy_clips")
            return cf, ct[:k], s1[:k], e1[:k], mn[:k], an[:k], cl[:k]
        return cf, ct[:k], s1[:k], e1[:k], mn[:k], an[:k]

    def find_copies(self, cands, restricted=False, clips=False):
        """-> per candidate list of (contig, start1, end1, minus, anchors); needs genome_pack() first (restricted, clips: see
        find_copies_table; clips=True appends the packed clip word to every tuple: flank_region_align reads it from there)"""
        if len(cands) > self.FIND_COPIES_BATCH:    # one device call handles < 2^19 candidates: larger libraries go in batches
            out = []
            for k in range(0, len(cands), self.FIND_COPIES_BATCH):     # (batches share one full index)
                out += self.find_copies(cands[k:k + self.FIND_COPIES_BATCH], clips=clips)
            return out
        tab = self.find_copies_table(cands, restricted, clips)
        cf, ct, s1, e1, mn, an = tab[:6]
        rows = list(zip(ct.tolist(), s1.tolist(), e1.tolist(), mn.tolist(), an.tolist(), *([tab[6].tolist()] if clips else [])))
        cf = cf.tolist()
        return [rows[cf[c]:cf[c + 1]] for c in range(len(cands))]

    def copy_index_build(self, stream=0, fresh=False):
        """fresh: the minimizer tiles the handle keeps from its last build are dropped first (hite_copy_index_forget)"""
        if getattr(self, "_copy_state", None) is None:
            self._copy_state = C.c_void_p(None)
        if fresh:
            self.lib.hite_copy_index_forget(self._copy_state)
        self._check(self.lib.hite_copy_index_build(self.h, C.byref(self._copy_state), C.c_void_p(stream)), "hite_copy_index_build")

    def find_copies_dev(self, n_cand, d_cand, d_cand_off, cand_bytes, stream=0):
        """device-resident: -> (n_copies, d_copy_first, d_contig, d_start1, d_end1, d_minus, d_anchors) raw device pointers.
        PRECONDITION (include/hite_gpu.h): the buffer at d_cand is readable for 16 bytes beyond cand_bytes -- allocate
        cand_bytes + 16 (the end extension fetches candidate words ahead of use)."""
        v = C.c_void_p
        outs = [v() for _ in range(6)]
        n = C.c_int64(0)
        rc = self.lib.hite_find_copies_dev(self.h, self._copy_state, int(n_cand), v(d_cand), v(d_cand_off), C.c_int64(cand_bytes),
                                           C.byref(outs[0]), C.byref(n), C.byref(outs[1]), C.byref(outs[2]), C.byref(outs[3]),
                                           C.byref(outs[4]), C.byref(outs[5]), v(stream))
        self._check(rc, "hite_find_copies_dev")
        return (n.value,) + tuple(o.value or 0 for o in outs)

    def copy_clips_dev(self):
        """raw device pointer of the clip words of the last find_copies_dev call's records (0: none) -- the d_clip of flank_region_align_dev"""
        d = C.c_void_p()
        n = C.c_int64(0)
        self._check(self.lib.hite_copy_clips_dev(self._copy_state, C.byref(d), C.byref(n)), "hite_copy_clips_dev")
        return d.value or 0

    # ---- full-length copy support of the intact LTR elements (FiLTR's step 4; include/hite_gpu.h) -----------------------------
    @staticmethod
    def _std_arrays(std):
        std = list(std)
        return (_arr([t[0] for t in std], np.int32), _arr([t[1] for t in std], np.int64), _arr([t[2] for t in std], np.int64))

    @staticmethod
    def _support_rows(n, of, oc, os_, oe):
        of = of.tolist()
        rows = list(zip(oc[:of[n]].tolist(), os_[:of[n]].tolist(), oe[:of[n]].tolist()))
        return [rows[of[k]:of[k + 1]] for k in range(n)]

    def ltr_copy_support_records(self, el_len, records, std, contig_len, full_length_coverage=0.985, overlap_threshold=0.95,
                                 segment_len=100000, cap=None, stats=None):
        """hite_ltr_copy_support_records: el_len[k] bases of element k, records[k] its copy records (contig, start1, end1, clip) in
        input order (clip = left | right << 16, as find_copies(clips=True) gives it); std: (contig, start, end) per candidate line in
        the order of ltr_lines (start = lLTR_start - 1, end = rLTR_end); contig_len per contig -> per element the list of
        (contig, start1, end1) kept.  cap: room for the output (None: every record); stats: a dict that receives the four counts.
        A HiteError of code HITE_ECAP carries .n_out, the room the call needs."""
        n = len(el_len)
        cf = np.zeros(n + 1, dtype=np.int64)
        np.cumsum([len(r) for r in records], out=cf[1:])
        if len(records) != n or cf[n] >= 2 ** 31:
            raise ValueError("ltr_copy_support_records: one list of records per element, fewer than 2^31 records in all")
        flat = [t for r in records for t in r]
        ct, s1, e1 = _arr([t[0] for t in flat], np.int32), _arr([t[1] for t in flat], np.int64), _arr([t[2] for t in flat], np.int64)
        cl = _arr([t[3] for t in flat], np.uint32)
        sc, ss, se = self._std_arrays(std)
        clen = _arr(contig_len, np.int64)
        cap = len(flat) if cap is None else int(cap)
        of = np.zeros(n + 1, dtype=np.int32)
        oc, os_, oe = np.zeros(cap + 1, dtype=np.int32), np.zeros(cap + 1, dtype=np.int64), np.zeros(cap + 1, dtype=np.int64)
        nout = C.c_int64(0)
        st = np.zeros(4, dtype=np.int64)
        rc = self.lib.hite_ltr_copy_support_records(self.h, C.c_int64(n), _p(_arr(el_len, np.int64)), _p(cf.astype(np.int32)), _p(ct), _p(s1), _p(e1),
                                                    _p(cl), C.c_int64(len(sc)), _p(sc), _p(ss), _p(se), C.c_int32(len(clen)), _p(clen),
                                                    C.c_double(full_length_coverage), C.c_double(overlap_threshold), C.c_int64(segment_len),
                                                    C.c_int64(cap), _p(of), _p(oc), _p(os_), _p(oe), C.byref(nout), _p(st))
        return self._support_result(rc, "hite_ltr_copy_support_records", n, of, oc, os_, oe, nout, st, stats)

    def _support_result(self, rc, what, n, of, oc, os_, oe, nout, st, stats):
        if stats is not None:
            stats.update(zip(("records", "covered", "matched", "kept"), (int(x) for x in st)))
        if rc != 0:
            try:
                self._check(rc, what)
            except HiteError as e:
                e.code, e.n_out = rc, nout.value
                raise
        return self._support_rows(n, of, oc, os_, oe)

    def ltr_copy_support(self, elements, std, full_length_coverage=0.985, overlap_threshold=0.95, segment_len=100000, stats=None):
        """hite_ltr_copy_support: the elements (str / bytes) against the packed genome (genome_pack() first) -- the copy finder in
        aligned-interval mode, then the rules of get_copies_minimap2 and get_intact_ltr_copies on its table where it lies on the
        device -> per element the list of (contig, start1, end1) kept; std, stats: see ltr_copy_support_records.  More than
        FIND_COPIES_BATCH elements go in batches that share the index; the order of equally long copies of an element on different
        contigs follows the contigs' first appearance inside the batch."""
        if getattr(self, "_copy_state", None) is None:
            self._copy_state = C.c_void_p(None)
        eb = [e.encode() if isinstance(e, str) else bytes(e) for e in elements]
        sc, ss, se = self._std_arrays(std)
        out, tot = [], np.zeros(4, dtype=np.int64)
        for k in range(0, len(eb), self.FIND_COPIES_BATCH):
            part = eb[k:k + self.FIND_COPIES_BATCH]
            n = len(part)
            off = np.zeros(n + 1, dtype=np.int64)
            np.cumsum([len(e) for e in part], out=off[1:])
            buf = np.frombuffer(b"".join(part) + b"\0" * 16, dtype=np.uint8)
            cap = 300 * n
            of = np.zeros(n + 1, dtype=np.int32)
            oc, os_, oe = np.zeros(cap + 1, dtype=np.int32), np.zeros(cap + 1, dtype=np.int64), np.zeros(cap + 1, dtype=np.int64)
            nout = C.c_int64(0)
            st = np.zeros(4, dtype=np.int64)
            rc = self.lib.hite_ltr_copy_support(self.h, C.byref(self._copy_state), C.c_int32(n), _p(buf), _p(off), C.c_int64(len(sc)), _p(sc), _p(ss),
                                                _p(se), C.c_double(full_length_coverage), C.c_double(overlap_threshold), C.c_int64(segment_len),
                                                C.c_int64(cap), _p(of), _p(oc), _p(os_), _p(oe), C.byref(nout), _p(st))
            tot += st
            out += self._support_result(rc, "hite_ltr_copy_support", n, of, oc, os_, oe, nout, tot, stats)
        if stats is not None and not eb:
            stats.update(dict.fromkeys(("records", "covered", "matched", "kept"), 0))
        return out

    def query_copies(self, qid, sid, qs, qe, ss, se, ident, qlen, slen=None, ns=None, qcov=0.95, scov=0.0, qthr=200, sthr=200, max_copy=100):
        """get_query_copies on an HSP table in file order -> per query list of (subject id, start, end, chain length, '+'/'-')"""
        n = len(qid)
        a = lambda x, t: _arr(x, t)  # noqa: E731
        qid, sid = a(qid, np.int32), a(sid, np.int32)
        qs, qe, ss, se = a(qs, np.int64), a(qe, np.int64), a(ss, np.int64), a(se, np.int64)
        ident = a(ident, np.float64) if ident is not None else None
        qlen = a(qlen, np.int64)
        nq = len(qlen)
        slen = a(slen, np.int64) if slen is not None else None
        if ns is None:
            ns = len(slen) if slen is not None else (int(sid.max()) + 1 if n else 1)
        cap = (max_copy + 1) * nq + 16
        cf = np.zeros(nq + 1, dtype=np.int64)
        osid = np.zeros(cap, dtype=np.int32)
        os_, oe, ol = (np.zeros(cap, dtype=np.int64) for _ in range(3))
        om = np.zeros(cap, dtype=np.uint8)
        nout = C.c_int64(0)
        self._check(self.lib.hite_query_copies(self.h, C.c_int64(n), _p(qid), _p(sid), _p(qs), _p(qe), _p(ss), _p(se),
                                               _p(ident) if ident is not None else None, nq, _p(qlen), int(ns),
                                               _p(slen) if slen is not None else None, C.c_double(qcov), C.c_double(scov), C.c_int64(qthr),
                                               C.c_int64(sthr), int(max_copy), C.c_int64(cap), _p(cf), _p(osid), _p(os_), _p(oe), _p(ol),
                                               _p(om), C.byref(nout)), "hite_query_copies")
        return [[(int(osid[i]), int(os_[i]), int(oe[i]), int(ol[i]), "-" if om[i] else "+") for i in range(cf[q], cf[q + 1])]
                for q in range(nq)]

    def chain_all(self, qid, sid, qs, qe, ss, se, nq, ns, qgap):
        """every chain of every cluster (hite_chain_all: the core of FMEA / get_full_length_copies_from_blastn_v1) ->
        per query list of (subject id, q_start, q_end, s_start, s_end, extend_num) in the reference's order"""
        n = len(qid)
        qid, sid = _arr(qid, np.int32), _arr(sid, np.int32)
        qs, qe, ss, se = _arr(qs, np.int64), _arr(qe, np.int64), _arr(ss, np.int64), _arr(se, np.int64)
        gap = _arr(qgap, np.int64)
        cap = n + 16
        cf = np.zeros(nq + 1, dtype=np.int64)
        osid, onext = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32)
        oqs, oqe, oss, ose = (np.zeros(cap, dtype=np.int64) for _ in range(4))
        tot = C.c_int64(0)
        self._check(self.lib.hite_chain_all(self.h, C.c_int64(n), _p(qid), _p(sid), _p(qs), _p(qe), _p(ss), _p(se), int(nq), int(ns), _p(gap),
                                            C.c_int64(cap), _p(cf), _p(osid), _p(oqs), _p(oqe), _p(oss), _p(ose), _p(onext), C.byref(tot)),
                    "hite_chain_all")
        return [[(int(osid[i]), int(oqs[i]), int(oqe[i]), int(oss[i]), int(ose[i]), int(onext[i])) for i in range(cf[q], cf[q + 1])]
                for q in range(nq)]

    def lib_chain(self, qid, sid, qs, qe, ss, se, seq_len, threshold, chunk_size=0):
        """library-vs-itself HSP table -> chain records [chunk, q, qs-1, qe, s, ss-1, se] in the reference's chunk-file order"""
        n = len(qid)
        a = lambda x, t: _arr(x, t)  # noqa: E731
        qid, sid = a(qid, np.int32), a(sid, np.int32)
        qs, qe, ss, se = a(qs, np.int64), a(qe, np.int64), a(ss, np.int64), a(se, np.int64)
        sl = a(seq_len, np.int64)
        cap = n + 16
        oc, oq, os_ = (np.zeros(cap, dtype=np.int32) for _ in range(3))
        oqs, oqe, oss, ose = (np.zeros(cap, dtype=np.int64) for _ in range(4))
        nout = C.c_int64(0)
        self._check(self.lib.hite_lib_chain(self.h, C.c_int64(n), _p(qid), _p(sid), _p(qs), _p(qe), _p(ss), _p(se), len(sl), _p(sl),
                                            C.c_double(threshold), C.c_int64(chunk_size), C.c_int64(cap), _p(oc), _p(oq), _p(oqs), _p(oqe),
                                            _p(os_), _p(oss), _p(ose), C.byref(nout)), "hite_lib_chain")
        k = nout.value
        return [[int(oc[i]), int(oq[i]), int(oqs[i]), int(oqe[i]), int(os_[i]), int(oss[i]), int(ose[i])] for i in range(k)]

    def lib_cluster(self, recs, seq_len, threshold):
        """chain records -> clusters (lists of sequence ids: the query, then the subjects in the order they joined)"""
        n = len(recs)
        col = lambda k, t: _arr([r[k] for r in recs], t)  # noqa: E731
        ch, q, qs, qe, s, ss, se = col(0, np.int32), col(1, np.int32), col(2, np.int64), col(3, np.int64), col(4, np.int32), col(5, np.int64), col(6, np.int64)
        sl = _arr(seq_len, np.int64)
        capc, capm = n + 2, 2 * n + 2
        cf = np.zeros(capc + 1, dtype=np.int64)
        mem = np.zeros(capm, dtype=np.int32)
        ncl = C.c_int64(0)
        self._check(self.lib.hite_lib_cluster(C.c_int64(n), _p(ch), _p(q), _p(qs), _p(qe), _p(s), _p(ss), _p(se), len(sl), _p(sl),
                                              C.c_double(threshold), C.c_int64(capc), C.c_int64(capm), _p(cf), _p(mem), C.byref(ncl)),
                    "hite_lib_cluster")
        return [[int(x) for x in mem[cf[c]:cf[c + 1]]] for c in range(ncl.value)]

    def msa_consensus(self, alignments):
        """batch of alignments (each a list of equal-length byte strings) -> list of consensus strings (cons_from_mafft_v1)"""
        nmat = len(alignments)
        if nmat == 0:
            return []
        rows = np.array([len(al) for al in alignments], dtype=np.int32)
        cols = np.array([len(al[0]) for al in alignments], dtype=np.int64)
        flat = []
        for al in alignments:
            for r in al:
                rb = r.encode() if isinstance(r, str) else bytes(r)
                if len(rb) != len(al[0]):
                    raise ValueError("ragged alignment")
                flat.append(rb)
        buf = np.frombuffer(b"".join(flat) + b"\0" * 16, dtype=np.uint8)
        moff = np.zeros(nmat + 1, dtype=np.int64)
        np.cumsum(rows.astype(np.int64) * cols, out=moff[1:])
        ooff = np.zeros(nmat + 1, dtype=np.int64)
        np.cumsum(cols, out=ooff[1:])
        cons = np.zeros(int(ooff[-1]) + 16, dtype=np.uint8)
        clen = np.zeros(nmat, dtype=np.int64)
        self._check(self.lib.hite_msa_consensus(self.h, nmat, _p(rows), _p(cols), _p(moff), _p(buf), _p(ooff), _p(cons), _p(clen)),
                    "hite_msa_consensus")
        return [cons[ooff[a]:ooff[a] + clen[a]].tobytes().decode("latin-1") for a in range(nmat)]

    def msa_subcluster(self, alignments, cutoff=0.2):
        """batch of alignments (each a list of equal-length byte strings or a 2-D uint8 array) -> per alignment the sub-clusters of its
        rows, a list of lists of row indices in order of their leaders: the leader clustering include/hite_gpu.h defines
        (hite_msa_subcluster; the value util.ninja_stand_in returns, where the reference runs Ninja)"""
        nmat = len(alignments)
        if nmat == 0:
            self._check(self.lib.hite_msa_subcluster(self.h, 0, None, None, None, None, C.c_double(cutoff), None, None, None),
                        "hite_msa_subcluster")
            return []
        rows = np.zeros(nmat, dtype=np.int32)
        cols = np.zeros(nmat, dtype=np.int64)
        flat = []
        for a, al in enumerate(alignments):
            if isinstance(al, np.ndarray):
                if al.ndim != 2:
                    raise ValueError("msa_subcluster: an alignment array has two dimensions")
                rows[a], cols[a] = al.shape
                flat.append(np.ascontiguousarray(al, dtype=np.uint8).reshape(-1))
                continue
            rb = [r.encode("latin-1") if isinstance(r, str) else bytes(r) for r in al]
            if any(len(r) != len(rb[0]) for r in rb):
                raise ValueError("ragged alignment")
            rows[a], cols[a] = len(rb), len(rb[0]) if rb else 0
            flat.append(np.frombuffer(b"".join(rb), dtype=np.uint8))
        buf = np.concatenate(flat + [np.zeros(16, dtype=np.uint8)])
        moff = np.zeros(nmat + 1, dtype=np.int64)
        np.cumsum(rows.astype(np.int64) * cols, out=moff[1:])
        roff = np.zeros(nmat + 1, dtype=np.int64)
        np.cumsum(rows, out=roff[1:])
        sub = np.zeros(int(roff[-1]) + 1, dtype=np.int32)
        nsub = np.zeros(nmat, dtype=np.int32)
        self._check(self.lib.hite_msa_subcluster(self.h, nmat, _p(rows), _p(cols), _p(moff), _p(buf), C.c_double(cutoff), _p(roff), _p(sub),
                                                 _p(nsub)), "hite_msa_subcluster")
        sub, at, out = sub.tolist(), roff.tolist(), []
        for a, k in enumerate(nsub.tolist()):
            groups = [[] for _ in range(k)]
            for r, g in enumerate(sub[at[a]:at[a + 1]]):
                groups[g].append(r)
            out.append(groups)
        return out

    def frame_cluster(self, groups, ident, cov_short=0.0, cov_long=0.0, min_cov=0, min_len=10, both_strands=True):
        """batch of groups (each a list of short sequences, str or bytes, gap-free) -> per group its clusters in order of creation,
        each a list of row indices (the representative, then the rows that joined it, in the order they joined), or None for a group
        beyond HITE_FRAMECLUSTER_MAX_ROWS / HITE_FRAMECLUSTER_MAX_LEN: the greedy clustering include/hite_gpu.h defines
        (hite_frame_cluster; where FiLTR runs `cd-hit-est -c ident -aS cov_short -aL cov_long -A min_cov -l min_len`).  Rows of
        length <= min_len are in no cluster."""
        ng = len(groups)
        flat = [r.encode("latin-1") if isinstance(r, str) else bytes(r) for g in groups for r in g]
        roff = np.zeros(ng + 1, dtype=np.int64)
        np.cumsum([len(g) for g in groups], out=roff[1:])
        soff = np.zeros(len(flat) + 1, dtype=np.int64)
        np.cumsum([len(r) for r in flat], out=soff[1:])
        buf = np.frombuffer(b"".join(flat) + b"\0" * 16, dtype=np.uint8)
        cl = np.zeros(len(flat) + 1, dtype=np.int32)
        ncl = np.zeros(ng + 1, dtype=np.int32)
        self._check(self.lib.hite_frame_cluster(self.h, C.c_int64(ng), _p(roff), _p(buf), _p(soff), C.c_double(ident), C.c_double(cov_short),
                                                C.c_double(cov_long), C.c_int32(min_cov), C.c_int32(min_len), C.c_int32(int(bool(both_strands))),
                                                _p(cl), _p(ncl)), "hite_frame_cluster")
        cl, lens, at, out = cl.tolist(), np.diff(soff).tolist(), roff.tolist(), []
        for g, k in enumerate(ncl[:ng].tolist()):
            if k < 0:
                out.append(None)
                continue
            cls = [[] for _ in range(k)]
            r0 = at[g]
            for r in sorted(range(at[g + 1] - r0), key=lambda r: (-lens[r0 + r], r)):
                if cl[r0 + r] >= 0:
                    cls[cl[r0 + r]].append(r)
            out.append(cls)
        return out

    # ---- high-copy LTR vote of FiLTR's hybrid CNN (hite_ltr_deep) ---------------------------------------------------------------
    def ltr_model(self, params):
        """the canonical flat fp32 array of HITE_LTRDEEP_PARAMS parameters (util.ltr_model_params / util.load_ltr_model) -> a model
        resident on the device (hite_ltr_model_build folds the batch norms); released with the context or by .release()"""
        return LtrModel(self, params)

    @staticmethod
    def _ltr_deep_rows(matrices):
        """matrices: {name: rows} or a list of them, a row being (left frame, right frame) or one string -> (bytes of the rows of
        200, row offsets).  A matrix with a row that is not 200 wide goes up without rows: it is not scored."""
        mats = list(matrices.values()) if isinstance(matrices, dict) else list(matrices)
        flat, counts = [], []
        for m in mats:
            rb = [("".join(r) if isinstance(r, (tuple, list)) else r) for r in m]
            rb = [r.encode("latin-1") if isinstance(r, str) else bytes(r) for r in rb]
            if any(len(r) != LTRDEEP_COLS for r in rb):
                rb = []
            flat.extend(rb)
            counts.append(len(rb))
        roff = np.zeros(len(mats) + 1, dtype=np.int64)
        np.cumsum(counts, out=roff[1:])
        return np.frombuffer(b"".join(flat) + b"\0" * 16, dtype=np.uint8), roff

    def ltr_deep(self, model, matrices, pooled=False):
        """the two logits of FiLTR's hybrid CNN for every matrix (in the order of `matrices`): float32 [n, 2], (with pooled=True the
        64 pooled values [n, 64],) int8 status [n]: 0 scored, 1 not scored (fewer than 5 or more than 100 rows, or a row that is not
        200 wide; its logits are 0).  include/hite_gpu.h, "high-copy LTR vote"."""
        buf, roff = self._ltr_deep_rows(matrices)
        n = len(roff) - 1
        logits = np.zeros((n, 2), dtype=np.float32)
        pool = np.zeros((n, 64), dtype=np.float32)
        status = np.zeros(n, dtype=np.int8)
        self._check(self.lib.hite_ltr_deep(self.h, model.h, C.c_int64(n), _p(buf), _p(roff), _p(logits), _p(pool) if pooled else None,
                                           _p(status)), "hite_ltr_deep")
        return (logits, pool, status) if pooled else (logits, status)

    def ltr_deep_features(self, matrices):
        """the integer features of hite_ltr_deep by themselves: uint8 image [n, 3, 100, 200], int32 k-mer counts [n, 2, 3872], int8
        status [n] (the features of a matrix that is not scored are 0)"""
        buf, roff = self._ltr_deep_rows(matrices)
        n = len(roff) - 1
        img = np.zeros((n, 3, LTRDEEP_ROWS, LTRDEEP_COLS), dtype=np.uint8)
        kmer = np.zeros((n, 2, LTRDEEP_KMER), dtype=np.int32)
        status = np.zeros(n, dtype=np.int8)
        self._check(self.lib.hite_ltr_deep_features(self.h, C.c_int64(n), _p(buf), _p(roff), _p(img), _p(kmer), _p(status)),
                    "hite_ltr_deep_features")
        return img, kmer, status

    def ltr_both_ends(self, alignments, cur_seqs, flank):
        """FiLTR get_both_ends_frame on a batch: alignments = lists of equal-length rows, cur_seqs = terminal sequences ->
        per alignment None (boundary not found) or (frames [(left, right)], full rows, new_start, new_end)"""
        n = len(alignments)
        if n == 0:
            return []
        rows = np.array([len(al) for al in alignments], dtype=np.int32)
        cols = np.array([len(al[0]) if al else 0 for al in alignments], dtype=np.int32)
        flat = []
        for al in alignments:
            for r in al:
                rb = r.encode() if isinstance(r, str) else bytes(r)
                if len(rb) != len(al[0]):
                    raise ValueError("ragged alignment")
                flat.append(rb)
        buf = np.frombuffer(b"".join(flat) + b"\0" * 16, dtype=np.uint8)
        moff = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(rows.astype(np.int64) * cols, out=moff[1:])
        cb = [c.encode() if isinstance(c, str) else bytes(c) for c in cur_seqs]
        coff = np.zeros(n + 1, dtype=np.int64)
        np.cumsum([len(c) for c in cb], out=coff[1:])
        cbuf = np.frombuffer(b"".join(cb) + b"\0" * 16, dtype=np.uint8)
        froff = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(rows.astype(np.int64) * 2 * flank, out=froff[1:])
        fuoff = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(rows.astype(np.int64) * (2 * flank + cols.astype(np.int64)), out=fuoff[1:])
        frames = np.zeros(int(froff[-1]) + 16, dtype=np.uint8)
        full = np.zeros(int(fuoff[-1]) + 16, dtype=np.uint8)
        fcols = np.zeros(n, dtype=np.int32)
        npos = np.zeros(2 * n, dtype=np.int32)
        status = np.zeros(n, dtype=np.int32)
        self._check(self.lib.hite_ltr_both_ends(self.h, n, _p(buf), _p(moff), _p(rows), _p(cols), _p(cbuf), _p(coff), int(flank), _p(frames),
                                                _p(froff), _p(full), _p(fuoff), _p(fcols), _p(npos), _p(status)), "hite_ltr_both_ends")
        out = []
        for a in range(n):
            if status[a] != 0:
                out.append(None)
                continue
            R, stride = int(rows[a]), 2 * flank + int(cols[a])
            fr = [(frames[froff[a] + r * 2 * flank:froff[a] + r * 2 * flank + flank].tobytes().decode("latin-1"),
                   frames[froff[a] + r * 2 * flank + flank:froff[a] + (r + 1) * 2 * flank].tobytes().decode("latin-1")) for r in range(R)]
            fu = [full[fuoff[a] + r * stride:fuoff[a] + r * stride + fcols[a]].tobytes().decode("latin-1") for r in range(R)]
            out.append((fr, fu, int(npos[2 * a]), int(npos[2 * a + 1])))
        return out

    def nonltr_prep(self, seqs, flank=50, win5=25):
        """search_polyA_TSD on a batch -> [(found_TSD, direct, tsd_start, tsd_len, lo, hi)]"""
        sb = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
        n = len(sb)
        off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum([len(s) for s in sb], out=off[1:])
        buf = np.frombuffer(b"".join(sb) + b"\0" * 16, dtype=np.uint8)
        out = np.zeros(6 * max(1, n), dtype=np.int64)
        self._check(self.lib.hite_nonltr_prep(self.h, n, _p(buf), _p(off), int(flank), int(win5), _p(out)), "hite_nonltr_prep")
        return [tuple(int(x) for x in out[6 * i:6 * i + 6]) for i in range(n)]

    def ltr_frame(self, matrices, flank, window=20, side="left"):
        """FiLTR flank-frame vote on a batch: matrices = list of lists of equal-length frame strings -> [(is_ltr, boundary)]"""
        n = len(matrices)
        rows = np.array([len(m) for m in matrices], dtype=np.int32)
        cols = np.array([len(m[0]) if m else 0 for m in matrices], dtype=np.int32)
        off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(rows.astype(np.int64) * cols, out=off[1:])
        buf = np.frombuffer(("".join("".join(m) for m in matrices)).encode() + b"\0" * 16, dtype=np.uint8)
        ok = np.zeros(n, dtype=np.int32)
        b = np.zeros(n, dtype=np.int32)
        self._check(self.lib.hite_ltr_frame(self.h, n, _p(buf), _p(off), _p(rows), _p(cols), int(flank), int(window),
                                            0 if side == "left" else 1, _p(ok), _p(b)), "hite_ltr_frame")
        return [(bool(o), int(x)) for o, x in zip(ok, b)]

    def genome_mask(self, contig, start1, end1):
        """N-mask the 1-based inclusive intervals of the resident genome (mask_genome_intactTE)"""
        c, a, b = _arr(contig, np.int32), _arr(start1, np.int64), _arr(end1, np.int64)
        self._check(self.lib.hite_genome_mask(self.h, C.c_int64(len(c)), _p(c), _p(a), _p(b)), "hite_genome_mask")

    def seed_segments(self, seg_len=1_000_000):
        """-> (seg_chrom int32[nseg], seg_off int64[nseg]): the 'chr$offset' segment table of the packed genome"""
        n = C.c_int32(0)
        self._check(self.lib.hite_seed_segments(self.h, C.c_int64(seg_len), 0, None, None, C.byref(n)), "hite_seed_segments")
        sc = np.zeros(max(1, n.value), dtype=np.int32)
        so = np.zeros(max(1, n.value), dtype=np.int64)
        self._check(self.lib.hite_seed_segments(self.h, C.c_int64(seg_len), n.value, _p(sc), _p(so), C.byref(n)), "hite_seed_segments")
        return sc[:n.value], so[:n.value]

    def seed_shard(self, rank, world):
        """the seeding calls of this context compute rank's share of `world` (hite_seed_shard); world <= 1: everything"""
        self._check(self.lib.hite_seed_shard(self.h, int(rank), int(world)), "hite_seed_shard")
        self._seed_shard = (int(rank), int(world)) if int(world) > 1 else (0, 0)

    def _seed_allvsall_once(self, seg_len, max_anchors, cap):
        """one hite_seed_allvsall call -> (table or None, anchors): None when the call's anchors exceed what one call sorts"""
        if getattr(self, "_copy_state", None) is None:
            self._copy_state = C.c_void_p(None)
        stats = (C.c_int64 * 4)()
        n = C.c_int64(0)
        cap = int(cap) if cap is not None else 1 << 20
        while True:
            qseg = np.empty(cap, dtype=np.int32); sseg = np.empty(cap, dtype=np.int32)
            qs = np.empty(cap, dtype=np.int64); qe = np.empty(cap, dtype=np.int64)
            ss = np.empty(cap, dtype=np.int64); se = np.empty(cap, dtype=np.int64)
            rc = self.lib.hite_seed_allvsall(self.h, C.byref(self._copy_state), C.c_int64(seg_len), C.c_int64(max_anchors), C.c_int64(cap),
                                             _p(qseg), _p(sseg), _p(qs), _p(qe), _p(ss), _p(se), C.byref(n), stats)
            if rc == -4 and n.value > cap:   # HITE_ECAP with the needed size known: retry once with room
                cap = n.value + 16
                continue
            if rc == -4 and (int(stats[1]) > max_anchors or int(stats[1]) >= 0xffffffff):
                return None, int(stats[1])
            self._check(rc, "hite_seed_allvsall")
            break
        k = n.value
        return {"qseg": qseg[:k].copy(), "sseg": sseg[:k].copy(), "qs": qs[:k].copy(), "qe": qe[:k].copy(), "ss": ss[:k].copy(),
                "se": se[:k].copy(), "stats": tuple(int(x) for x in stats)}, int(stats[1])

    def seed_allvsall(self, seg_len=1_000_000, max_anchors=2_000_000_000, cap=None):
        """all-vs-all seeding of the packed genome -> dict(qseg, sseg, qs, qe, ss, se, stats): the HSP table fmea_chain takes.
        A search with more anchors than one call sorts (the merged library of eight population genomes: dozens of near-identical
        sequences per family, 5 x 10^9 anchors) runs in SHARES, one after the other -- the (strand, diagonal) ranges of hite_seed_shard,
        whose union, put in share order and sorted stably by (query segment, subject segment), is the whole table record for record
        (what hite_amd.dist does across ranks).
        A context that is itself a rank's shard (seed_shard(r, W)) splits ITS share (seed_sub_shard: rank r S + s of world W S) and
        is the shard (r, W) again afterwards."""
        tab, anchors = self._seed_allvsall_once(seg_len, max_anchors, cap)
        if tab is not None:
            return tab
        rank0, world0 = getattr(self, "_seed_shard", (0, 0))
        world = 2
        while world * max_anchors < 2 * anchors:
            world *= 2
        while True:
            if max(world0, 1) * world > 256:
                raise HiteError("hite_seed_allvsall: %d anchors do not fit %d shares" % (anchors, max(world0, 1) * world // 2))
            parts = []
            try:
                for s in range(world):
                    self.seed_shard(*seed_sub_shard(rank0, world0, s, world))
                    t, _a = self._seed_allvsall_once(seg_len, max_anchors, cap)
                    if t is None:
                        break
                    parts.append(t)
            finally:
                self.seed_shard(rank0, world0)
            if len(parts) == world:
                break
            world *= 2
        cat = {k: np.concatenate([t[k] for t in parts]) for k in ("qseg", "sseg", "qs", "qe", "ss", "se")}
        order = np.lexsort((cat["sseg"], cat["qseg"]))          # (stable: equal keys stay in share order)
        out = {k: v[order] for k, v in cat.items()}
        st = np.asarray([t["stats"] for t in parts], dtype=np.int64)
        out["stats"] = (int(st[0, 0]), int(st[:, 1].sum()), int(st[:, 2].sum()), int(st[:, 3].sum()))
        out["shares"] = world
        return out

    def coarse_stage_dev(self, seg_len, seg_chrom, seg_off, skip_gap, max_len, max_anchors=8_000_000_000):
        """all-vs-all seeding + FMEA with the HSP table kept on the device -> ((chrom ids, starts, ends), seeding stats)"""
        if getattr(self, "_copy_state", None) is None:
            self._copy_state = C.c_void_p(None)
        v = C.c_void_p
        ptr = [v() for _ in range(6)]
        stats = (C.c_int64 * 4)()
        n = C.c_int64(0)
        self._check(self.lib.hite_seed_allvsall_dev(self.h, C.byref(self._copy_state), C.c_int64(seg_len), C.c_int64(max_anchors),
                                                    *[C.byref(x) for x in ptr], C.byref(n), stats), "hite_seed_allvsall_dev")
        sc, so = _arr(seg_chrom, np.int32), _arr(seg_off, np.int64)
        cap = max(16, n.value + 16)
        oc = np.empty(cap, dtype=np.int32); os_ = np.empty(cap, dtype=np.int64); oe = np.empty(cap, dtype=np.int64)
        nout = C.c_int64(0)
        if n.value:
            self._check(self.lib.hite_fmea_chain_dev(self.h, n, *ptr, len(sc), _p(sc), _p(so), C.c_int64(skip_gap), C.c_int64(max_len),
                                                     C.c_int64(cap), _p(oc), _p(os_), _p(oe), C.byref(nout)), "hite_fmea_chain_dev")
        k = nout.value
        return (oc[:k].copy(), os_[:k].copy(), oe[:k].copy()), tuple(int(x) for x in stats)

    def copy_stats(self):
        """sizes of the last find_copies call: (candidate minimizers, index hits, diagonal clusters, copies before the cap)"""
        out = (C.c_int64 * 4)()
        self._check(self.lib.hite_copy_stats(self._copy_state, out), "hite_copy_stats")
        return tuple(int(x) for x in out)

    def tr_mask(self, max_period=500):
        """tandem repeats of the resident genome -> N (in place, for every later stage); returns a bool array over the
        concatenated contigs (True = masked) -- the build's stage where the reference runs TRF (Util.py:2855)"""
        G = int(self.lib.hite_genome_bases(self.h))
        bits = np.zeros((G + 31) // 32 + 1, dtype=np.uint32)
        n = C.c_int64(0)
        self._check(self.lib.hite_tr_mask(self.h, int(max_period), _p(bits), C.byref(n)), "hite_tr_mask")
        m = np.unpackbits(bits.view(np.uint8), bitorder="little")[:G].astype(bool)
        assert int(m.sum()) == n.value
        return m

    def tr_mask_dev(self, max_period=500):
        """tr_mask without the bit map on the host: the resident genome is masked in place -> number of masked bases"""
        n = C.c_int64(0)
        self._check(self.lib.hite_tr_mask(self.h, int(max_period), None, C.byref(n)), "hite_tr_mask")
        return int(n.value)

    def flanking_seq_dev(self, chrom, start0, end0, flank, contig_len=None):
        """generate_final_result + flanking_seq (Util.py:4783, 4614) for intervals (contig id, 0-based start, end) of the resident
        genome: the window of each interval with `flank` bases either side, clamped into the contig as the reference clamps it
        -> total bytes gathered (hite_flank_gather: coordinates up, sequences down)"""
        c = _arr(chrom, np.int32)
        if len(c) == 0:
            return 0
        if contig_len is None:
            contig_len = self.contig_len
        clen = np.asarray(contig_len, dtype=np.int64)[c]
        s1 = _arr(start0, np.int64) + 1
        e1 = _arr(end0, np.int64).copy()
        s1 = np.where(s1 - 1 - flank < 0, flank + 1, s1)
        e1 = np.where(e1 + flank > clen, clen - flank, e1)
        n = len(c)
        ws, we, mn = np.ascontiguousarray(s1 - flank), np.ascontiguousarray(e1 + flank), np.zeros(n, dtype=np.uint8)
        ln, tl = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        self._check(self.lib.hite_flank_sizes(self.h, C.c_int64(n), _p(c), _p(ws), _p(we), 0, _p(ln), _p(tl)), "hite_flank_sizes")
        off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum((ln + 15) // 16 * 16, out=off[1:])
        # flanking_seq wants the whole window only (the first500 + last500 form belongs to the copy windows of the fine stage); the
        # host buffer is kept between calls: fresh pages would be faulted in under the copy
        need = int(off[-1]) + 16
        if getattr(self, "_flank_out", None) is None or len(self._flank_out) < need:
            self._flank_out = np.empty(need + need // 8, dtype=np.uint8)
        out = self._flank_out
        self._check(self.lib.hite_flank_gather(self.h, C.c_int64(n), _p(c), _p(ws), _p(we), _p(mn), 0, _p(off), _p(out), None, None),
                    "hite_flank_gather")
        self.flank_windows = (out, off, ln)      # (bytes, 16-byte aligned offsets, lengths) of the last call
        return int(ln.sum())

    def copy_stats_ext(self):
        """copy_stats() + (chains with a long end to extend, the other chains, DP columns of the end extension, 0)"""
        out = (C.c_int64 * 8)()
        self._check(self.lib.hite_copy_stats_ext(self._copy_state, out), "hite_copy_stats_ext")
        return tuple(int(x) for x in out)

    def download(self, d_ptr, count, dtype):
        """numpy copy of `count` elements of `dtype` at raw device pointer d_ptr"""
        out = np.zeros(int(count), dtype=dtype)
        if count:
            self._check(self.lib.hite_memcpy_d2h(_p(out), C.c_void_p(d_ptr), C.c_int64(out.nbytes)), "hite_memcpy_d2h")
        return out


class ProteinLib:
    """a protein library resident on the device (hite_protein_lib_build): residue codes + the 20^4-bucket seed directory"""

    def __init__(self, ctx, proteins):
        self.ctx = ctx
        self.h = None
        buf, off = Context._csr(proteins)
        self.n_prot = len(off) - 1
        self.n_res = int(off[-1])
        h = C.c_void_p(None)
        ctx._check(ctx.lib.hite_protein_lib_build(ctx.h, C.c_int64(self.n_prot), _p(buf), _p(off), C.byref(h)), "hite_protein_lib_build")
        self.h = h
        if not hasattr(ctx, "_prot_libs"):
            ctx._prot_libs = []
        ctx._prot_libs.append(self)

    def release(self):
        if self.h is not None and getattr(self.ctx, "h", None):
            self.ctx.lib.hite_protein_lib_release(self.h)
        self.h = None
        if self in getattr(self.ctx, "_prot_libs", ()):
            self.ctx._prot_libs.remove(self)


class LtrModel:
    """the parameters of FiLTR's hybrid CNN resident on the device (hite_ltr_model_build): batch norms folded, weights laid out for
    the convolution kernels"""

    def __init__(self, ctx, params):
        self.ctx = ctx
        self.h = None
        params = _arr(params, np.float32).reshape(-1)
        h = C.c_void_p(None)
        ctx._check(ctx.lib.hite_ltr_model_build(ctx.h, _p(params), C.c_int64(params.size), C.byref(h)), "hite_ltr_model_build")
        self.h = h
        if not hasattr(ctx, "_ltr_models"):
            ctx._ltr_models = []
        ctx._ltr_models.append(self)

    def release(self):
        if self.h is not None and getattr(self.ctx, "h", None):
            self.ctx.lib.hite_ltr_model_release(self.h)
        self.h = None
        if self in getattr(self.ctx, "_ltr_models", ()):
            self.ctx._ltr_models.remove(self)
