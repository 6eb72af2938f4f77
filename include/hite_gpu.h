/*
 * hite_gpu.h -- C ABI of libhite_gpu.so: the MI355X-native (gfx950, HIP) implementation of
 * HiTE's dynamic-boundary-adjustment hot path.  Plain pointers and sizes only.
 *
 * HiTE is pure Python: it has no FFI today.  Each entry point below replaces the inside of
 * one Python function of /root/reference/module/Util.py (cited per function); the binding a
 * maintainer adds is the ctypes stub shown in INTEGRATION.md (hite_amd/_lib.py is that stub).
 *
 * Conventions
 *  - every function returns 0 on success or a negative HITE_E* code; nothing aborts.
 *  - "host" entry points take host pointers (numpy buffers) and copy in/out;
 *    "_dev" entry points take DEVICE pointers and a hipStream_t (as void*), launch
 *    asynchronously on that stream and never synchronise (bench / pipelines / torch tensors).
 *  - strings cross the boundary as uint8 arrays + int64 CSR offsets, never char**.
 *  - an alignment ("msa") is rows x cols bytes, row-major, alphabet ACGTN and '-' (any other
 *    byte is folded to 'N' on entry, the same folding getReverseSequence applies, Util.py:1635).
 *  - thread-safety: one hite_ctx per thread / per GPU; no global HIP state before the first call.
 */
#ifndef HITE_GPU_H
#define HITE_GPU_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* A row window handed to the star alignment may BEGIN and END with runs of PAD bytes (never the centre, row 0 of a candidate): bytes
 * with bit 5 set -- HITE_ROW_PAD ('.'), which matches nothing (1 per column against a centre base instead of 3 per base of a gap), or a
 * base in LOWER CASE (a, c, g, t), which matches its base.  Genome and candidate bytes are upper case: no pad is ever mistaken.  Pads
 * take part in the pairwise alignment and are removed afterwards -- centre positions aligned to them become gaps of the row, the ops
 * refer to the row without them.  hite_flank_region_align_clip[_dev] pads the rows of copy records in the reference's coordinates with
 * the centre's own bases in lower case (see there). */
#define HITE_ROW_PAD 0x2e   /* '.' */
#define HITE_IS_ROW_PAD(c) (((c) & 0x20u) != 0)

#define HITE_OK 0
#define HITE_EINVAL (-1)   /* bad argument */
#define HITE_ENOMEM (-2)   /* host or device allocation failed */
#define HITE_EHIP (-3)     /* HIP runtime error (hite_last_error() has the text) */
#define HITE_ECAP (-4)     /* caller-provided output capacity too small */
#define HITE_ENODEV (-5)   /* no usable GPU */

#define HITE_TE_TIR 0      /* judge_boundary_v5  Util.py:9145 */
#define HITE_TE_HELITRON 1 /* judge_boundary_v6  Util.py:9821 */
#define HITE_TE_NON_LTR 2  /* judge_boundary_v9  Util.py:9483 */

#define HITE_INFO_NONE 0   /* ''    */
#define HITE_INFO_NB 1     /* 'nb'  : anchor not found */
#define HITE_INFO_FL1 2    /* 'fl1' : <= 1 full-length row */
#define HITE_INFO_EXC 3    /* the reference would raise a Python exception on this input */

typedef struct hite_ctx hite_ctx;

/* One boundary call = the tuple judge_boundary_v5/v6/v9 return (is_TE, info, cons_seq, row_num)
 * plus the final boundary columns the reference only prints in debug mode.  32 bytes; this is also
 * the record all-gathered between GPUs. */
typedef struct hite_call {
    int32_t is_te;
    int32_t info;
    int32_t row_num;
    int32_t bstart;   /* final_boundary_start column (-1 if none) */
    int32_t bend;     /* final_boundary_end column   (-1 if none) */
    int32_t cons_len; /* consensus length */
    int64_t cons_off; /* offset of the consensus inside the caller's cons pool */
} hite_call;

/* ---- context ------------------------------------------------------------------------- */
int hite_ctx_create(int device_id, hite_ctx **out);
void hite_ctx_destroy(hite_ctx *ctx);
const char *hite_last_error(hite_ctx *ctx);
int hite_version(void);

/* ---- genome residency (2-bit bases + 1-bit non-ACGT mask in HBM) ------------------------
 * Replaces the per-stage `read_fasta(reference)` (Util.py:1650, called at :8073, :4616, :4788).
 * seq = all contigs concatenated (upper-cased ASCII), contig_off[n_contigs+1] CSR. */
int hite_genome_pack(hite_ctx *ctx, const uint8_t *seq, const int64_t *contig_off, int32_t n_contigs);
/* same, from an ASCII buffer already in device memory (async on `stream`) */
int hite_genome_pack_dev(hite_ctx *ctx, const uint8_t *d_seq, const int64_t *contig_off_host, int32_t n_contigs,
                         void *stream);
int64_t hite_genome_bases(hite_ctx *ctx);
/* Byte order of the contig names, each followed by ':' (rank[i] = position of contig i): tools/ready_for_MSA.sh keeps the 100
 * longest windows and breaks length ties by window NAME "<contig>:<start>-<end>(<strand>)" (`sort -nk 2 -r` on the .fai,
 * POSIX locale; Util.py:8110, 10410).  Optional: without it contigs compare by their index.  Cleared by hite_genome_pack. */
int hite_set_contig_order(hite_ctx *ctx, const int32_t *rank, int32_t n);
/* N-mask intervals (contig id, 1-based inclusive, clamped into the contig) of the resident genome: the masking step of
 * mask_genome_intactTE (Util.py:6389-6431).  A minimizer index built before the call does not see the mask. */
int hite_genome_mask(hite_ctx *ctx, int64_t n, const int32_t *contig, const int64_t *start1, const int64_t *end1);

/* ---- flank-window gather --- Util.py:8095-8124 (inside flank_region_align_v5) -------------
 * copy i = (contig[i], start1[i], end1[i]) 1-based inclusive, minus[i] = strand '-'.
 * Pass 1 (sizes): out_len[i] = window length, 0 if the reference skips the copy (off-contig
 *   :8103 or shorter than 100 :8108); trunc_len[i] = 1000 if window > 1000 (:8117) else 0.
 * Pass 2 (fill): windows written at out_off[i] (caller's exclusive scan of out_len), the
 *   first500+last500 form at trunc_off[i] when trunc_len[i] != 0 (trunc_* may be NULL). */
int hite_flank_sizes(hite_ctx *ctx, int64_t n, const int32_t *contig, const int64_t *start1, const int64_t *end1,
                     int32_t flank, int64_t *out_len, int64_t *trunc_len);
int hite_flank_sizes_dev(hite_ctx *ctx, int64_t n, const int32_t *d_contig, const int64_t *d_start1,
                         const int64_t *d_end1, int32_t flank, int64_t *d_out_len, int64_t *d_trunc_len, void *stream);
int hite_flank_gather(hite_ctx *ctx, int64_t n, const int32_t *contig, const int64_t *start1, const int64_t *end1,
                      const uint8_t *minus, int32_t flank, const int64_t *out_off, uint8_t *out,
                      const int64_t *trunc_off, uint8_t *trunc_out);
int hite_flank_gather_dev(hite_ctx *ctx, int64_t n, const int32_t *d_contig, const int64_t *d_start1,
                          const int64_t *d_end1, const uint8_t *d_minus, int32_t flank, const int64_t *d_out_off,
                          uint8_t *d_out, const int64_t *d_trunc_off, uint8_t *d_trunc_out, void *stream);

/* ---- sparse-column removal --- remove_sparse_col_in_align_file  Util.py:10344-10405 --------
 * batch of n alignments: msa_off[i] = byte offset of alignment i, rows[i] x cols[i].
 * Writes the cleaned alignment IN THE SAME SLOT of `out` (offset msa_off[i], row stride
 * new_cols[i]) and new_cols[i]. */
int hite_sparse_cols(hite_ctx *ctx, int32_t n, const uint8_t *msa, const int64_t *msa_off, const int32_t *rows,
                     const int32_t *cols, uint8_t *out, int32_t *new_cols);
/* device-resident: d_col_off = exclusive scan of cols (n+1), total_cols = its last element;
 * d_out must not alias d_msa. */
int hite_sparse_cols_dev(hite_ctx *ctx, int32_t n, const uint8_t *d_msa, const int64_t *d_msa_off,
                         const int32_t *d_rows, const int32_t *d_cols, const int64_t *d_col_off, int64_t total_cols,
                         uint8_t *d_out, int32_t *d_new_cols, void *stream);

/* ---- tandem-repeat masking --- run_remove_TR / filter_tandem_repeats  Util.py:2855-2874, 4672-4697 (a-2) ---
 * The reference runs `trf <file> 2 7 7 80 10 50 500 -f -d -m -h` and continues with the .mask FASTA.  This build's own stage
 * (definition: oracle/hite_oracle_trf.c; TRF is third-party, parity unpinned): stretches of the resident genome that align
 * with themselves max_period (<= 500) or fewer bases further on with score >= 50 under match 2 / mismatch 7 / indel 7 and
 * at least 1.85 copies become N for every later stage.  mask_bits_host (optional, (n_bases + 31) / 32 words): bit (i & 31) of
 * word (i >> 5) = base i of the concatenated contigs is masked.  masked_bases_out (optional): their number. */
int hite_tr_mask(hite_ctx *ctx, int32_t max_period, uint32_t *mask_bits_host, int64_t *masked_bases_out);

/* ---- column vote --- col_base_map  Util.py:9251-9266 (a-15) --------------------------------
 * counts_out[col_off[i] + c][6] = per-column counts of A,C,G,T,N,'-' over ALL rows of
 * alignment i, with col_off[i] = caller's exclusive scan of cols. */
int hite_column_vote(hite_ctx *ctx, int32_t n, const uint8_t *msa, const int64_t *msa_off, const int32_t *rows,
                     const int32_t *cols, const int64_t *col_off, int32_t *counts_out);

/* ---- boundary search --- search_boundary_homo_v3 / _v4  Util.py:8887-9143 / 8556-8824 --------
 * One search per alignment: pos[i], side[i] (0 'start', 1 'end'), thr[i]; variant 3 or 4.
 * For v4 int_thr/out_thr as the caller passes them; valid_out (v4's first tuple element)
 * may be NULL for v3.  win_in = 20, win_out = 10 in every reference call. */
int hite_boundary_search(hite_ctx *ctx, int32_t n, const uint8_t *msa, const int64_t *msa_off, const int32_t *rows,
                         const int32_t *cols, const int32_t *pos, const int32_t *side, const double *thr,
                         const double *int_thr, const double *out_thr, int32_t variant, int32_t win_in,
                         int32_t win_out, int32_t *boundary_out, int32_t *valid_out);

/* ---- judge --- judge_boundary_v5 / v6 / v9 (result_type 'cons') ------------------------------
 * te_type selects the variant for the whole batch.  cand = candidate sequences (cur_seq), CSR
 * cand_off[n+1].  calls[i].cons_off = msa col prefix: cons pool must hold sum(cols[i] + 8) bytes
 * and candidate i's consensus is written at cons_off = sum_{j<i}(cols[j] + 8). */
int hite_judge(hite_ctx *ctx, int32_t te_type, int32_t plant, int32_t n, const uint8_t *msa, const int64_t *msa_off,
               const int32_t *rows, const int32_t *cols, const uint8_t *cand, const int64_t *cand_off,
               hite_call *calls, uint8_t *cons);
int hite_judge_dev(hite_ctx *ctx, int32_t te_type, int32_t plant, int32_t n, const uint8_t *d_msa,
                   const int64_t *d_msa_off, const int32_t *d_rows, const int32_t *d_cols, const uint8_t *d_cand,
                   const int64_t *d_cand_off, const int64_t *d_col_off, int32_t max_cols, int32_t max_rows,
                   hite_call *d_calls, uint8_t *d_cons, void *stream);

/* ---- TSDsearch_v5  Util.py:2460-2492 (batch of rows) --------------------------------------- */
int hite_tsd_search(hite_ctx *ctx, int32_t n, const uint8_t *rows_bytes, const int64_t *row_off,
                    const int32_t *bstart, const int32_t *bend, int32_t plant, int32_t *tsd_len_out,
                    uint8_t *left_out /* n x 16 */, uint8_t *right_out /* n x 16 */);

/* ---- non-LTR candidate preparation --- search_polyA_TSD  Util.py:10915-11007 (get_candidate_non_LTR :11009) -------------
 * batch of flanked repeats (CSR): polyA / tandem tail near the 3' end (or polyT / tandem head), then an 8-20 bp TSD
 * (<= 1 edit) within win5 (<= 25) of the 5' end.  out: 6 x int64 per sequence = {found_TSD, direct (0 none, 1 '+', 2 '-'),
 * TSD start, TSD length, lo, hi}: non_ltr_seq = seq[lo:hi], reverse-complemented by the caller when direct == 2. */
int hite_nonltr_prep(hite_ctx *ctx, int32_t n, const uint8_t *seqs, const int64_t *seq_off, int32_t flank, int32_t win5,
                     int64_t *out);

/* ---- LTR flank-frame vote (vendored FiLTR) --- judge_left_frame_LTR / judge_right_frame_LTR
 * bin/FiLTR-main/src/Util.py:9327 / :9175 -----------------------------------------------------------------------------
 * n matrices of rows[i] x cols[i] bytes at off[i] (the left OR right frames of the copies of one LTR candidate, what the
 * reference reads from the '.matrix' file, one column of the tab-separated pair), side 0 = left frames (start column
 * flank-1, walk left, tolerance 5), side 1 = right frames (start column 0, walk right, tolerance 20).
 * ok_out[i] = 1 / 0 (is the candidate kept), boundary_out[i] = new boundary column or -1.  cols[i] <= 1024, flank <= cols[i]. */
int hite_ltr_frame(hite_ctx *ctx, int32_t n, const uint8_t *frames, const int64_t *off, const int32_t *rows,
                   const int32_t *cols, int32_t flank, int32_t window, int32_t side, int32_t *ok_out, int32_t *boundary_out);

/* ---- FMEA --- get_longest_repeats_v4 + process_all_seqs  Util.py:4122-4400, 4529-4569 -------------
 * n HSPs in blast6 file order (cols 0,1,6,7,8,9 of -outfmt 6): qseg/sseg = ids of the 'chr$offset'
 * segment names, 1-based inclusive coordinates (reverse hits have ss > se); seg_chrom/seg_off give the
 * chromosome id and the offset of each segment (nseg <= 4096).  skip_gap = fixed_extend_base_threshold.
 * Output = the keys 'chr:start-end' of the reference's longest_repeats dict, in insertion order, as
 * (chrom id, start, end); *n_out is set even when HITE_ECAP is returned.
 * HITE_EINVAL for a zero-length HSP (the reference raises ZeroDivisionError, :4270) or coordinates
 * outside [0, 2^31) / chain spans >= 1.31 Mbp (the de-duplication key is packed into 64 bits). */
int hite_fmea_chain(hite_ctx *ctx, int64_t n, const int32_t *qseg, const int32_t *sseg, const int64_t *qs,
                    const int64_t *qe, const int64_t *ss, const int64_t *se, int32_t nseg, const int32_t *seg_chrom,
                    const int64_t *seg_off, int64_t skip_gap, int64_t max_len, int64_t cap, int32_t *out_chrom,
                    int64_t *out_start, int64_t *out_end, int64_t *n_out);
/* same, HSP arrays resident on the device (e.g. straight from hite_seed_allvsall_dev: no PCIe round trip of the table) */
int hite_fmea_chain_dev(hite_ctx *ctx, int64_t n, const int32_t *d_qseg, const int32_t *d_sseg, const int64_t *d_qs,
                        const int64_t *d_qe, const int64_t *d_ss, const int64_t *d_se, int32_t nseg, const int32_t *seg_chrom,
                        const int64_t *seg_off, int64_t skip_gap, int64_t max_len, int64_t cap, int32_t *out_chrom,
                        int64_t *out_start, int64_t *out_end, int64_t *n_out);

/* ---- copy clustering of a blast6 HSP table --- get_query_copies  Util.py:6828-7030 (+ get_copies_v1 :7032-7060) -----
 * n HSPs in file order (host arrays): query id in [0, nq), subject id in [0, ns), 1-based inclusive coordinates
 * (s_start > s_end = minus strand), identity column (may be NULL: only its equality between otherwise identical
 * lines matters).  Per query: cluster per (subject in order of first appearance, strand), longest chain per cluster
 * with the 200 bp gap rules (qthr / sthr), longest first, keep chain_len / qlen >= qcov (and, if scov > 0,
 * subject_span / slen[sid] >= scov), de-duplicate on (subject, start, end), stop after max_copy + 1 (<= 254).
 * Output CSR copy_first[nq + 1] into (o_sid, o_s <= o_e, o_len, o_minus); *n_out = total; HITE_ECAP if total > cap.
 * HITE_EINVAL on ids / coordinates out of range. */
int hite_query_copies(hite_ctx *ctx, int64_t n, const int32_t *qid, const int32_t *sid, const int64_t *qs, const int64_t *qe,
                      const int64_t *ss, const int64_t *se, const double *ident, int32_t nq, const int64_t *qlen, int32_t ns,
                      const int64_t *slen, double qcov, double scov, int64_t qthr, int64_t sthr, int32_t max_copy, int64_t cap,
                      int64_t *copy_first, int32_t *o_sid, int64_t *o_s, int64_t *o_e, int64_t *o_len, uint8_t *o_minus,
                      int64_t *n_out);

/* ---- every chain of every cluster --- the chaining core of FMEA (Util.py:10452-10645) and of
 * get_full_length_copies_from_blastn_v1 (:5907-6105; with generate_full_length_out_v1 :6288 what mask_genome_intactTE :6389
 * consumes), i.e. get_longest_repeats_v4's core without its de-duplication.  n HSPs in file order (host arrays; the caller
 * drops the lines its function skips), query id in [0, nq), subject id in [0, ns), 1-based inclusive coordinates (s_start >
 * s_end = minus strand).  qgap[q] = the query's skip_gap: an HSP joins a cluster / extends a chain while the distance is
 * < qgap[q] (FMEA: fixed_extend_base_threshold for every query; full-length copies: ceil(len(query) * threshold) -- an
 * integer distance is below a real gap exactly when it is below its ceiling).  Output CSR chain_first[nq + 1] over the chains
 * of each query in the reference's order (subjects by first appearance, forward clusters before reverse ones, clusters in
 * sweep order, chains by their first fragment): subject id, (prev_query_start, prev_query_end, prev_subject_start,
 * prev_subject_end) as the reference holds them (1-based, s_start > s_end on the minus strand), cur_extend_num.
 * *n_out = total; HITE_ECAP if total > cap; HITE_EINVAL on ids / coordinates out of range. */
int hite_chain_all(hite_ctx *ctx, int64_t n, const int32_t *qid, const int32_t *sid, const int64_t *qs, const int64_t *qe,
                   const int64_t *ss, const int64_t *se, int32_t nq, int32_t ns, const int64_t *qgap, int64_t cap,
                   int64_t *chain_first, int32_t *o_sid, int64_t *o_qs, int64_t *o_qe, int64_t *o_ss, int64_t *o_se,
                   int32_t *o_next, int64_t *n_out);

/* ---- library de-duplication (panHiTE merge) --- the arithmetic between the external tools of deredundant_for_LTR_v5 -----
 * hite_lib_chain: process_blast_results_in_chunks + process_chunk + extend_fragments (Util.py:12146-12200, 11958-12003,
 * 11869-11944).  n blast6 lines of a library-vs-itself search in file order (host arrays), ids into seq_len[nseq],
 * 1-based inclusive coordinates; a line with qid == sid, qs == ss, qe == se is skipped.  chunk_size as in the reference
 * (<= 0: one chunk): a chunk is closed by a kept line whose 1-based number is a multiple of chunk_size, chains never
 * cross chunks.  skip_gap = seq_len[query] * (1 - threshold).  Output records in the order of the reference's chunk
 * files (chunk, query by first appearance, subject by first appearance, forward then reverse, creation order):
 * (o_chunk, o_q, o_qs = q_start - 1, o_qe, o_s, o_ss = s_start - 1, o_se); *n_out records, HITE_ECAP if > cap. */
int hite_lib_chain(hite_ctx *ctx, int64_t n, const int32_t *qid, const int32_t *sid, const int64_t *qs, const int64_t *qe,
                   const int64_t *ss, const int64_t *se, int32_t nseq, const int64_t *seq_len, double threshold, int64_t chunk_size,
                   int64_t cap, int32_t *o_chunk, int32_t *o_q, int64_t *o_qs, int64_t *o_qe, int32_t *o_s, int64_t *o_ss,
                   int64_t *o_se, int64_t *n_out);
/* hite_lib_cluster: cluster_sequences_from_chunks (Util.py:12067-12115) on the records above (host code: the greedy
 * pass is sequential by definition).  Cluster c = members[cl_first[c] .. cl_first[c+1]): its query, then the subjects in
 * the order they joined (the reference keeps a Python set: membership is the contract).  *n_cl clusters. */
int hite_lib_cluster(int64_t nrec, const int32_t *chunk, const int32_t *q, const int64_t *qs, const int64_t *qe, const int32_t *s,
                     const int64_t *ss, const int64_t *se, int32_t nseq, const int64_t *seq_len, double threshold, int64_t cap_cl,
                     int64_t cap_mem, int64_t *cl_first, int32_t *members, int64_t *n_cl);
/* hite_msa_consensus: cons_from_mafft_v1 (Util.py:12515-12566) for a batch of alignments.  Alignment a = rows[a] x cols[a]
 * bytes, row-major, at mats + mat_off[a] (mat_off[nmat] = total); a column contributes its most frequent non-gap byte if
 * that count > rows[a] / 2.  Consensus a is written at cons + out_off[a] (reserve cols[a] bytes), length cons_len[a]. */
int hite_msa_consensus(hite_ctx *ctx, int32_t nmat, const int32_t *rows, const int64_t *cols, const int64_t *mat_off,
                       const uint8_t *mats, const int64_t *out_off, uint8_t *cons, int64_t *cons_len);
/* hite_msa_subcluster: sub-clusters of an alignment, the step between the two alignments of generate_cons_v1 (Util.py:12467-12476,
 * where the reference runs `Ninja --corr_type m --cluster_cutoff 0.2`).  The tool is not pinned: what is computed is the leader
 * clustering below (util.ninja_stand_in; twin tests/subcluster_twin.py), not Ninja's neighbour-joining tree.
 *  - An alignment is R rows x C columns of bytes.  A gap is byte 45 and nothing else; bytes compare as bytes ('a' != 'A').
 *  - For two rows x, y: n = columns where x or y is not a gap; diff = columns where x != y (a column where both are gaps has x == y).
 *    x matches y when n > 0 and (double)diff <= cutoff * (double)n, evaluated in binary64 as written.
 *  - Rows are visited in order: row r joins the FIRST leader, in leader order, that it matches; if it matches none it becomes the
 *    next leader.  Membership is never transitive: a row that matches only a non-leader member founds its own sub-cluster.
 *  - Output per row: the index of its sub-cluster, counted in order of the leaders' appearance.
 * Batch layout as hite_msa_consensus: alignment a = rows[a] x cols[a] bytes, row-major, at mats + mat_off[a]; mat_off and row_off
 * have nmat + 1 ascending entries (mat_off[a+1] - mat_off[a] >= rows[a] * cols[a], row_off[a+1] - row_off[a] >= rows[a]); the
 * alignments may start at any byte offset; mats is readable 16 bytes past its end.  sub_of_row + row_off[a] receives rows[a]
 * indices, n_sub[a] the number of sub-clusters.  nmat = 0 is valid; rows[a] = 0 gives n_sub[a] = 0; with cols[a] = 0 every row is
 * its own sub-cluster (n = 0).  HITE_EINVAL for a negative count, a missing buffer, descending offsets, cols[a] > 65 535 and a
 * cutoff that is NaN or outside [0, 1].  The alignments go to the device in batches of bounded bytes (one alignment larger than a
 * batch runs alone); the work is on the context's stream and scratch.
 * Rows are taken in chunks of HITE_SUBCLUSTER_CHUNK (hite_subcluster.hip); $HITE_SUBCLUSTER_CHUNK_ROWS = 1 .. HITE_SUBCLUSTER_CHUNK,
 * read by hite_ctx_create, sets a smaller chunk (a test knob: small inputs then take the chunked path; never changes a result), as
 * $HITE_SUBCLUSTER_BATCH_BYTES sets the bytes of a batch (default 256 MiB). */
#define HITE_SUBCLUSTER_CHUNK 64
int hite_msa_subcluster(hite_ctx *ctx, int32_t nmat, const int32_t *rows, const int64_t *cols, const int64_t *mat_off,
                        const uint8_t *mats, double cutoff, const int64_t *row_off, int32_t *sub_of_row, int32_t *n_sub);

/* ---- clusters of a group of frames --- the three `cd-hit-est` calls of FiLTR's step 3 (bin/FiLTR-main/utils/data_util.py:2872-2920
 * sort_frame, `-aS 0.3 -c 0.8 -G 0 -g 1 -A 20` on the left and on the right frames of a candidate's copies;
 * bin/FiLTR-main/src/Util.py:10938-10983 filter_ltr_by_flanking_cluster_sub, `-aS 0.95 -aL 0.95 -c 0.95 -G 0 -g 1 -A 50` on the
 * joined frames).  The tool is not pinned: what is computed is the definition below (twin tests/framecluster_twin.py), not the
 * tool's word filter, banded affine alignment or `-g 1` choice of the best cluster.
 *  - Bytes: letters count in either case; anything outside ACGT is N, and N matches nothing, not even N.  Callers strip '-' first.
 *  - Pair value R(A, B): a value is a tuple (score, matches, columns, bases of A, bases of B), compared lexicographically;
 *    E = (0, 0, 0, 0, 0).  V(i, 0) = V(0, j) = E.  For i, j >= 1, V(i, j) is the largest of
 *        V(i-1, j-1) + (+2, 1, 1, 1, 1) when A[i] = B[j] and both are in ACGT, else V(i-1, j-1) + (-2, 0, 1, 1, 1);
 *        V(i-1, j)   + (-3, 0, 1, 1, 0);
 *        V(i, j-1)   + (-3, 0, 1, 0, 1);
 *    replaced by E when its score is <= 0.  R(A, B) is the largest V over all cells (E when a sequence is empty).  It is this
 *    recurrence, not a claim of optimality over alignment paths.  With both_strands, R is the larger of R(A, B) and
 *    R(A, revcomp(B)).  (The fields fit 10 + 9 + 10 + 9 + 9 bits: one 64-bit integer maximum is the whole rule.)
 *  - Similar(A, B), A the earlier row in cluster order and B the later, R = (s, k, c, a, b): c > 0, and
 *    (double)k >= ident * (double)c, and a >= min_cov and b >= min_cov, and (double)a >= cov_long * (double)|A|, and
 *    (double)b >= cov_short * (double)|B|; every compare in binary64 exactly as written.
 *  - A group: rows with length <= min_len are dropped (cluster_of_row = -1; they count nowhere; cd-hit's `-l`, callers pass 10).
 *    The others are taken by length descending, ties by ascending row index.  A row joins the FIRST representative, in order of
 *    creation, that it is similar to; otherwise it becomes the next representative.  cluster_of_row = the cluster's creation
 *    index, n_cluster[g] = the number of clusters.
 * Layout: the rows of group g are row_off[g] .. row_off[g+1] (n_group + 1 ascending entries, row_off[0] >= 0); row r is the bytes
 * seqs + seq_off[r] .. seq_off[r+1] (ascending; any byte offset).  A group of more than HITE_FRAMECLUSTER_MAX_ROWS rows, or holding
 * a row longer than HITE_FRAMECLUSTER_MAX_LEN, gets n_cluster[g] = -1 and -1 on all its rows; the other groups are unaffected.
 * n_group = 0, empty groups and empty rows are valid.  HITE_EINVAL for a negative count (n_group, min_cov, min_len), a missing
 * buffer, descending offsets and a threshold (ident, cov_short, cov_long) that is NaN or outside [0, 1]; the context stays usable.
 * The groups go to the device in batches of bounded sequence bytes ($HITE_FRAMECLUSTER_BATCH_BYTES, read by hite_ctx_create, sets a
 * smaller batch: a test knob that never changes a result; default 64 MiB); the work is on the context's stream and scratch. */
#define HITE_FRAMECLUSTER_MAX_ROWS 128
#define HITE_FRAMECLUSTER_MAX_LEN  256
int hite_frame_cluster(hite_ctx *ctx, int64_t n_group, const int64_t *row_off /* n_group + 1 */,
                       const uint8_t *seqs, const int64_t *seq_off /* rows + 1 */,
                       double ident, double cov_short, double cov_long, int32_t min_cov, int32_t min_len,
                       int32_t both_strands, int32_t *cluster_of_row, int32_t *n_cluster);

/* ---- LTR frames of the vendored FiLTR --- get_both_ends_frame  bin/FiLTR-main/src/Util.py:1401-1497 (+ :1341-1399) -----
 * Batch of alignments (rows[a] x cols[a] bytes at msa + msa_off[a], upper case) with the terminal sequence of each
 * (cand + cand_off[a] .. cand_off[a+1]).  Per alignment: anchors from the first row carrying both 20-mers within two
 * edits, FiLTR's sparse-column rule (more than R/2 gaps, anchor columns always kept), then per row the `.matrix` line
 * (left frame | right frame, 2 * flank bytes at frames + frame_off[a] + r * 2 * flank, '-' padded) and the full-length row
 * (left frame + cleaned[new_start:new_end] + right frame at full + full_off[a] + r * (2 * flank + cols[a]), full_cols[a]
 * bytes used).  new_pos[2a], new_pos[2a+1] = anchor columns in cleaned coordinates.  status[a]: 0 ok, 1 boundary not
 * found (the reference returns None, None), 2 both anchors on the same column (not restated). */
int hite_ltr_both_ends(hite_ctx *ctx, int32_t n, const uint8_t *msa, const int64_t *msa_off, const int32_t *rows, const int32_t *cols,
                       const uint8_t *cand, const int64_t *cand_off, int32_t flank, uint8_t *frames, const int64_t *frame_off,
                       uint8_t *full, const int64_t *full_off, int32_t *full_cols, int32_t *new_pos, int32_t *status);

/* ---- high-copy LTR vote of the vendored FiLTR's hybrid CNN --- bin/FiLTR-main/src/Deep_Learning/hybridLTR_feature_extractor.py,
 * hybridLTR_model.py (class CNNCAT), hybridLTR_predicter.py; run by LTR_filter.py:146-170 on every matrix of more than 5 rows.
 * PINNED to the reference: the features are integers and equal the reference's, the logits are fp32 and are held to the
 * reference's within the bound recorded in tests/golden/ltr_deep.json.gz (twin tests/ltrdeep_twin.py).
 * Input per candidate: row_off[c+1] - row_off[c] rows of HITE_LTRDEEP_COLS bytes at rows + row_off[c] * HITE_LTRDEEP_COLS, each the
 * left frame of 100 bytes followed by the right frame of 100 bytes.  A candidate of fewer than 5 or more than HITE_LTRDEEP_ROWS rows
 * is NOT SCORED: status 1, logits (pooled, img, kmer) 0; the others are unaffected.  A scored candidate has status 0.
 *  - Characters: anything other than upper-case A C G T is '-'.  Fewer than 100 rows are padded below with all-'-' rows.
 *  - img [3][100][200] (uint8): `block` 100 on a base, 0 on '-'; `support` on a base (int)(((double)count / (double)total) * 100.0),
 *    count = rows with that base in the column, total = rows with any base in the column (binary64, from a 101 x 101 table the
 *    host builds: it differs from floor(100 count / total) at (29, 50), (29, 100), (57, 100), (58, 100)), 0 on '-'; `base` G 100,
 *    C 75, A 50, T 25, '-' 0.
 *  - kmer [2][HITE_LTRDEEP_KMER] (int32), left half then right half: for k = 3, 4, 5 the count of every word of k consecutive columns
 *    of every row of the half (100 - k + 1 words per row), the word read as a base-5 number over A 0, G 1, C 2, T 3, '-' 4, first
 *    column most significant; the all-'-' word (the last number) has no slot: 124 + 624 + 3124 slots, the three k one after another.
 *  - Both are L2-normalised over the channel axis (the 3 planes of a pixel, the 2 halves of a slot), x / max(|x|_2, 1e-12) in
 *    binary64 rounded to fp32.
 *  - Model (eval mode): two branches (img with 3 input planes on 100 x 200, kmer with 2 on 1 x 3872) of three residual blocks
 *    in -> 8 -> 16 -> 32; a block is conv 3x3 (pad 1, no bias) -> BN -> ReLU -> conv 3x3 -> BN, plus BN(conv 1x1 of the block's
 *    input), -> ReLU; the mean over H x W of each of the 32 + 32 planes is `pooled`; then Linear 64 -> 16, BN, ReLU, Linear 16 -> 8,
 *    BN, ReLU, Linear 8 -> 2: the logits.  All in fp32 FMAs in a fixed order -- a convolution sums over (input plane, ky, kx)
 *    ascending, a mean sums the pixels of a tile in a fixed tree and the tiles in ascending order -- so a candidate's result is the
 *    same bits at every batch size and at every place of a batch.
 * params: HITE_LTRDEEP_PARAMS floats, every tensor in PyTorch's element order: the img branch, then the kmer branch, each block
 * after block as conv1.weight [out][in][3][3], bn1 (weight, bias, running_mean, running_var), conv2.weight, bn2, shortcut
 * conv.weight [out][in][1][1], shortcut bn; then Linear1 (weight [16][64], bias), its bn, Linear2 ([8][16], bias), its bn, Linear3
 * ([2][8], bias).  hite_ltr_model_build folds every batch norm (eps 1e-5) into a scale and a shift in binary64, rounds to fp32 and
 * uploads; the handle goes to hite_ltr_model_release before the context is destroyed.  n_params != HITE_LTRDEEP_PARAMS or a
 * parameter that is not finite: HITE_EINVAL.
 * hite_ltr_deep_features runs the feature kernel of hite_ltr_deep alone (tests, diagnosis).  n = 0 is valid; HITE_EINVAL for a
 * negative count, a missing buffer and descending offsets.  The candidates go to the device in batches of HITE_LTRDEEP_BATCH_DEFAULT
 * ($HITE_LTRDEEP_BATCH, read by hite_ctx_create, sets another size: a test knob that never changes a result); a candidate of a batch
 * holds about 5.8 MB of the context's scratch (features 0.11 MB, fp32 planes 59 x 80 000 + 58 x 15 488 bytes, partial sums).
 * The convolution kernels take tiles of HITE_LTRDEEP_TILE_H x HITE_LTRDEEP_TILE_W pixels of the image and of HITE_LTRDEEP_KMER_TILE
 * slots of the k-mer axis. */
#define HITE_LTRDEEP_PARAMS   40026
#define HITE_LTRDEEP_ROWS     100
#define HITE_LTRDEEP_COLS     200
#define HITE_LTRDEEP_KMER     3872
#define HITE_LTRDEEP_TILE_H   8
#define HITE_LTRDEEP_TILE_W   32
#define HITE_LTRDEEP_KMER_TILE 256
#define HITE_LTRDEEP_BATCH_DEFAULT 64
int hite_ltr_model_build(hite_ctx *ctx, const float *params, int64_t n_params, void **model_out);
void hite_ltr_model_release(void *model);
int hite_ltr_deep(hite_ctx *ctx, void *model, int64_t n, const uint8_t *rows /* 200 bytes per row */,
                  const int64_t *row_off /* n + 1, in rows */, float *logits /* n x 2 */, float *pooled /* n x 64, may be NULL */,
                  int8_t *status /* 0 scored, 1 not scored */);
int hite_ltr_deep_features(hite_ctx *ctx, int64_t n, const uint8_t *rows, const int64_t *row_off,
                           uint8_t *img /* n x 3 x 100 x 200 */, int32_t *kmer /* n x 2 x 3872 */, int8_t *status);

/* ---- k-mer TSD seed matching --- search_confident_tir_v4  Util.py:7734-7845 -------------------------
 * batch of flanked candidates (CSR); the raw boundaries are (flank+1, len-flank), 1-based, as
 * search_confident_tir_batch_v1 passes them (Util.py:6550), tsd_search_distance = flank (<= 63).
 * Per candidate up to 100 records (tsd_len, tir_start, tir_end, distance), 0-based inclusive, in the
 * canonical order (distance, tir_start, tir_end, tsd_len) that replaces the reference's
 * PYTHONHASHSEED-dependent tie order; rec_out is n x 100 x 4 int32, cnt_out[n] (-1: window too long).
 * Any byte is a letter of its own, as in the reference's string compare: a k-mer with R never pairs with
 * the same k-mer with Y or N (the sequences are not folded; the "NN" filter is literal). */
int hite_tsd_kmer(hite_ctx *ctx, int32_t n, const uint8_t *seqs, const int64_t *seq_off, int32_t flank, int32_t plant,
                  int32_t *rec_out, int32_t *cnt_out);
int hite_tsd_kmer_dev(hite_ctx *ctx, int32_t n, const uint8_t *d_seqs, const int64_t *d_seq_off, int32_t flank,
                      int32_t plant, int32_t *d_rec_out, int32_t *d_cnt_out, void *stream);

/* ---- terminal inverted repeats --- run_itrsearch  Util.py:216-224 (third-party ELF tools/itrsearch, `-i 0.7 -l 7`) ----------
 * The filter of search_confident_tir_batch_v1 (Util.py:6556-6587: first 40 + last 40 bases of every k-mer TSD variant; a variant
 * without a terminal inverted repeat is dropped, "Length itr=" feeds filter_dup_itr_v3) and of remove_no_tirs (Util.py:13897-13920:
 * whole low-copy sequences).  In-tree stage; definition oracle/hite_oracle_itr.c, read from the tool's disassembly and pinned to
 * the tool's own output (tests/golden/itr_search.json.gz).  Per sequence (CSR batch; bytes outside ACGT are N, and N scores as a
 * match against anything, as in the tool): seq1 = first h bases, seq2 = reverse complement of the last h, h = min(500, len / 2), or
 * min(len, end_len) when end_len > 0 (the record `s[:end_len] + s[-end_len:]` composed on the device); affine-gap extension
 * alignment from (0,0) with a free end (match / mismatch / gap_open / gap_extend: the tool's defaults are 10 / 16 / 32 / 32 and the
 * reference passes none of them).
 * out[8k ..] = { score, end in seq1, end in seq2, equal bases, aligned columns, found, "Length itr=" (end1 - 1; -1 without an
 * alignment), flags }; found = min_len <= end1 && equal / aligned >= min_identity (binary64), what makes the tool write the record
 * to <input>.itr.  flags bit 3: the sequence needs more than max_h (the _dev caller's promise) and was skipped. */
int hite_itr_search(hite_ctx *ctx, int64_t n, const uint8_t *seqs, const int64_t *seq_off, int32_t end_len, double min_identity,
                    int32_t min_len, int32_t match, int32_t mismatch, int32_t gap_open, int32_t gap_extend, int32_t *out);
/* device-resident, asynchronous on `stream`; max_h = upper bound of h over the batch (sizes LDS / the scratch slots; <= 64 keeps
 * everything in LDS).  d_seqs must be readable up to d_seq_off[n]. */
int hite_itr_search_dev(hite_ctx *ctx, int64_t n, const uint8_t *d_seqs, const int64_t *d_seq_off, int32_t end_len, int32_t max_h,
                        double min_identity, int32_t min_len, int32_t match, int32_t mismatch, int32_t gap_open, int32_t gap_extend,
                        int32_t *d_out, void *stream);
/* the kernel's constants, for the tests at its limits (no GPU is touched): out = { cap on h (500, the tool's own), largest h whose
 * traceback store lives in LDS, sequences in flight per workgroup, grid cap on the LDS path, grid cap on the HBM path, columns of
 * a strip } */
int hite_itr_limits(int32_t out[6]);

/* ---- translated protein search --- get_domain_info  Util.py:4571-4612 (third-party `blastx -evalue 1e-20 -outfmt 6`) -------------
 * The search behind the recall of low-copy candidates by intact protein domains (Util.py:8215-8276; the fragments are chained by
 * multiple_alignment_blastx_v1 :1006-1262).  In-tree stage, not pinned to the tool (no machine of the project has it): the
 * definition below, its CPU twin tests/protein_twin.py + tests/protein_twin.c, HIP == twin record for record.  No SEG masking, no
 * composition-based statistics, no length adjustment of the search space.
 *  1 translation: the query in upper case; frames +1 +2 +3 read it, -1 -2 -3 its reverse complement; standard genetic code, a codon
 *    with a byte outside ACGT is X, a stop '*'; residue t of frame f covers bases f + 3 t .. f + 3 t + 2 (0-based) of that strand, a
 *    trailing partial codon is dropped.  Library letters outside the 20 standard residues (either case) are X.  A protein of more than
 *    65 535 residues or a query of more than 196 605 bases is HITE_EINVAL.
 *  2 scores: '*' against anything -4, else X against anything -1, else BLOSUM62; a gap of g residues costs 11 + g.
 *  3 seeds: four consecutive equal standard residues at frame position i and protein position j; a 4-mer with fewer than three distinct
 *    letters is no seed.
 *  4 ungapped filter: every seed is extended along its diagonal, to the right from its last column and to the left from its first;
 *    a side keeps the first position of its best running sum and stops at either sequence's end or once the sum has dropped MORE
 *    than 16 below that best.  Segment = seed + both extensions; it survives with a score >= 41 (22 bits under lambda 0.3176,
 *    K 0.134).  Survivors with the same (query, frame, protein, diagonal, segment) count once.
 *  5 tasks: per (query, frame, protein) the survivors by (diagonal d = j - i, segment start, segment end); one joins the open cluster
 *    while d <= c + 16, c = the diagonal of the cluster's first survivor.  The cluster by (segment start, segment end) splits where a
 *    segment starts more than 128 residues after the largest segment end so far.  A piece is a task: band c - 24 .. c + 39 (64
 *    diagonals), frame rows max(0, first start - 128) .. min(L_f - 1, largest end + 128).
 *  6 gapped alignment: the best local alignment (Gotoh) over the cells (i, j) of the task's rows and band with 0 <= j < protein
 *    length; other cells do not exist.  E(i,j) (gap in the protein, from (i-1,j)) = max(H - 12, E - 1), F(i,j) (gap in the frame, from
 *    (i,j-1)) likewise, opening preferred on a tie; H = max(H(i-1,j-1) + s, E, F) preferring the diagonal, then E, then F; values
 *    below 1 are 0 = no alignment, and the diagonal move starts a new alignment at (i, j) when H(i-1,j-1) is 0.  The best cell is the
 *    first maximum in row-major order.  Start cell, identical columns (equal standard residues) and columns are those of the path
 *    these preferences choose (propagated forward with the scores; no traceback).
 *  7 E = m n K exp(-lambda S), lambda 0.267, K 0.041 (gapped BLOSUM62 11/1), m = floor(query bases / 3), n = all library residues;
 *    hite_protein_smin turns the requested E-value into the smallest integer S with E <= evalue (binary64, once per query), the
 *    device compares integers.
 *  8 output: per (query, frame, protein) the HSPs by (score descending, frame start, protein start, frame end, protein end); one is
 *    dropped when it shares its start cell or its end cell with a kept one or lies inside a kept one on both sequences.  Query
 *    coordinates are 1-based bases (minus strand: q_start > q_end, as the tool prints them), protein coordinates 1-based residues.
 *    Final order: (query, score descending, protein, frame in the order +1 +2 +3 -1 -2 -3, q_start, s_start).  Nothing depends on
 *    launch geometry or on the order of an atomic append.
 *
 * hite_translate6: step 1 alone (host in, host out): aa_out = the six frames of every query as letters, frame 6 q + f (f = 0..5 for
 * +1 +2 +3 -1 -2 -3) at frame_off[6 q + f] .. frame_off[6 q + f + 1]; frame_off (6 n + 1 entries) is always filled, HITE_ECAP when
 * frame_off[6 n] > cap. */
int hite_translate6(hite_ctx *ctx, int64_t n, const uint8_t *nt, const int64_t *nt_off, int64_t cap, uint8_t *aa_out, int64_t *frame_off);
/* the library: n_prot proteins as letters + CSR.  Builds the 20^4-bucket seed directory (entries in position order).  *state_io
 * (initially NULL; an existing handle is released first) owns the index and the grow-only arena of every search; release it with
 * hite_protein_lib_release before the context is destroyed. */
int hite_protein_lib_build(hite_ctx *ctx, int64_t n_prot, const uint8_t *aa, const int64_t *aa_off, void **state_io);
void hite_protein_lib_release(void *state);
/* steps 1-8 for n_query queries (bytes + CSR).  Parallel output arrays of `cap` entries: query, protein (indices), frame (+-1..3),
 * q_start, q_end, s_start, s_end, raw score, identical columns, columns; *n_out = the number of HSPs; HITE_ECAP when it exceeds cap
 * (the first cap are written, nothing behind them).  stats (may be NULL): seed hits, distinct survivors, tasks.  Bit score and
 * E-value are the caller's arithmetic on the raw score. */
int hite_protein_search(hite_ctx *ctx, void *state, int64_t n_query, const uint8_t *nt, const int64_t *nt_off, double evalue, int64_t cap,
                        int32_t *o_query, int32_t *o_prot, int32_t *o_frame, int32_t *o_qstart, int32_t *o_qend, int32_t *o_sstart,
                        int32_t *o_send, int32_t *o_score, int32_t *o_ident, int32_t *o_cols, int64_t *n_out, int64_t *stats);
/* host code (no GPU needed).  Step 7: *smin for m query residues and n library residues. */
int hite_protein_smin(int64_t m, int64_t n, double evalue, int32_t *smin);
/* step 5 on survivors ordered as step 5 says, each once (frame = index into frame_len[n_frames], the frame lengths in residues)
 * -> tasks (frame, protein, c, first row, last row) in the order of their groups; HITE_ECAP when there are more than cap. */
int hite_protein_tasks(int64_t n, const int32_t *frame, const int32_t *prot, const int32_t *diag, const int32_t *seg_start,
                       const int32_t *seg_end, int64_t n_frames, const int32_t *frame_len, int64_t cap, int32_t *o_frame, int32_t *o_prot,
                       int32_t *o_c, int32_t *o_lo, int32_t *o_hi, int64_t *n_out);
/* the filter of step 8 on the HSPs of one (query, frame, protein) group (0-based inclusive cells): keep[k] = 1 when HSP k stays */
int hite_protein_hsp_filter(int64_t n, const int32_t *score, const int32_t *f_start, const int32_t *p_start, const int32_t *f_end,
                            const int32_t *p_end, uint8_t *keep);

/* ---- pairwise identity --- the `-c` / `-A` of `cd-hit-est -aS 0.95 -aL 0.95 -c <c> -G 0 -g 1 -A 80` (judge_TIR_transposons.py:87,
 * Util.py:12330; third-party) -------------
 * The primitive under the identity test of the build's cd-hit-est stand-in (util.remove_redundant_sequences with identity="gpu").
 * In-tree stage, not pinned to the tool (no machine of the project has it; its own identity is a banded local alignment with scores
 * 2 / -2 / -6 / -1): the definition below, its CPU twin tests/identity_twin.py + tests/identity_twin.c, HIP == twin on
 * (cost, matches) for every pair.
 *
 * Pair p names two intervals, 0-based and half-open, of sequences in one CSR batch of ASCII bytes.
 *  - A = seq[a_id][a_start:a_end].
 *  - B = seq[b_id][b_start:b_end].  It is reverse-complemented when strand[p] != 0.
 *  - Bytes are upper-cased.  Anything outside ACGT is N.
 *  - N matches nothing, not even N.
 *  - m = |A| and n = |B|.  Both may be 0.
 * Cells (i, j), with 0 <= i <= m and 0 <= j <= n, exist only inside the band lo <= j - i <= hi.
 *  - lo = min(0, n - m) - band.
 *  - hi = max(0, n - m) + band.
 *  - band >= 0 is one value per call.
 * A path runs from (0,0) to (m,n) by three kinds of step, all between cells of the band:
 *  - a diagonal step: a match costs 0 and adds one to matches; a mismatch costs 1;
 *  - a step down, cost 1;
 *  - a step right, cost 1.
 * The result of a pair is the lexicographic optimum: the smallest cost, and among the paths of that cost the largest matches.
 * It is a pair of integers.
 *  - It does not depend on any tie order of the implementation.
 *  - The number of alignment columns is cost + matches.
 *  - The identity is matches / (cost + matches).  Only host code forms that ratio.
 * Limits:
 *  - m, n <= 32 767.  This is the aligner's window limit, STAR_MAX_LEN.
 *  - The band width hi - lo + 1 may not exceed HITE_IDENT_MAX_WIDTH = 2048 (32 strips of 64 diagonals; one wavefront keeps a row
 *    of that many cell states in LDS).
 *  - A pair beyond either limit, or with an id or interval outside its sequence, gets cost = -1, matches = 0.  The other pairs of
 *    the call are unaffected.
 *  - n_pair = 0 is a valid call.
 *
 * Caller-owned host buffers; seqs + seq_off[n_seq + 1] is the CSR batch, the pair arrays and the two outputs hold n_pair entries.
 * The pairs are launched in batches, so device memory is the batch of sequences plus a fixed number of pairs.  HITE_EINVAL for a
 * negative count or band, a missing buffer or descending offsets. */
#define HITE_IDENT_MAX_WIDTH 2048
int hite_pair_identity(hite_ctx *ctx, int64_t n_seq, const uint8_t *seqs, const int64_t *seq_off, int64_t n_pair,
                       const int32_t *a_id, const int64_t *a_start, const int64_t *a_end,
                       const int32_t *b_id, const int64_t *b_start, const int64_t *b_end,
                       const uint8_t *strand, int32_t band, int32_t *cost_out, int32_t *match_out);

/* ---- local alignments of pairs of intervals --- the one `blastn -query Q -subject S -outfmt 6` process FiLTR starts per candidate
 * line in its steps 1 and 2 (is_recombination bin/FiLTR-main/src/Util.py:5923, get_ltr_from_line :11149,
 * judge_scn_line_by_flank_seq_v2 :10759).  In-tree stage, NOT blastn and not pinned to it (no machine of the project has the tool):
 * what is computed is the definition below, its CPU twin tests/pairhsp_twin.py + tests/pairhsp_twin.c, HIP == twin record for
 * record.  Stated deviations: the plus strand only; no e-value; alignments live in bands of 192 diagonals; there is no X-drop, so
 * an HSP can bridge what megablast would split.  The arithmetic is megablast's default scoring times two.
 *
 * For a pair (Q, S): m = |Q|, n = |S|; diag_min is one integer per call (INT32_MIN: none).  Bytes are read as A C G T in either
 * case; anything else matches nothing and is in no word.
 *  1. Limits.  m or n is 0 or above HITE_PAIRHSP_MAX_LEN, or an id or interval outside its sequence: status -1, no HSPs; the
 *     other pairs of the call are unaffected.
 *  2. Word hits.  A hit is (i, j), 0-based, with Q[i, i+12) = S[j, j+12), all twelve bases in ACGT, and j - i >= diag_min.  A word
 *     that occurs more than HITE_PAIRHSP_MAX_OCC times in Q casts no hit.  The diagonal index is k = j - i + m - 1, and vote[b] is
 *     the number of hits with k >> HITE_PAIRHSP_BIN_SHIFT = b.
 *  3. Windows.  w(b) = vote[b] + vote[b+1].  Up to HITE_PAIRHSP_MAX_WINDOWS times the b with the largest w(b) >=
 *     HITE_PAIRHSP_MIN_VOTES is taken, the lowest b on ties, skipping every b with |b - b'| < 2 for a b' already taken.  The band of
 *     a taken b is the diagonals 64 b - HITE_PAIRHSP_BAND_BELOW <= k < 64 b + HITE_PAIRHSP_BAND_ABOVE, further cut by
 *     j - i >= diag_min.
 *  4. Banded local alignment, within a band and a rectangle of rows r0 .. r1 of Q and columns c0 .. c1 of S (1-based).  A cell value
 *     is the tuple (score, matches, columns, q_start, s_start); V(i, j) is the best of
 *        V(i-1, j-1) + (+2, 1, 1) when Q[i] = S[j] and both are in ACGT, else V(i-1, j-1) + (-4, 0, 1);
 *        V(i-1, j)   + (-5, 0, 1);
 *        V(i, j-1)   + (-5, 0, 1).
 *     A neighbour outside the band or the rectangle is the empty value; a path that leaves the empty value at (i, j) has
 *     q_start = i, s_start = j; a value whose score is <= 0 is the empty value.  "Best" is lexicographic: larger score, then larger
 *     matches, then larger columns, then smaller q_start, then smaller s_start.  The result is the best cell of the rectangle, on
 *     equal values the one with the smallest i, then the smallest j; q_end = i, s_end = j.  It is an HSP only at score >=
 *     HITE_PAIRHSP_MIN_SCORE.  It is this recurrence, not a claim of optimality over alignment paths.
 *  5. HSPs per band.  The first is the result on [1, m] x [1, n].  If there is one, one more is taken from the rectangle before it
 *     (rows < q_start, columns < s_start) and one from the rectangle after it (rows > q_end, columns > s_end); a rectangle with
 *     fewer than HITE_PAIRHSP_MIN_RECT rows or columns is skipped.  No further recursion: at most 3 per band,
 *     HITE_PAIRHSP_MAX_HSPS per pair.
 *  6. Order and duplicates.  The HSPs of a pair are ordered by (score descending, q_start, s_start, q_end, s_end); equal keys stay
 *     in the order they were found (windows in the order taken; first, before, after).  An HSP is dropped when an earlier kept one
 *     contains both of its intervals.
 *  7. Record.  Seven int32: q_start, q_end, s_start, s_end (1-based, inclusive, relative to the intervals, as blast6 columns 7-10),
 *     score, matches, columns.
 *
 * Caller-owned host buffers; seqs + seq_off[n_seq + 1] is the CSR batch; the pair arrays hold n_pair entries, intervals 0-based and
 * half-open.  status[p] is the number of records of pair p or -1; its records are recs[7 * first[p]] .. recs[7 * first[p+1]]
 * (first holds n_pair + 1 entries).  *n_out is the number of records of the call: HITE_ECAP when cap is smaller, with status, first
 * and *n_out still filled and the first cap records written.  n_pair = 0 is a valid call and returns 0.  HITE_EINVAL for a negative
 * count, a missing buffer or descending offsets.  The pairs go to the device in batches of bounded size
 * ($HITE_PAIRHSP_BATCH_PAIRS, read by hite_ctx_create, sets a smaller batch: a test knob that never changes a result; default
 * 8 192 pairs and 64 MiB of interval bytes); the work is on the context's stream and scratch. */
#define HITE_PAIRHSP_MAX_LEN     32768
#define HITE_PAIRHSP_WORD        12
#define HITE_PAIRHSP_MAX_OCC     8
#define HITE_PAIRHSP_BIN_SHIFT   6
#define HITE_PAIRHSP_MIN_VOTES   8
#define HITE_PAIRHSP_MAX_WINDOWS 4
#define HITE_PAIRHSP_BAND_BELOW  32
#define HITE_PAIRHSP_BAND_ABOVE  160
#define HITE_PAIRHSP_MATCH       2
#define HITE_PAIRHSP_MISMATCH    (-4)
#define HITE_PAIRHSP_GAP         (-5)
#define HITE_PAIRHSP_MIN_SCORE   56
#define HITE_PAIRHSP_MIN_RECT    28
#define HITE_PAIRHSP_MAX_HSPS    12
int hite_pair_hsps(hite_ctx *ctx, int64_t n_seq, const uint8_t *seqs, const int64_t *seq_off, int64_t n_pair,
                   const int32_t *a_id, const int64_t *a_start, const int64_t *a_end,
                   const int32_t *b_id, const int64_t *b_start, const int64_t *b_end,
                   int32_t diag_min, int64_t cap, int32_t *status /* n_pair: count or -1 */, int64_t *first /* n_pair + 1 */,
                   int32_t *recs /* cap x 7 */, int64_t *n_out);

/* ---- LTR candidate scan --- the `.scn` candidate table FiLTR gets from the vendored LtrDetector (main.py:135-156 through
 * Reproduction/run_LtrDetector_parallel.py and convert_LtrDetector_scn) and HiTE's other branch from `gt ltrharvest` and LTR_FINDER
 * (Util.py:569-667).  In-tree stage, genome in, candidate pairs of direct repeats out.  PARITY UNPINNED against LtrDetector /
 * LTR_harvest / LTR_FINDER (no machine of the project has any of them, and none of their text is here): what is computed is the
 * definition below, its CPU twin tests/ltrscan_twin.py + tests/ltrscan_twin.c, HIP == twin record for record and counter for
 * counter; the stage is measured on planted truth (profiles/r13_ltr_scan.txt).  Stated deviations: a position links to its nearest
 * admissible copy only; words of 13 bases; alignments live in a band of 192 diagonals; no TSD, TG..CA motif or PPT test.
 *
 * The input is a CSR batch of byte sequences.  Bytes are read as A C G T in either case; any other byte is in no word and matches
 * nothing.  Positions are 0-based inside their sequence; len is the length of the sequence at hand.
 *  1. Words.  Position i has a word when s[i, i+13) is all ACGT (HITE_LTRSCAN_WORD).
 *  2. Links.  dmin = min_ltr, dmax = max_len - min_ltr.  For a position i with a word, the next HITE_LTRSCAN_MAX_OCC later
 *     occurrences of the same word in the same sequence are looked at by ascending position; the first j with j - i >= dmin is
 *     taken, and (seq, i, d = j - i) is a hit iff d <= dmax.  A position gives at most one hit.
 *  3. Runs, on two lattices lambda = 0 and 32.  The bin of a hit is (d + lambda) >> 6.  With the hits ordered by (seq, bin, i), a
 *     run is a maximal chain of consecutive hits with equal (seq, bin) and i - i_prev <= HITE_LTRSCAN_GAP; it counts from
 *     HITE_LTRSCAN_MIN_HITS hits on and is (seq, i_lo, i_hi, d_lo, d_hi) (first and last i, smallest and largest d).  A run with
 *     i_hi - i_lo + 13 > max_ltr is dropped.  The runs of both lattices go on (step 6 removes what they find twice).
 *  4. Extension, per run.  dc = (d_lo + d_hi) >> 1.  The pads PL and PR each walk through the four values min(256, max_ltr),
 *     min(1024, max_ltr), min(4096, max_ltr), max_ltr, starting at the first.
 *        Q = [max(0, i_lo - PL), min(len, i_hi + 13 + PR)),  S = [max(0, Q.begin + dc - 96), min(len, Q.end + dc + 96)).
 *     The alignment is step 4 of hite_pair_hsps as it stands (the same cell tuple, 2 / -4 / -5, the same "best", the same best-cell
 *     tie rule) with Q as rows and S as columns, on the whole rectangle Q x S inside the band dc - 96 <= y - x <= dc + 95 (x, y:
 *     positions in the sequence); its result is an HSP at score >= HITE_PAIRHSP_MIN_SCORE, [ls, le) in Q and [rs, re) in S.  No
 *     HSP: the run gives nothing.  If ls - Q.begin < HITE_LTRSCAN_EDGE while Q.begin > 0 and PL is not at its fourth value, PL
 *     steps to its next value; if Q.end - le < HITE_LTRSCAN_EDGE while Q.end < len and PR is not at its fourth value, PR steps.
 *     If either stepped and fewer than HITE_LTRSCAN_MAX_REDO alignments have been redone, the alignment is redone.
 *  5. Filters, integers only, in this order; a record is counted at the first it fails:
 *        min_ltr <= le - ls <= max_ltr and min_ltr <= re - rs <= max_ltr;   min_len <= re - ls <= max_len;   le <= rs;
 *        100 * matches >= identity * columns.
 *  6. Order and duplicates.  Records are ordered by (seq, ls, re, le, rs, -score, -matches, columns); the first of every
 *     (seq, ls, le, rs, re) is kept.
 *  Record: eight int32 -- seq, ls, le, rs, re (0-based, half-open, plus strand: direct repeats need no minus-strand pass), score,
 *  matches, columns.  The caller passes the limits; LtrDetector's defaults are 400 / 22 000 / 100 / 6 000 / 85.
 *
 * Limits: 1 <= min_ltr <= max_ltr <= HITE_LTRSCAN_MAX_LTR (a window then stays under the 32 768 the packed start coordinates of a
 * cell hold), min_len <= max_len, identity in 1 .. 100, every sequence shorter than 2^31: anything else, a negative count, a missing
 * buffer or descending offsets is HITE_EINVAL.  n = 0, empty sequences and sequences shorter than a word are valid and give nothing.
 * recs holds cap records; *n_out is the number of records of the call, HITE_ECAP when cap is smaller (the first cap are written).
 * stats (may be NULL) receives HITE_LTRSCAN_STATS counters: positions with a word, hits, runs that count (both lattices), of these
 * dropped for their span, alignments run, of these redone, runs without an HSP, records dropped by each of the four filters of
 * step 5, records.
 * Whole sequences go to the device in batches of bounded bytes; a sequence is never split (one longer than the bound is a batch of
 * its own).  Device memory of a batch: 33 bytes per base (the bases, 8 + 4 for the word keys and positions, as much again for the
 * sort, 8 for the hits), 34 bytes per hit while the runs are formed (a position gives at most one hit) and 40 per run that is
 * aligned; the default bound of 64 MiB of bases is 2.1 GiB (4.4 GiB if every position had a hit), which fits beside a resident
 * genome.  $HITE_LTRSCAN_BATCH_BYTES, read by hite_ctx_create,
 * sets another bound: a test knob that never changes a result. */
#define HITE_LTRSCAN_WORD       13
#define HITE_LTRSCAN_MAX_OCC    16
#define HITE_LTRSCAN_BIN_SHIFT  6
#define HITE_LTRSCAN_LATTICE    32
#define HITE_LTRSCAN_GAP        100
#define HITE_LTRSCAN_MIN_HITS   4
#define HITE_LTRSCAN_BAND_BELOW 96
#define HITE_LTRSCAN_BAND_ABOVE 96
#define HITE_LTRSCAN_PAD_0      256
#define HITE_LTRSCAN_PAD_1      1024
#define HITE_LTRSCAN_PAD_2      4096
#define HITE_LTRSCAN_EDGE       32
#define HITE_LTRSCAN_MAX_REDO   3
#define HITE_LTRSCAN_MAX_LTR    8192
#define HITE_LTRSCAN_STATS      12
int hite_ltr_scan(hite_ctx *ctx, int64_t n, const uint8_t *seqs, const int64_t *seq_off,
                  int32_t min_len, int32_t max_len, int32_t min_ltr, int32_t max_ltr, int32_t identity /* percent */,
                  int64_t cap, int32_t *recs /* cap x 8 */, int64_t *n_out, int64_t *stats);

/* ---- genome annotation --- the `RepeatMasker -e ncbi -gff -lib <lib> -cutoff 225 <genome>` run that ends HiTE
 * (module/annotate_genome.py:17, module/pan_annotate_genome.py:27) and gives HiTE.out / HiTE.gff / HiTE.tbl and panHiTE's
 * <genome>.full_length.gff.  In-tree stage, library + genome in, annotation records out.  PARITY UNPINNED against RepeatMasker (no
 * machine of the project has it, and none of its text is here): what is computed is the definition below, its CPU twin
 * tests/annotate_twin.py + tests/annotate_twin.c, HIP == twin record for record and counter for counter; the stage is measured on
 * planted truth (tools/annotate_bench.py).  Stated deviations: exact 13-base seeds; alignments live in a band of 192 diagonals; no
 * scoring matrix by divergence and no e-value (the 2 / -4 / -5 arithmetic of hite_pair_hsps at a fixed score threshold instead of
 * -cutoff 225); a copy longer than a window comes as several records; no simple-repeat or low-complexity annotation; no `.cat.gz`.
 *
 * The genome and the library are CSR batches of byte sequences.  Bytes are read as A C G T in either case; any other byte is in no
 * word and matches nothing.  Positions are 0-based; g is a position in its genome sequence (of len bases), q one in a text.
 *  1. Library table.  Entry e (of L bases) gives two texts of L bases: t = 2e is the entry, t = 2e + 1 its reverse complement (a
 *     byte outside ACGT stays outside).  An entry with L > HITE_ANNOT_MAX_LIB_LEN gives no text and has lib_status -1; the others
 *     have 0.  The table holds (word, t, q) for every position q of a text where text[q, q+13) is all ACGT (HITE_ANNOT_WORD).  A
 *     word with more than HITE_ANNOT_MAX_OCC entries in the whole table casts no hit ("silenced": counted per entry).
 *  2. Pieces and hits.  P = piece_len (0: HITE_ANNOT_PIECE).  Piece k of a sequence is [kP, min(len, (k+1)P + HITE_ANNOT_OVERLAP)),
 *     k = 0 .. ceil(len / P) - 1.  piece_len is part of the definition (it decides which hits chain); the number of pieces that go
 *     to the device together is not.  Inside a piece, a position g with piece.begin <= g and g + 13 <= piece.end whose word is a
 *     table word that is not silenced gives one hit (t, q, g) per table entry, with d = g - q.
 *  3. Runs, on two lattices lambda = 0 and 32.  The bin of a hit is (d - piece.begin + lambda + HITE_ANNOT_MAX_LIB_LEN) >> 6.  The
 *     hits of equal (piece, t, bin) are taken by ascending g (hits of equal g in any order: a run is made of minima, maxima and a count).  A hit joins the chain of the
 *     hit before it when g - g_prev <= HITE_ANNOT_GAP and g - g_first < HITE_ANNOT_MAX_SPAN (g_first: the chain's first hit);
 *     otherwise it starts a new chain.  A chain of at least HITE_ANNOT_MIN_HITS hits is a run (t, g_lo, g_hi, d_lo, d_hi): the
 *     first and the last g, the smallest and the largest d.  The runs of both lattices and of all pieces go on.
 *  4. Extension, per run.  dc = (d_lo + d_hi) >> 1, q_lo = g_lo - dc, q_hi = g_hi - dc.  The pads PL and PR each walk through
 *     HITE_ANNOT_PAD_0 .. _3, starting at the first.
 *        Q = [max(0, q_lo - PL), min(L, q_hi + 13 + PR)) of text t,
 *        S = [max(0, Q.begin + dc - 96), min(len, Q.end + dc + 96)) of the sequence (the whole sequence, not the piece).
 *     The alignment is step 4 of hite_pair_hsps as it stands (the same cell tuple, 2 / -4 / -5, the same "best", the same best-cell
 *     tie rule) with Q as rows and S as columns, on the whole rectangle inside the band dc - 96 <= g - q <= dc + 95; its result is
 *     an HSP at score >= HITE_PAIRHSP_MIN_SCORE, [qs, qe) in the text and [gs, ge) in the sequence.  No HSP: the run gives
 *     nothing.  If qs - Q.begin < HITE_ANNOT_EDGE while Q.begin > 0 and PL is not at its last value, PL steps; if Q.end - qe <
 *     HITE_ANNOT_EDGE while Q.end < L and PR is not at its last value, PR steps.  If either stepped and fewer than
 *     HITE_ANNOT_MAX_REDO alignments have been redone, the alignment is redone.  (A run spans less than HITE_ANNOT_MAX_SPAN + 13
 *     bases and the last pad is 8 192: a window stays under the 32 768 the packed start coordinates of a cell hold.)
 *  5. Resolve.  The record of an HSP is ten int32: seq, g_start, g_end (0-based, half-open, plus strand of the sequence), lib = t >> 1,
 *     strand = t & 1 (1: the entry's reverse complement), q_start, q_end (0-based, half-open, on the entry's FORWARD strand: for
 *     strand 1 they are L - qe, L - qs), score, matches, columns.  The order key of a record is (seq, g_start, g_end, lib, strand,
 *     q_start, q_end, -score, -matches, columns).  (a) Of the records equal in (seq, g_start, g_end, lib, strand, q_start, q_end)
 *     the first by the order key is kept (two lattices or two pieces find a copy twice).  (b) Of what (a) kept, a record A is
 *     dropped when a record B != A of the same sequence is better -- a higher score, or the same score and a smaller order key --
 *     and 5 * overlap(A, B) >= 4 * (A.g_end - A.g_start), overlap being the number of bases the two g intervals share.  A is held
 *     against every B of (a), dropped or not: the rule does not depend on an order.
 *  6. Order.  The records are written by ascending order key.
 *
 * Limits: n_lib <= HITE_ANNOT_MAX_LIB, every genome sequence shorter than 2^31, piece_len 0 or HITE_ANNOT_MIN_PIECE ..
 * HITE_ANNOT_PIECE: anything else, a negative count, a missing buffer or descending offsets is HITE_EINVAL.  n_seq = 0, n_lib = 0,
 * empty sequences and sequences shorter than a word are valid and give nothing.  recs holds cap records; *n_out is the number of
 * records of the call, HITE_ECAP when cap is smaller (the first cap are written).  lib_status (may be NULL) holds n_lib entries.
 * stats (may be NULL) receives HITE_ANNOT_STATS counters: table entries, of these silenced, entries too long, hits, runs (both
 * lattices, all pieces), alignments run, of these redone, runs without an HSP, HSPs before the resolve, duplicates dropped by
 * 5 (a), records dropped by 5 (b), records.
 * Pieces go to the device whole, each with the HITE_ANNOT_PAD_3 + 109 bases of its sequence on either side that a window can
 * reach, as many as stay within 64 MiB of bases; $HITE_ANNOT_BATCH_BYTES, read by hite_ctx_create, sets a smaller bound: a knob
 * that never changes a result.  Device memory: 12 bytes per table entry and as much again for its sort, the bases of a batch, 32
 * bytes per hit (the hit, its sort key and its diagonal, and as much again for the sort; the room for the hits comes from a first
 * pass that counts them and a second that writes them when the first guess was too small) and 72 per run. */
#define HITE_ANNOT_WORD        13
#define HITE_ANNOT_MAX_OCC     16
#define HITE_ANNOT_BIN_SHIFT   6
#define HITE_ANNOT_LATTICE     32
#define HITE_ANNOT_GAP         300
#define HITE_ANNOT_MIN_HITS    3
#define HITE_ANNOT_MAX_SPAN    8192
#define HITE_ANNOT_BAND_BELOW  96
#define HITE_ANNOT_BAND_ABOVE  96
#define HITE_ANNOT_PAD_0       256
#define HITE_ANNOT_PAD_1       1024
#define HITE_ANNOT_PAD_2       4096
#define HITE_ANNOT_PAD_3       8192
#define HITE_ANNOT_EDGE        32
#define HITE_ANNOT_MAX_REDO    3
#define HITE_ANNOT_PIECE       (1 << 24)
#define HITE_ANNOT_MIN_PIECE   256
#define HITE_ANNOT_OVERLAP     (1 << 16)
#define HITE_ANNOT_MAX_LIB_LEN 24576
#define HITE_ANNOT_MAX_LIB     32768
#define HITE_ANNOT_REC         10
#define HITE_ANNOT_STATS       12
int hite_annotate(hite_ctx *ctx, int64_t n_seq, const uint8_t *seqs, const int64_t *seq_off,
                  int32_t n_lib, const uint8_t *lib, const int64_t *lib_off, int32_t piece_len /* 0: HITE_ANNOT_PIECE */,
                  int64_t cap, int32_t *recs /* cap x 10 */, int64_t *n_out, int8_t *lib_status /* n_lib: 0 or -1 */, int64_t *stats);

/* ---- Helitron candidate scan --- multi_process_helitronscanner  Util.py:263 (third-party HelitronScanner.jar: scanHead, scanTail,
 * pairends, draw -pure_helitron per 50 kb part of longest_repeats_{i}.flanked.fa; judge_Helitron_transposons.py:27-34) -------------
 * In-tree stage, not pinned to the tool (no machine of the project runs it, and the tool's pairing rule and the tie-breaks of its
 * regex engine are not reproduced): the definition below, its CPU twin tests/helitron_twin.py, HIP == twin record for record and
 * score for score.
 *
 * Patterns are the tool's "LCV" lines (TrainingSet/head.lcvs, tail.lcvs; HiTE's data, read at run time, util.parse_lcvs):
 *  - head: the literal `TC`, an optional gap `.{n}` / `.{a,b}`, a body of letters ACGT and single `.`;
 *  - tail: a body, an optional gap, the literal `CT[AG]{2}`.
 * A compiled pattern (hite_lcv, 24 bytes) holds the gap range, the body length and, per body position j in the order of the line,
 * two bits at 2 j of `body` (A 0, C 1, G 2, T 3; 0 under a `.`) and of `care` (3 under a letter, 0 under a `.`).
 * Limits: body_len 1 .. HITE_HELITRON_MAX_BODY, gap_min <= gap_max <= HITE_HELITRON_MAX_GAP, at most HITE_HELITRON_MAX_PATTERNS
 * patterns per side, sequences shorter than 2^31 bytes, fewer than 2^31 anchors per call.
 *
 * The input is a CSR batch of sequences, as bytes.
 *  - A letter of a pattern matches only the same upper-case byte; `.` and a gap position match any byte (N, lower case);
 *    `[AG]` matches A or G.  Nothing matches across a sequence end.
 *  - Head score at p, the 0-based index of the T of `TC`: the number of head patterns with s[p:p+2] == "TC" whose body matches at
 *    p + 2 + g for at least one g in [gap_min, gap_max].  A pattern adds at most 1 per position; a repeated line counts again.
 *  - Tail score at q, the index of the last base of `CT[AG][AG]`: the number of tail patterns with s[q-3:q+1] matching the literal
 *    whose body ends at q - 4 - g for at least one such g.
 *  - Pairing, per sequence and strand: heads are the positions with score >= head_threshold; each pairs with the nearest q >= p +
 *    len_min - 1 that has tail score >= tail_threshold, if q - p + 1 <= len_max; a head without such a tail gives nothing.  Two heads
 *    may share a tail.  One record per paired head: (seq, start = p, end = q + 1, strand, head score, tail score).
 *  - Minus strand: the same on the reverse complement (A<->T, C<->G, every other byte N); start and end are reported on the forward
 *    strand (start = L - 1 - q, end = L - p), strand = 1.
 *  - Order: (seq, strand, start, end).
 * The tool's defaults, which the reference leaves alone: thresholds 1, length range 200 .. 20000 (the caller passes them).
 *
 * HITE_EINVAL for a negative count, descending offsets, a missing buffer, a pattern beyond a limit or malformed (care pairs other
 * than 0 / 3, bits beyond body_len, body bits under a `.`), a threshold or len_min below 1 (every base would be a head), len_min >
 * len_max.  n = 0 and zero patterns on a side are valid calls (no records).  Parallel output arrays of `cap` entries; *n_out = the
 * number of records, HITE_ECAP when it exceeds cap (the first cap are written).  stats (may be NULL): anchors tested, heads, tails,
 * pairs.  The _dev form takes the sequences on the device (d_seqs = the byte of seq_off[0]; the offsets and the outputs stay on the
 * host), works on `stream` and returns after it has drained. */
#define HITE_HELITRON_MAX_BODY 32
#define HITE_HELITRON_MAX_GAP 63
#define HITE_HELITRON_MAX_PATTERNS 1024
typedef struct hite_lcv {
    uint64_t body;
    uint64_t care;
    uint8_t gap_min, gap_max, body_len, pad[5];
} hite_lcv;
int hite_helitron_scan(hite_ctx *ctx, int64_t n, const uint8_t *seqs, const int64_t *seq_off, int32_t n_head, const hite_lcv *head,
                       int32_t n_tail, const hite_lcv *tail, int32_t head_threshold, int32_t tail_threshold, int32_t len_min,
                       int32_t len_max, int64_t cap, int32_t *seq_out, int32_t *start_out, int32_t *end_out, uint8_t *strand_out,
                       int32_t *hscore_out, int32_t *tscore_out, int64_t *n_out, int64_t *stats);
int hite_helitron_scan_dev(hite_ctx *ctx, int64_t n, const uint8_t *d_seqs, const int64_t *seq_off, int32_t n_head, const hite_lcv *head,
                           int32_t n_tail, const hite_lcv *tail, int32_t head_threshold, int32_t tail_threshold, int32_t len_min,
                           int32_t len_max, int64_t cap, int32_t *seq_out, int32_t *start_out, int32_t *end_out, uint8_t *strand_out,
                           int32_t *hscore_out, int32_t *tscore_out, int64_t *n_out, int64_t *stats, void *stream);
/* the scores alone, for every position of both strands: scores_out = four rows of seq_off[n] - seq_off[0] entries, each in its
 * strand's own coordinates at (offset of the sequence) + position: plus heads at p, plus tails at q, minus heads, minus tails (the
 * positions of the reverse complement).  0 where there is no anchor. */
int hite_helitron_scores(hite_ctx *ctx, int64_t n, const uint8_t *seqs, const int64_t *seq_off, int32_t n_head, const hite_lcv *head,
                         int32_t n_tail, const hite_lcv *tail, int32_t *scores_out);

/* ---- copy finding: this build's GPU-native stage where the reference runs the external
 * `minimap2 -ax map-ont -N 300 -p 0.2` + SAM filtering (get_full_length_copies_minimap2, Util.py:7933-8030;
 * third-party, unpinned -> parity is pinned against the build's own CPU twin, oracle/hite_oracle_copies.c,
 * whose header holds the definition: (w=10,k=15) minimizers, diagonal clustering, >= 3 anchors spanning
 * >= 80 % of the candidate and covering a candidate span >= 95 % of the genome span they cover (the target-coverage
 * filter of get_copies_minimap2), boundaries extrapolated from the extreme anchors, <= 300 copies per candidate
 * ordered by anchors).  Needs a packed genome (< 4 Gbp).  The index handle (*state_io, initially NULL)
 * is built once per genome; free it with hite_copy_index_release.
 * Output = the copy table get_full_length_copies_minimap2 returns, as the CSR that
 * hite_flank_region_align consumes (1-based inclusive coordinates).  n_cand < 2^19 per call.
 * _dev: the returned device arrays live in the index state's arena until the next call. */
int hite_copy_index_build(hite_ctx *ctx, void **state_io, void *stream);
/* A build keeps the genome's minimizers (tiles of 2048 window starts, in the handle's build arena); the next build on the same handle and
 * the same packed genome -- the restricted index of hite_find_copies_restricted, then the full index behind hite_genome_mask: stage 3.1's
 * prev_TE step -- computes only the tiles a mask call has touched since, and gives the index a build from scratch gives (the kept tiles
 * are void after hite_genome_pack* / hite_tr_mask; HITE_KEEP_MINIMIZERS=0 keeps nothing).  hite_copy_index_forget drops them: the next
 * build starts from the genome (what a benchmark that times repeated builds of one genome wants).  state NULL: no-op. */
int hite_copy_index_forget(void *state);
/* which interval the copy records of hite_find_copies[_dev] carry (process-wide DEFAULT, for contexts without a setting of their own): 1 = the ALIGNED interval, reference_start + 1 ..
 * reference_end exactly as get_copies_minimap2 reports it (Util.py:8026) -- the default since round 5, with the clipped candidate
 * bases handed on beside the records (hite_copy_clips) --; 0 = the interval of the WHOLE candidate, the ends that the extension clipped
 * extrapolated on the diagonal (the default of rounds 2-4); -1 = take the setting from the environment again
 * (HITE_COPY_INTERVAL=aligned | whole).  Both are twin-pinned (orc_find_copies_config). */
int hite_copy_config(int32_t aligned_interval);
/* the same setting for ONE context (what the library's per-context thread safety covers): 1 / 0 as above, -1 = follow the process-wide
 * setting of hite_copy_config again (the state of a new context) */
int hite_copy_config_ctx(hite_ctx *ctx, int32_t aligned_interval);
void hite_copy_index_release(void *state);
/* sizes of the last hite_find_copies[_dev] call on this index (diagnostics / roofline accounting):
 * out = {candidate minimizers, index hits, diagonal clusters, copies before the 300-per-candidate cap} */
int hite_copy_stats(void *state, int64_t out[4]);
/* the same four numbers + {chains with a long end to extend, the other chains, DP columns of the end extension, 0} */
int hite_copy_stats_ext(void *state, int64_t out[8]);

/* ---- all-vs-all seeding (stage 3.1) --- where the reference runs blastn of every 1 Mbp segment file against every
 * file: process_blast_alignments / sequence2sequenceBlastn  Util.py:4724-4780, 4068-4091 (rmblast is third-party and
 * absent: this is the build's own stage, pinned against its CPU twin orc_seed_allvsall) ---------------------------------
 * Uses the minimizer index of the packed genome (*state_io as for hite_find_copies; built on demand).  Output = the HSP
 * table hite_fmea_chain consumes (cols 0,1,6,7,8,9 of -outfmt 6): ids of the 'chr$offset' segments of seg_len bases
 * (hite_seed_segments gives the table, split_genome_chunks.py:41-52), 1-based inclusive coordinates inside the segment,
 * ss > se for reverse-strand hits; ordered by (query segment, subject segment).  *n_out is set even on HITE_ECAP.
 * max_anchors bounds the device memory of the anchor sort (24 B per anchor).  stats_out (may be NULL) =
 * {seeds, anchors, clusters, records}. */
int hite_seed_allvsall_dev(hite_ctx *ctx, void **state_io, int64_t seg_len, int64_t max_anchors, int32_t **d_qseg, int32_t **d_sseg,
                           int64_t **d_qs, int64_t **d_qe, int64_t **d_ss, int64_t **d_se, int64_t *n_out, int64_t *stats_out);
int hite_seed_segments(hite_ctx *ctx, int64_t seg_len, int32_t cap, int32_t *seg_chrom, int64_t *seg_off, int32_t *nseg_out);
/* Sharding of the all-vs-all stage over the ranks of a node (one process per GPU, the packed genome replicated):
 * after hite_seed_shard(ctx, rank, world) the seeding calls of this context emit the HSPs of rank's share only -- the
 * anchors whose (strand, diagonal) falls into the rank's range; clusters never straddle two ranges, so the tables of the
 * ranks, concatenated in rank order and stably sorted by (query segment, subject segment), are the unsharded table record
 * for record.  world <= 1 restores the whole.  hite_amd/dist.py routes the records to the owners of the query files
 * (all-to-all), runs hite_fmea_chain per file there and all-gathers the interval lists. */
int hite_seed_shard(hite_ctx *ctx, int32_t rank, int32_t world);
int hite_seed_allvsall(hite_ctx *ctx, void **state_io, int64_t seg_len, int64_t max_anchors, int64_t cap, int32_t *qseg,
                       int32_t *sseg, int64_t *qs, int64_t *qe, int64_t *ss, int64_t *se, int64_t *n_out, int64_t *stats_out);
int hite_find_copies(hite_ctx *ctx, void **state_io, int32_t n_cand, const uint8_t *cand, const int64_t *cand_off,
                     int64_t cap, int32_t *copy_first, int32_t *contig, int64_t *start1, int64_t *end1, uint8_t *minus,
                     int32_t *anchors, int64_t *n_out);
/* _dev PRECONDITION: d_cand must be readable for 16 bytes beyond cand_bytes (the end extension fetches candidate words ahead
 * of use); hite_find_copies pads its upload, a caller that owns the device buffer allocates cand_bytes + 16. */
int hite_find_copies_dev(hite_ctx *ctx, void *state, int32_t n_cand, const uint8_t *d_cand, const int64_t *d_cand_off,
                         int64_t cand_bytes, int32_t **d_copy_first, int64_t *n_copies, int32_t **d_contig,
                         int64_t **d_start1, int64_t **d_end1, uint8_t **d_minus, int32_t **d_anchors, void *stream);
/* hite_find_copies_dev for ONE candidate set on a genome whose index nothing else will use (stage 3.1 masks the genome with the
 * previous TE library -- Util.py:6021-6081 `mask_genome_intactTE`, the reference's blastn of the library against the chunk -- and only then
 * indexes the MASKED genome): the index is built for these candidates only -- the genome pass keeps the minimizers whose hash one of
 * their minimizers looks up, so the hash sort and the directory run on those few entries.  Every entry the look-up would read is
 * there, with the same run lengths and order: the copy table equals hite_find_copies_dev's on the full index (tests assert it).
 * *state_io as for hite_find_copies (created when null); the handle is left flagged restricted, and hite_find_copies[_dev] /
 * hite_seed_allvsall[_dev] rebuild the full index before they use it.  Same _dev PRECONDITION. */
int hite_find_copies_restricted_dev(hite_ctx *ctx, void **state_io, int32_t n_cand, const uint8_t *d_cand, const int64_t *d_cand_off,
                                    int64_t cand_bytes, int32_t **d_copy_first, int64_t *n_copies, int32_t **d_contig,
                                    int64_t **d_start1, int64_t **d_end1, uint8_t **d_minus, int32_t **d_anchors, void *stream);
/* host-buffer form (arguments as hite_find_copies) */
int hite_find_copies_restricted(hite_ctx *ctx, void **state_io, int32_t n_cand, const uint8_t *cand, const int64_t *cand_off,
                                int64_t cap, int32_t *copy_first, int32_t *contig, int64_t *start1, int64_t *end1, uint8_t *minus,
                                int32_t *anchors, int64_t *n_out);
/* The clip words of the records of the last hite_find_copies[_dev] / _restricted[_dev] call on this index, in record order: candidate
 * bases the left | right << 16 end extension cut off (minimap2 would soft-clip them; each <= 5 % of the candidate), in the orientation
 * of the genome.  For aligned intervals (the default) hite_flank_region_align_clip[_dev] takes them; zero for whole-candidate
 * intervals (hite_copy_config(0): the clipped bases are inside the interval).  _dev: *d_clip (NULL when the call found nothing) lives as long
 * as the copy table; host form: cap >= the number of records, else HITE_ECAP. */
int hite_copy_clips_dev(void *state, const uint32_t **d_clip, int64_t *n);
int hite_copy_clips(void *state, int64_t cap, uint32_t *clip);

/* ---- full-length copy support of the confident intact LTR elements --- FiLTR's step 4 (bin/FiLTR-main/src/Util.py:6119
 * filter_ltr_by_copy_num): `minimap2 -ax asm20 -N 100 -p 0.2` of every element against the genome, get_copies_minimap2 (:6509-6556)
 * at 0.985, then get_intact_ltr_copies (:11022-11147).  The search is this build's copy finder (unpinned against minimap2); the
 * rules on its records are the reference's, integer for integer, every floating-point compare in binary64 with the reference's
 * operations in its order (a division or a multiplication of exactly converted integers, then the compare; a zero denominator,
 * where the reference raises ZeroDivisionError, answers false).  Twin: tests/ltrcopy_twin.py; rules: hite_amd/csrc/hite_ltrcopy.h.
 *  The table: element k has el_len[k] bases and the records copy_first[k] .. copy_first[k + 1] (copy_first[0] = 0, at most 300 each)
 *  -- contig, start1 <= end1 (1-based, inclusive) and clip = the element's bases the alignment left out at its ends,
 *  left | right << 16 (hite_copy_clips; the soft clips of a record of minimap2; clip NULL: none).  The candidate lines, in the order
 *  of ltr_lines: std_start = lLTR_start - 1, std_end = rLTR_end on std_contig.
 *  1. Coverage: aligned = el_len - left - right; a record stays when aligned / el_len >= full_length_coverage and
 *     aligned / (end1 - start1 + 1) >= full_length_coverage.
 *  2. Candidate table: in input order a line goes into the bucket (std_contig, map_fragment(std_start, std_end, segment_len))
 *     (:4837) unless a line stored there before overlaps it (get_overlap_len, :4200: min of the ends - max of the starts, at least
 *     0) by >= overlap_threshold of |end - start| of either.  A line beyond the segments of its contig is not stored.
 *  3. Match: a record stays when a stored line of the bucket (contig, map_fragment(start1, end1, segment_len)) -- that bucket alone
 *     -- passes the same two-sided test with (start1, end1).
 *  4. Redundancy, per element: the records that stayed, stably ascending by end1 - start1 -- before the sort the reference holds
 *     them contig by contig, the contigs in the order in which the records that pass rule 1 first name them over the whole call,
 *     and in input order inside a contig --; record i is dropped when a LATER record j of that order lies on the same contig with
 *     min(end) - max(start) + 1 >= 0.95 * (end1_i - start1_i + 1) (the literal 0.95).  The others are the output, in that order.
 * Output: the copies of element k are out_first[k] .. out_first[k + 1] of (out_contig, out_start1, out_end1); *n_out = their number,
 * set even when HITE_ECAP is returned because it exceeds cap (out_first is all zero then and no copy is written; stats are).  stats (may be NULL) =
 * {records in, records that pass rule 1, that also pass rule 3, copies kept}.  n_el = 0, n_std = 0 and empty elements are valid.
 * HITE_EINVAL: a negative count, a missing buffer, descending offsets, an element of more than 300 records, a contig outside
 * 0 .. n_contig - 1, a negative coordinate of a line, thresholds that are NaN or outside [0, 1], segment_len <= 0.
 * hite_ltr_copy_support takes the elements as sequences (el, el_off as hite_find_copies takes candidates; n_el < 2^19; *state_io the
 * index handle, built when NULL), runs hite_find_copies_dev on the packed genome and applies the rules to its table where it lies:
 * the copy table never comes down.  The finder runs in aligned-interval mode whatever hite_copy_config[_ctx] says; the context's
 * setting is the same after the call.  Contigs and their lengths are the packed genome's. */
int hite_ltr_copy_support_records(hite_ctx *ctx, int64_t n_el, const int64_t *el_len, const int32_t *copy_first /* n_el + 1 */,
                                  const int32_t *contig, const int64_t *start1, const int64_t *end1, const uint32_t *clip, int64_t n_std,
                                  const int32_t *std_contig, const int64_t *std_start, const int64_t *std_end, int32_t n_contig,
                                  const int64_t *contig_len, double full_length_coverage, double overlap_threshold, int64_t segment_len,
                                  int64_t cap, int32_t *out_first /* n_el + 1 */, int32_t *out_contig, int64_t *out_start1, int64_t *out_end1,
                                  int64_t *n_out, int64_t *stats /* 4 */);
int hite_ltr_copy_support(hite_ctx *ctx, void **state_io, int32_t n_el, const uint8_t *el, const int64_t *el_off /* n_el + 1 */, int64_t n_std,
                          const int32_t *std_contig, const int64_t *std_start, const int64_t *std_end, double full_length_coverage,
                          double overlap_threshold, int64_t segment_len, int64_t cap, int32_t *out_first /* n_el + 1 */, int32_t *out_contig,
                          int64_t *out_start1, int64_t *out_end1, int64_t *n_out, int64_t *stats /* 4 */);

/* ---- star alignment: this build's GPU-native stage where the reference runs the external
 * `mafft --preservecase --quiet --thread 1` (Util.py:10416; third-party, unpinned, absent -> parity unpinned against
 * mafft itself).  Definition of the stage: every row is aligned to the centre (first row of the candidate) by the
 * optimal global alignment under the costs mismatch 1, gap 3 per base (two bases match only when they are the same
 * A, C, G or T; a lower-case a / c / g / t of a ROW is read as its base -- mafft --preservecase compares case-insensitively --
 * BUT a run of bytes with bit 5 set at the BEGINNING or END of a row is a run of pad bytes, see HITE_IS_ROW_PAD above: lower
 * case at the ends of a row is RESERVED for pads and leaves the alignment as gaps.  A caller whose windows may begin or end with
 * soft-masked lower-case sequence upper-cases them first, as hite_amd/util.py does; the centre is compared as it is, upper
 * case), canonical traceback diagonal > up > left -- the textbook full-matrix
 * programme of oracle/hite_oracle_nw.c; insertion blocks are left-justified.  The device computes it with a banded
 * bit-parallel aligner that CERTIFIES its result (twin: oracle/hite_oracle_msa.c, byte-exact): a certified row is the
 * alignment of the definition, a row without certificate is a valid alignment whose cost bounds the optimum from above.
 * hite_align_config: exact_cap = 0 (fast: band of 128 centre rows only), 8 / 16 / 32 = widest band (x 32 rows) that
 * is tried to obtain a certificate (default 8, or the environment variable HITE_ALIGN_EXACT).
 * hite_align_stats: out8 = pairs, certified, kept from a band wider than 128 rows, wide fall-backs, rows dropped,
 * sum of the costs, sum of the row lengths (columns), exact_cap -- accumulated over the calls since the last reset.
 * windows of candidate c = rows row_first[c] .. row_first[c+1]-1 of the CSR (win, win_off);
 * the first row of each candidate is the centre.  Window length <= 32767.  A row that cannot be aligned (shorter than
 * half the centre, or an insertion / deletion beyond the widest band) is DROPPED: rows_out[c] (may be NULL) = rows of
 * the alignment.
 * hite_star_msa: pass msa_out = NULL to get cols_out / rows_out only; otherwise the rows x cols matrices are
 * written at msa_off_out[c] (16-byte aligned slots) and msa_cap is checked.
 * hite_star_msa_info: same + info_out = 5 int32 per input window (zeros for centres): cost U of the alignment kept,
 * certified, status (0 aligned, else dropped), the certificate's bound k*, band words of the run kept (| 0x100: wide fall-back).
 * _dev: window g starts at d_win_off[g] (16-byte aligned, readable up to the next multiple of 16) and is d_win_len[g]
 * long; d_ops_base[n+1] = exclusive scan of (R_c + 1) * (m_c + 1) (m_c = centre length),
 * ops_elems its last element; d_status[c] != 0 marks a candidate whose alignment failed (wider than 65535 columns;
 * cols_out[c] = 0); d_rows_out (may be NULL) = rows per alignment.  The fill call must follow the align call on the
 * same ctx/stream. */
int hite_align_config(hite_ctx *ctx, int32_t exact_cap);
/* hite_align_lanes: the LONGEST pairs of a call are aligned by kernels that spread one pair over several lanes (4 or 8 lanes
 * = the words of its band in the forward pass; a wavefront whose lanes re-compute 64 strips at once in the traceback), beside
 * the thread-per-pair kernels of the others -- a kernel cannot end before its longest pair's dependent chain, which in a small
 * batch (one rank's share of a sharded run; the reference gives every candidate its own process, Util.py:8141-8147) is the
 * step.  Same recurrence, same records, same ops: which kernel takes a pair never changes a result.  min_cols = -1 (default,
 * or the environment variable HITE_ALIGN_LANES): pairs whose row is longer than 1/160 000 of all pair-columns of the call
 * and at least 512 columns; >= 0: pairs of at least this many columns (0: every pair -- the parity tests); -2: never. */
int hite_align_lanes(hite_ctx *ctx, int32_t min_cols);
int hite_align_stats(hite_ctx *ctx, int64_t *out8, int32_t reset);
int hite_star_msa(hite_ctx *ctx, int32_t n, const uint8_t *win, const int64_t *win_off, const int32_t *row_first,
                  int32_t *cols_out, int32_t *rows_out, int64_t msa_cap, uint8_t *msa_out, int64_t *msa_off_out);
/* hite_star_msa followed by remove_sparse_col_in_align_file in one step (same two-call protocol; cols_out = surviving columns) */
int hite_star_msa_sparse(hite_ctx *ctx, int32_t n, const uint8_t *win, const int64_t *win_off, const int32_t *row_first,
                         int32_t *cols_out, int32_t *rows_out, int64_t msa_cap, uint8_t *msa_out, int64_t *msa_off_out);
int hite_star_msa_info(hite_ctx *ctx, int32_t n, const uint8_t *win, const int64_t *win_off, const int32_t *row_first,
                       int32_t *cols_out, int32_t *rows_out, int32_t *info_out, int64_t msa_cap, uint8_t *msa_out,
                       int64_t *msa_off_out);
/* One call for the host form (the sizes call + the fill call each run the whole pairwise alignment): the alignments come back in
 * a host buffer the library allocates (*msa_out, *msa_bytes_out bytes, alignment i at msa_off_out[i]; release with
 * hite_host_free); sparse != 0: sparse columns removed; info_out (optional): 5 int32 per input row as hite_star_msa_info. */
int hite_star_msa_once(hite_ctx *ctx, int32_t n, const uint8_t *win, const int64_t *win_off, const int32_t *row_first,
                       int32_t sparse, int32_t *cols_out, int32_t *rows_out, int32_t *info_out, uint8_t **msa_out,
                       int64_t *msa_off_out, int64_t *msa_bytes_out);
void hite_host_free(void *p);
int hite_star_msa_dev(hite_ctx *ctx, int32_t n, const uint8_t *d_win, const int64_t *d_win_off,
                      const int32_t *d_win_len, const int32_t *d_row_first, int64_t total_rows, const int64_t *d_ops_base, int64_t ops_elems,
                      int32_t max_win_len, int32_t *d_cols_out, int32_t *d_status, int32_t *d_rows_out, void *stream);
int hite_star_msa_fill_dev(hite_ctx *ctx, int32_t n, const uint8_t *d_win, const int64_t *d_win_off,
                           const int32_t *d_win_len, const int32_t *d_row_first, const int64_t *d_ops_base, const int32_t *d_cols,
                           const int64_t *d_msa_off, uint8_t *d_msa, void *stream);
/* Fused variant used by hite_flank_region_align: alignment + column layout + the column selection of
 * remove_sparse_col_in_align_file (Util.py:10344-10405) in one step, so that only the surviving columns are ever written.
 * d_cols_out = columns of the full alignment (0 = failed), d_new_cols = surviving columns, d_last_extra = fill hint.
 * hite_star_msa_fill_sparse_dev then writes rows x d_new_cols[i] bytes at d_msa_off[i]; the result is byte-identical to
 * hite_star_msa_fill_dev followed by hite_sparse_cols_dev. */
int hite_star_msa_sparse_dev(hite_ctx *ctx, int32_t n, const uint8_t *d_win, const int64_t *d_win_off,
                             const int32_t *d_win_len, const int32_t *d_row_first, int64_t total_rows,
                             const int64_t *d_ops_base, int64_t ops_elems, int32_t max_win_len, int32_t *d_cols_out,
                             int32_t *d_status, int32_t *d_new_cols, int32_t *d_last_extra, int32_t *d_rows_out, void *stream);
int hite_star_msa_fill_sparse_dev(hite_ctx *ctx, int32_t n, const uint8_t *d_win, const int64_t *d_win_off,
                                  const int32_t *d_win_len, const int32_t *d_row_first, const int64_t *d_ops_base,
                                  const int32_t *d_new_cols, const int32_t *d_last_extra, const int64_t *d_msa_off,
                                  uint8_t *d_msa, void *stream);
/* The sparse fill has two forms that write the same bytes: tiles of positions built in LDS (the default) and the per-cell form.
 * mode 1 / 0 selects the tile / per-cell form for this context, -1 follows the process default again (HITE_FILL_TILES=0 in the
 * environment: the per-cell form).  hite_fill_tile_limits: out[0] = positions of a tile, out[1] = bytes of a row's window range
 * (and of a tile's output columns) that fit the LDS slot, out[2] = rows a workgroup takes per trip, out[3] = row slices of a
 * candidate (a workgroup takes the rows out[2] * z + wave, stepping by out[2] * out[3]). */
int hite_fill_config_ctx(hite_ctx *ctx, int32_t mode);
/* The window gather of the fine stage has two forms that write the same window bytes: in chunks of the destination -- a row
 * descriptor per row, items of up to 256 chunks of 16 bytes per wavefront, the bytes between a row's length and the end of its slot
 * zero (the default) -- and a wavefront per row, which leaves those bytes as they were.  mode 1 / 0 selects the chunk / per-row form
 * for this context, -1 follows the process default again (HITE_GATHER_CHUNKS=0 in the environment: the per-row form). */
int hite_gather_config_ctx(hite_ctx *ctx, int32_t mode);
/* the form the next call of this context runs: 1 chunks / 0 per row (its own setting, else the process default) */
int hite_gather_mode_ctx(hite_ctx *ctx);
/* The star alignment re-aligns the pairs whose traceback left its slice (the fall-back: a few dozen lone wavefronts).  mode 1: that runs
 * beside the pad fix and the layout of the candidates it does not touch, which are then done once more for the others; mode 0: one after
 * the other; -1 follows the process default again (on, unless HITE_FALLBACK_OVERLAP=0 in the environment).  The same bytes either way. */
int hite_fallback_overlap_ctx(hite_ctx *ctx, int32_t mode);
/* The traceback of that fall-back has two forms that write the same bytes: by runs -- up to 64 diagonal or left steps of the path per
 * trip to memory (the default) -- and a column per step.  mode 1 / 0 selects the run / column form for this context, -1 follows the
 * process default again (HITE_WIDE_TB_RUNS=0 in the environment: a column per step). */
int hite_wide_tb_runs_ctx(hite_ctx *ctx, int32_t mode);
int hite_fill_tile_limits(int32_t out[4]);

/* ---- the fine stage in one call --- body of flank_region_align_v5 from the copy table on ----------
 * (Util.py:8095-8194 + run_find_members_v8 :10439 + is_TE_from_align_file :10407).
 * Candidates: cand/cand_off CSR (cur_seq of each candidate).  Copies of candidate c are entries
 * copy_first[c] .. copy_first[c+1]-1 of (contig, start1, end1, minus) -- what
 * get_full_length_copies_minimap2 (:7933) returns, 1-based inclusive.  Needs a packed genome.
 * calls[c] = the tuple is_TE_from_align_file returns for candidate c; consensus bytes are packed
 * into cons (cons_off/cons_len in the record); HITE_ECAP if cons_cap is too small.
 * stats_out (12 x int64, host, optional): [0..3] pass A rows, window bytes, matrix bytes, alignment
 * algorithmic bytes; [4..7] the same for pass B; [8],[9] anti-diagonal steps of pass A / B (x64 = DP
 * cells); [10] consensus bytes kept; [11] cleaned alignment columns judged (both passes).
 * _dev: all pointers are device pointers; *state_io (initially NULL) keeps the arenas between
 * calls so the steady state performs no allocation; free it with hite_pipeline_release. */
int hite_flank_region_align(hite_ctx *ctx, int32_t te_type, int32_t plant, int32_t n_cand, const uint8_t *cand,
                            const int64_t *cand_off, const int32_t *copy_first, int64_t n_copies, const int32_t *contig,
                            const int64_t *start1, const int64_t *end1, const uint8_t *minus, int32_t flank,
                            hite_call *calls, uint8_t *cons, int64_t cons_cap, int64_t *stats_out);
int hite_flank_region_align_dev(hite_ctx *ctx, void **state_io, int32_t te_type, int32_t plant, int32_t n_cand,
                                const uint8_t *d_cand, const int64_t *d_cand_off, const int32_t *d_copy_first,
                                int64_t n_copies, const int32_t *d_contig, const int64_t *d_start1, const int64_t *d_end1,
                                const uint8_t *d_minus, int32_t flank, hite_call *d_calls, uint8_t *d_cons,
                                int64_t cons_cap, int64_t *stats_out, void *stream);
/* The same stage with the clip words of the copy records given.  A copy record in the REFERENCE'S coordinates (reference_start + 1 ..
 * reference_end of the alignment, Util.py:8026, as get_copies_minimap2 hands it to flank_region_align_v5: what hite_find_copies reports
 * by default) covers only the part of the candidate that aligned; `clip` (per record) says how many candidate bases were left out at
 * its two ends -- left | right << 16, in the orientation of the genome (hite_copy_clips[_dev]) -- and the row's window (interval +
 * flanks, Util.py:8110-8125) is padded with pad bytes (HITE_IS_ROW_PAD): the CENTRE's own first / last bases in lower case, which match
 * the centre positions they face -- in front by the left clip (a minus copy: the right one, its window is reverse-complemented) LESS
 * what the centre's own record leaves out on that side (round 6: the row's first base faces centre position clip_row - clip_centre),
 * behind by the other; the centre (the first row kept) is never padded; the first500 + last500 form of a long window (Util.py:8119) is
 * cut from the padded window; the <= 100 rows are chosen by the length of the genome window.  A padded row faces the part of the
 * centre its copy was found with, so its path stays on the diagonal; the pads leave the alignment as gaps of the row (where mafft,
 * which does not charge terminal gaps like internal ones, leaves such a row unaligned).
 * clip == NULL (and hite_flank_region_align[_dev], which have no such argument) -- the reference's own 5-tuples, real minimap2 records:
 * the clip words are ESTIMATED from the sequences (round 6, clip_probe_kernel; definition orc_clip_probe in
 * oracle/hite_oracle_copies.c): the first 21 bases of the record's interval, read on the candidate's strand, are laid on the candidate
 * at every offset 0 .. |cand| / 20 + 32; the offset with the fewest mismatches (the smallest on ties) is the left clip when it has <= 5
 * mismatches, else the next 21 bases are tried, else 0; the right clip the same from the other end.  A whole-candidate record probes
 * to 0 | 0.  Nothing is inferred from where the caller's arrays live (round 5 recognised the finder's own device table by its address).
 * Rows cut from aligned intervals WITHOUT pads are aligned globally at 3 per gap base against a centre that is clip_l + clip_r bases
 * longer: on config C2 8 633 rows left the band and TE calls fell by a fifth (profiles/r05_scale_tests.txt, last line). */
/* the estimate by itself (host buffers, arguments as hite_flank_region_align's table): clip_out[k] = left | right << 16 in the orientation
 * of the genome, what a call without clip words pads the rows by */
int hite_clip_probe(hite_ctx *ctx, int32_t n_cand, const uint8_t *cand, const int64_t *cand_off, const int32_t *copy_first,
                    int64_t n_copies, const int32_t *contig, const int64_t *start1, const int64_t *end1, const uint8_t *minus,
                    uint32_t *clip_out);
/* the rows of one pass by themselves (host buffers; parity tests, diagnostics): the table arguments of hite_flank_region_align_clip
 * (clip == NULL: probed, as the stage does), run through the stage's own row selection, row records and window gather.  pass = 0: the
 * modes of pass A (a candidate with a window > 1000 gives the first500 + last500 forms of those windows only); pass = 1: the modes
 * of pass B as if every such form had passed (full windows of the candidates that have a window > 1000, no row for the others).
 * nrows[n_cand]; per row (candidate after candidate, input order within one) row_copy = index into the table, row_len = bytes of
 * the (padded) window, row_trunc = 1 for a first500 + last500 form; row r's bytes are win[win_off[r] .. win_off[r] + row_len[r])
 * (slots are multiples of 16 bytes; win_off has rows + 1 entries).  totals[4] = rows, window bytes, longest row_len, 0 -- filled,
 * like nrows, also when HITE_ECAP is returned because rows > row_cap or window bytes > win_cap (nothing else is written then). */
int hite_fine_rows(hite_ctx *ctx, int32_t n_cand, const uint8_t *cand, const int64_t *cand_off, const int32_t *copy_first,
                   int64_t n_copies, const int32_t *contig, const int64_t *start1, const int64_t *end1, const uint8_t *minus,
                   const uint32_t *clip, int32_t flank, int32_t pass, int32_t *nrows, int64_t row_cap, int32_t *row_copy,
                   int32_t *row_len, uint8_t *row_trunc, int64_t *win_off, int64_t win_cap, uint8_t *win, int64_t *totals);
int hite_flank_region_align_clip(hite_ctx *ctx, int32_t te_type, int32_t plant, int32_t n_cand, const uint8_t *cand,
                                 const int64_t *cand_off, const int32_t *copy_first, int64_t n_copies, const int32_t *contig,
                                 const int64_t *start1, const int64_t *end1, const uint8_t *minus, const uint32_t *clip, int32_t flank,
                                 hite_call *calls, uint8_t *cons, int64_t cons_cap, int64_t *stats_out);
int hite_flank_region_align_clip_dev(hite_ctx *ctx, void **state_io, int32_t te_type, int32_t plant, int32_t n_cand,
                                     const uint8_t *d_cand, const int64_t *d_cand_off, const int32_t *d_copy_first,
                                     int64_t n_copies, const int32_t *d_contig, const int64_t *d_start1, const int64_t *d_end1,
                                     const uint8_t *d_minus, const uint32_t *d_clip, int32_t flank, hite_call *d_calls,
                                     uint8_t *d_cons, int64_t cons_cap, int64_t *stats_out, void *stream);
void hite_pipeline_release(void *state);

/* ---- per-stage profiling: HIP events recorded on the launch stream around each kernel of the
 * pipeline (stage names = kernel names).  ms_total / launches accumulate since the last reset. */
int hite_profile_enable(hite_ctx *ctx, int on);
int hite_profile_reset(hite_ctx *ctx);
int hite_profile_count(hite_ctx *ctx);
int hite_profile_get(hite_ctx *ctx, int idx, char *name_out, double *ms_total, int64_t *launches);

/* copy a device range returned by a _dev entry point to the host (synchronises the device) */
int hite_memcpy_d2h(void *dst, const void *d_src, int64_t bytes);

/* ---- timing helper: HIP-event elapsed ms around work already enqueued on `stream` ---------- */
int hite_event_create(void **ev);
int hite_event_record(void *ev, void *stream);
int hite_event_elapsed_ms(void *ev_start, void *ev_stop, float *ms);
int hite_event_destroy(void *ev);

/* ---- merge of the boundary calls between the GPUs of a node -----------------------------------------------
 * The reference has no counterpart (it collects results from a fork()ed process pool, Util.py:8141-8194).  One ncclAllGather
 * (RCCL over xGMI) of `bytes_per_rank` bytes per rank -- the fixed 32-byte hite_call records of a rank's share, padded to the
 * largest share -- on the communicator the CALLER owns (`nccl_comm` = its ncclComm_t), asynchronous on `stream`; d_recv holds
 * world x bytes_per_rank bytes in rank order.  The library neither links nor loads RCCL: the symbol is taken from the RCCL already in
 * the process (torch's, or the application's -- the communicator came out of it); HITE_ENODEV when there is none.  The Python driver's
 * merge (hite_amd/dist.py) goes through torch.distributed, which keeps its communicator to itself; this entry is for a C / C++ host. */
int hite_allgather_records(hite_ctx *ctx, void *nccl_comm, const void *d_send, void *d_recv, int64_t bytes_per_rank, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HITE_GPU_H */
