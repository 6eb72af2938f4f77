// hite_align.h -- internal interface of the pairwise aligner (hite_align.hip), used by the star alignment (hite_msa.hip).
#pragma once
#include "hite_common.h"

// Aligns every row of every candidate to the candidate's first row (its centre).  Row r of candidate c (global row
// g = row_first[c] + r, r >= 1) gets m + 1 ops at d_ops + ops_base[c] + r * (m + 1), m = length of the centre:
//   ops[p], p < m : q | gap << 15 -- centre position p faces row position q (gap = 0) or a gap before row position q
// (oracle/hite_oracle_nw.c).  d_row_dead (total_rows, may be NULL): 1 for a row that could not be aligned;
// d_cand_flag (n_cand, may be NULL): set to 2 for candidates that lost a row; d_info (5 x total_rows, may be NULL):
// per row the cost U, certified, status, k*, band words | 0x100 (fall-back).  `tag` names the profiler stages.
int hite_align_run(hite_ctx *ctx, int32_t n_cand, const uint8_t *d_win, const int64_t *d_win_off, const int32_t *d_win_len,
                   const int32_t *d_row_first, int64_t total_rows, const int64_t *d_ops_base, uint16_t *d_ops,
                   int32_t *d_row_dead, int32_t *d_cand_flag, int32_t *d_info, const char *tag, hipStream_t st);
// The same in two halves.  hite_align_begin does everything up to the fall-back (the pairs whose traceback left its slice, a few
// dozen lone wavefronts); hite_align_finish writes d_row_dead, d_cand_flag, d_info and the counters.  With fork == NULL the
// fall-back runs on `st` and the two halves back to back are hite_align_run.  With fork != NULL (d_row_dead and d_cand_flag are
// required then) and at least one fall-back pair, the fall-back runs on the aligner's high-priority stream and the caller may
// enqueue on `st`, between the halves, work on the candidates that own none of its rows:
//   cnt          fall-back pairs (0: no fork, nothing else is set; the caller proceeds as after hite_align_run) -- also an upper
//                bound of the pending candidates, for the grid of a launch over d_pend_list
//   dead_before  rows outside the fall-back's list that are dead already; when > 0, d_row_dead and d_cand_flag of the candidates
//                that are not pending are valid from the begin half on
//   d_pending    n_cand flags: 1 for a candidate with a row in the fall-back.  Nothing on `st` may touch anything of such a
//                candidate before hite_align_finish -- its ops, the status of its rows, whatever is derived from them
//   d_pend_list, d_pend_count  those candidates, each once, in no fixed order, and how many (both on the device)
// The arrays live in the aligner's arena until the next hite_align_begin.
struct HiteAlignFork {
    int64_t cnt, dead_before;
    const int32_t *d_pending, *d_pend_list, *d_pend_count;
};
int hite_align_begin(hite_ctx *ctx, int32_t n_cand, const uint8_t *d_win, const int64_t *d_win_off, const int32_t *d_win_len,
                     const int32_t *d_row_first, int64_t total_rows, const int64_t *d_ops_base, uint16_t *d_ops,
                     int32_t *d_row_dead, int32_t *d_cand_flag, int32_t *d_info, const char *tag, hipStream_t st, HiteAlignFork *fork);
int hite_align_finish(hite_ctx *ctx);
void hite_align_release(hite_ctx *ctx);
