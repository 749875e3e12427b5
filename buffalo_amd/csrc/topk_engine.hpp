// The top-k engine of csrc/topk.hip as other translation units of the library drive it (csrc/eval.hip: the validation ranking).
#pragma once
#include "common.hpp"

namespace bfh {

// a TopkHandle bound to `device` (own stream, own scratch buffers); release with `delete`
HandleBase* topk_engine_new(int device);
// the knobs of bfh_topk_set_mode
void topk_engine_set_mode(HandleBase* engine, const std::string& name, int64_t value);
// TopkHandle::rank_unseen: d_out_keys[b * k + r] = the r-th best column of query row d_rows[b] of dP among the columns that are not in
// that user's run of the END-offset CSR (d_seen_indptr, d_seen_keys; keys ascending inside a row), by (score desc, index desc); -1 beyond
// the unseen columns.  Scores: dP[row] . dQ[col] (+ dQb[col]) as topk_scores_kernel forms them.  All pointers are device pointers; the
// engine's stream is idle on return and its stats hold the HIP-event times (kernel_ms scores, aux_ms pack + selection).
void topk_engine_rank_unseen(HandleBase* engine, const int32_t* d_rows, int nq, const float* dP, const float* dQ, int q_rows, int d, int ld,
                             const float* dQb, const int64_t* d_seen_indptr, const int32_t* d_seen_keys, int k, int32_t* d_out_keys, int max_batch);

}  // namespace bfh
