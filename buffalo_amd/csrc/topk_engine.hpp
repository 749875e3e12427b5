// The top-k engine of csrc/topk.hip as other translation units of the library drive it (csrc/eval.hip: the validation ranking).
#pragma once
#include "common.hpp"

namespace bfh {

// The training matrix of a seen-aware ranking (bfh_eval_set_data, bfh_topk_set_seen) as the kernels rely on it: `num_users` non-decreasing
// END offsets <= nnz, the last one nnz, keys inside [0, num_items) and ascending inside a row.  Throws with a message that starts with `who`.
inline void validate_seen_csr(const char* who, int num_users, int num_items, const int64_t* seen_indptr, const int32_t* seen_keys, int64_t nnz) {
    const std::string w = std::string(who) + ": ";
    BFH_REQUIRE(num_users > 0 && num_items > 0, w + "empty shape");
    BFH_REQUIRE(nnz >= 0, w + "negative count");
    BFH_REQUIRE(seen_indptr && (nnz == 0 || seen_keys), w + "null training matrix");
    int64_t prev = 0;
    for (int u = 0; u < num_users; ++u) {
        const int64_t end = seen_indptr[u];
        if (end < prev || end > nnz) throw Error(BFH_ERR_INVALID, w + "indptr is not a non-decreasing list of END offsets <= nnz at row " + std::to_string(u));
        for (int64_t i = prev; i < end; ++i) {
            const int32_t k = seen_keys[i];
            if (k < 0 || k >= num_items) throw Error(BFH_ERR_INVALID, w + "training key outside [0, num_items) at position " + std::to_string(i));
            if (i > prev && k < seen_keys[i - 1]) throw Error(BFH_ERR_INVALID, w + "the keys of a training row must ascend (position " + std::to_string(i) + ")");
        }
        prev = end;
    }
    BFH_REQUIRE(prev == nnz, w + "the last END offset must equal nnz");
}

// a TopkHandle bound to `device` (own stream, own scratch buffers); release with `delete`
HandleBase* topk_engine_new(int device);
// the knobs of bfh_topk_set_mode
void topk_engine_set_mode(HandleBase* engine, const std::string& name, int64_t value);
// TopkHandle::rank_unseen: d_out_keys[b * k + r] = the r-th best column of query row d_rows[b] of dP among the columns that are not in
// that user's run of the END-offset CSR (d_seen_indptr, d_seen_keys; keys ascending inside a row), by (score desc, index desc); -1 beyond
// the unseen columns.  Scores: dP[row] . dQ[col] (+ dQb[col]) as topk_scores_kernel forms them.  All pointers are device pointers; the
// engine's stream is idle on return and its stats hold the HIP-event times (kernel_ms scores, aux_ms pack + selection) and the fused
// path's counters (merges, exchanges: bfh_topk_get_stats).
void topk_engine_rank_unseen(HandleBase* engine, const int32_t* d_rows, int nq, const float* dP, const float* dQ, int q_rows, int d, int ld,
                             const float* dQb, const int64_t* d_seen_indptr, const int32_t* d_seen_keys, int k, int32_t* d_out_keys, int max_batch);

}  // namespace bfh
