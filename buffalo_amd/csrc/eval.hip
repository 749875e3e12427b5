// Validation on the device -- Evaluable.get_validation_results (buffalo/evaluate/base.py:44-148) for gfx950: kernels, handle, C ABI.
//
// The reference ranks topk + max_seen candidates per user, throws the user's training items away in Python (filter_seen_items,
// base.py:71-78) and walks every list entry with `set` lookups (:83-122).  Here
//   ranking   TopkHandle::rank_unseen (csrc/topk.hip): the training row of the user is excluded INSIDE the selection (binary search
//             in the row's ascending keys), so exactly topk slots per user are selected and sorted and nothing leaves the device;
//             full sweeps at d <= 128 take the fused path (the seen-aware instances of its kernels), whose lists are the dense path's;
//   metrics   eval_rank_metrics_kernel, one wave per user: membership of the list entries in the user's ground truth by binary
//             search in a device CSR of the vali pairs (sorted; duplicates count once -- the reference's set), hit / AP / DCG /
//             accuracy / AUC in float64 in the reference's operation order, one record of five doubles per user;
//   scores    eval_score_kernel, 16 lanes per vali triple: P[row] . Q[col] (+ Qb[col]) as an fp32 dot, |err| and err^2 as doubles;
//             its L2 instance ("score_func" = 1), 8 lanes per triple: 1 - |P[row] - Q[col]|^2 with numpy's bits (warp.py:147);
//   sums      eval_sum_kernel: ONE block adds the per-user records one after the other in index order -- the order, and so the bits,
//             of the reference's loop over the same per-user values.  That is wanted, not incidental: a blocked sum of the 138 K
//             AUC values of the ML-20M shape lands 1.3e-12 from the host loop's total (the loop's own rounding), past the 1e-12 the
//             scale test holds the means to; the cost of the chain is recorded in profiles/eval_first_contact.txt.  The per-triple
//             records of the score metrics (no such bound: the reference sums them in float32) go through fixed chunks of 2048
//             first (eval_chunk_sum_kernel).
// No float atomics anywhere: the doubles are the same bits run to run and for every batching of the ranking (the records are
// written by list position, the sum never sees the batches).
#include "abi.hpp"
#include "pairwise_sum.hpp"
#include "topk_engine.hpp"

namespace bfh {

constexpr int kEvalCols = 5;   // ndcg, ap, accuracy, auc, counted

__device__ __forceinline__ int eval_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// rec[b * 5 ..] = (ndcg, ap, accuracy, auc, 1) of the user rows[b] from its list lists[b * topk ..] (-1 = no entry), or five zeros
// for a user that is not counted: empty training row (base.py:86-87) or no ground truth.  grid: ceil(n / 4) blocks of 4 waves.
__global__ __launch_bounds__(256) void eval_rank_metrics_kernel(const int32_t* __restrict__ rows, int n, const int32_t* __restrict__ lists, int topk,
                                                                const int64_t* __restrict__ seen_indptr, const int64_t* __restrict__ gt_indptr,
                                                                const int32_t* __restrict__ gt_keys, int num_items, const double* __restrict__ dcgs,
                                                                const double* __restrict__ idcgs, double* __restrict__ rec) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= n) return;
    const int u = rows[b];
    const int64_t n_seen = seen_indptr[u] - (u > 0 ? seen_indptr[u - 1] : 0);
    const int64_t gbeg = u > 0 ? gt_indptr[u - 1] : 0, gend = gt_indptr[u];
    int distinct = 0;   // len(gt[row]): the run is sorted, a pair listed twice counts once
    for (int64_t i = gbeg + lane; i < gend; i += 64) distinct += (i == gbeg || gt_keys[i] != gt_keys[i - 1]) ? 1 : 0;
    const int n_pos = eval_wave_sum(distinct);
    double* out = rec + static_cast<size_t>(b) * kEvalCols;
    if (n_seen == 0 || n_pos == 0) {   // wave-uniform
        if (lane < kEvalCols) out[lane] = 0.0;
        return;
    }
    const int32_t* list = lists + static_cast<size_t>(b) * topk;
    const unsigned long long below = (1ull << lane) - 1ull;
    int hit = 0, miss = 0;
    long long auc_int = 0;   // sum of `hit` over the misses (base.py:113): integers, exact in any order
    double ap = 0.0, dcg = 0.0;
    for (int base = 0; base < topk; base += 64) {
        const int i = base + lane;
        const int32_t key = i < topk ? list[i] : -1;
        const bool valid = key >= 0;
        const bool member = valid && sorted_contains(gt_keys, gbeg, gend, key);
        const unsigned long long mm = __ballot(member), vm = __ballot(valid);
        auc_int += eval_wave_sum((valid && !member) ? hit + __popcll(mm & below) : 0);
        miss += __popcll(vm & ~mm);
        for (unsigned long long m = mm; m; m &= m - 1ull) {   // the hits in list order (every lane runs the same loop): base.py:107-110
            const int p = base + __builtin_ctzll(m);
            hit += 1;
            ap = __dadd_rn(ap, static_cast<double>(hit) / (p + 1.0));
            dcg = __dadd_rn(dcg, dcgs[p]);
        }
    }
    if (lane == 0) {
        const int n_neg = num_items - n_pos;
        double auc = static_cast<double>(auc_int);
        auc = __dadd_rn(auc, __dmul_rn((static_cast<double>(hit) + n_pos) / 2.0, static_cast<double>(n_neg - miss)));   // base.py:114
        auc /= static_cast<double>(static_cast<long long>(n_pos) * n_neg);                                            // base.py:115
        const int m = n_pos < topk ? n_pos : topk;
        out[0] = dcg / idcgs[m - 1];                                  // base.py:97,117
        out[1] = ap / static_cast<double>(m);                         // base.py:119
        out[2] = static_cast<double>(hit) / static_cast<double>(n_pos);   // base.py:93
        out[3] = auc;
        out[4] = 1.0;
    }
}

// rec[i * 2 ..] = (|err|, err^2) of vali triple i, err = (P[row] . Q[col] (+ Qb[col])) - val in fp32 (base.py:138-144: the scores and
// the values are float32 arrays), widened to double before it is squared.  16 lanes per triple: lane l takes columns l, l + 16, ...
// and the 16 partial sums meet in four DPP row rotations -- the same order for every triple.  grid: ceil(n / 16) blocks of 256.
// L2 (the WARP front's _get_scores under score_func "L2", warp.py:147): the prediction is fl(1.0f - dist), dist = the float32 bits of
// ((P[row] - Q[col]) ** 2).sum(-1) -- pairwise_row_sum over SqDiffOf, the function topk_sqdist_kernel reports distances with -- on 8
// lanes per triple; no bias.  grid: ceil(n / 32) blocks of 256.
template <bool L2>
__global__ __launch_bounds__(256) void eval_score_kernel(const float* __restrict__ P, const float* __restrict__ Q, const float* __restrict__ Qb, int d,
                                                         int ld, const int32_t* __restrict__ row, const int32_t* __restrict__ col,
                                                         const float* __restrict__ val, int64_t n, double* __restrict__ rec) {
    constexpr int G = L2 ? 8 : 16;   // lanes per triple
    const int64_t i = static_cast<int64_t>(blockIdx.x) * (256 / G) + (threadIdx.x / G);
    const int l = threadIdx.x & (G - 1);
    if (i >= n) return;   // whole G-lane rows leave together
    const float* p = P + static_cast<int64_t>(row[i]) * ld;
    const float* q = Q + static_cast<int64_t>(col[i]) * ld;
    float acc = 0.f;
    if constexpr (L2) {
        acc = 1.0f - pairwise_row_sum(SqDiffOf{p, q}, d, l);
    } else {
        for (int c = l; c < d; c += 16) acc = fmaf(p[c], q[c], acc);
        acc += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, acc), 0x128, 0xf, 0xf, false));   // row_ror:8
        acc += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, acc), 0x124, 0xf, 0xf, false));   // row_ror:4
        acc += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, acc), 0x122, 0xf, 0xf, false));   // row_ror:2
        acc += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, acc), 0x121, 0xf, 0xf, false));   // row_ror:1
    }
    if (l == 0) {
        if (!L2 && Qb) acc += Qb[col[i]];
        const double err = static_cast<double>(acc - val[i]);
        rec[i * 2] = fabs(err);
        rec[i * 2 + 1] = __dmul_rn(err, err);
    }
}

// out[c] = sum_i rec[i * C + c], C <= 8, added ONE RECORD AFTER THE OTHER in index order -- the order of the reference's Python loop
// (base.py:83-122), so the totals are the bits that loop produces from the same per-user values, whatever the batching was.  One
// block: its 512 threads stage 1024 records at a time in LDS (coalesced), then lane 0 of wave c runs column c's chain (up to 8
// independent chains side by side).  The cost is linear in n, one dependent fp64 add per record and chain (measured:
// profiles/eval_first_contact.txt), which is why only the per-USER records take this kernel directly.
constexpr int kSumChunk = 1024;
__global__ __launch_bounds__(512) void eval_sum_kernel(const double* __restrict__ rec, int64_t n, int C, double* __restrict__ out) {
    __shared__ double stage[kSumChunk * 8];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double s = 0.0;
    for (int64_t base = 0; base < n; base += kSumChunk) {
        const int m = static_cast<int>(n - base < kSumChunk ? n - base : kSumChunk);
        for (int i = threadIdx.x; i < m * C; i += 512) stage[i] = rec[base * C + i];
        __syncthreads();
        if (lane == 0 && wv < C) {
            int i = 0;
            for (; i + 8 <= m; i += 8) {   // eight LDS reads in flight ahead of the chain; the order of the adds is unchanged
                double v[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = stage[(i + k) * C + wv];
#pragma unroll
                for (int k = 0; k < 8; ++k) s = __dadd_rn(s, v[k]);
            }
            for (; i < m; ++i) s = __dadd_rn(s, stage[i * C + wv]);
        }
        __syncthreads();
    }
    if (lane == 0 && wv < C) out[wv] = s;
}

// part[g * C + c] = sum of column c over the records [g * 2048, (g + 1) * 2048): thread t adds records t, t + 256, ... of the chunk in
// that order, the 256 partial sums meet in a binary LDS tree.  The shape depends on n alone; eval_sum_kernel then adds the chunk sums
// in chunk order.  grid: ceil(n / 2048) blocks of 256, C <= 8.
constexpr int kChunkRecords = 2048;
__global__ __launch_bounds__(256) void eval_chunk_sum_kernel(const double* __restrict__ rec, int64_t n, int C, double* __restrict__ part) {
    __shared__ double tree[256];
    const int64_t beg = static_cast<int64_t>(blockIdx.x) * kChunkRecords;
    const int64_t end = beg + kChunkRecords < n ? beg + kChunkRecords : n;
    for (int c = 0; c < C; ++c) {
        double s = 0.0;
        for (int64_t i = beg + threadIdx.x; i < end; i += 256) s = __dadd_rn(s, rec[i * C + c]);
        tree[threadIdx.x] = s;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if (static_cast<int>(threadIdx.x) < w) tree[threadIdx.x] = __dadd_rn(tree[threadIdx.x], tree[threadIdx.x + w]);
            __syncthreads();
        }
        if (threadIdx.x == 0) part[static_cast<int64_t>(blockIdx.x) * C + c] = tree[0];
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------
class EvalHandle : public HandleBase {
 public:
    ~EvalHandle() override {
        delete engine_;
        if (stream) (void)hipStreamDestroy(stream);
    }
    bool placed() const override { return stream || engine_; }   // the ranking engine lives on the device of first use as well
    void ensure() {
        BFH_HIP(hipSetDevice(device));
        if (!stream) BFH_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        if (!engine_) {
            engine_ = topk_engine_new(device);
            engine_->timing = timing;
            topk_engine_set_mode(engine_, "fused", fused_);
            topk_engine_set_mode(engine_, "score_func", l2_ ? 1 : 0);
        }
    }

    void set_data(int num_users, int num_items, const int64_t* seen_indptr, const int32_t* seen_keys, int64_t nnz, const int32_t* vali_row,
                  const int32_t* vali_col, const float* vali_val, int64_t n_vali) {
        BFH_REQUIRE(num_users > 0 && num_items > 0, "set_data: empty shape");
        BFH_REQUIRE(nnz >= 0 && n_vali >= 0, "set_data: negative count");
        BFH_REQUIRE(n_vali == 0 || (vali_row && vali_col && vali_val), "set_data: null vali arrays");
        validate_seen_csr("set_data", num_users, num_items, seen_indptr, seen_keys, nnz);
        std::vector<uint8_t> has(static_cast<size_t>(num_users), 0);
        for (int64_t i = 0; i < n_vali; ++i) {
            if (vali_row[i] < 0 || vali_row[i] >= num_users) throw Error(BFH_ERR_INVALID, "set_data: vali row outside [0, num_users) at entry " + std::to_string(i));
            if (vali_col[i] < 0 || vali_col[i] >= num_items) throw Error(BFH_ERR_INVALID, "set_data: vali col outside [0, num_items) at entry " + std::to_string(i));
            has[vali_row[i]] = 1;
        }
        ensure();
        all_rows_.clear();
        for (int u = 0; u < num_users; ++u)
            if (has[u]) all_rows_.push_back(u);
        num_users_ = num_users; num_items_ = num_items; nnz_ = nnz; n_vali_ = n_vali;
        const int slot = t_aux_.begin(stream);
        seen_indptr_.resize(num_users);
        seen_keys_.resize(std::max<int64_t>(nnz, 1));
        BFH_HIP(hipMemcpyAsync(seen_indptr_.get(), seen_indptr, sizeof(int64_t) * num_users, hipMemcpyHostToDevice, stream));
        if (nnz) BFH_HIP(hipMemcpyAsync(seen_keys_.get(), seen_keys, sizeof(int32_t) * nnz, hipMemcpyHostToDevice, stream));
        gt_indptr_.resize(num_users);
        d_all_rows_.resize(std::max<size_t>(all_rows_.size(), 1));
        if (n_vali == 0) {
            BFH_HIP(hipMemsetAsync(gt_indptr_.get(), 0, sizeof(int64_t) * num_users, stream));
        } else {
            vali_row_.resize(n_vali); vali_col_.resize(n_vali); vali_val_.resize(n_vali); gt_keys_.resize(n_vali); sort_vals_.resize(n_vali);
            BFH_HIP(hipMemcpyAsync(vali_row_.get(), vali_row, sizeof(int32_t) * n_vali, hipMemcpyHostToDevice, stream));
            BFH_HIP(hipMemcpyAsync(vali_col_.get(), vali_col, sizeof(int32_t) * n_vali, hipMemcpyHostToDevice, stream));
            BFH_HIP(hipMemcpyAsync(vali_val_.get(), vali_val, sizeof(float) * n_vali, hipMemcpyHostToDevice, stream));
            BFH_HIP(hipMemcpyAsync(gt_keys_.get(), vali_col_.get(), sizeof(int32_t) * n_vali, hipMemcpyDeviceToDevice, stream));
            BFH_HIP(hipMemcpyAsync(d_all_rows_.get(), all_rows_.data(), sizeof(int32_t) * all_rows_.size(), hipMemcpyHostToDevice, stream));
            // ground truth as compressed rows: (row, col) sorted on the device, duplicates kept (the metrics kernel counts a pair once)
            csr_from_device_coo(vali_row_.get(), gt_keys_.get(), vali_val_.get(), sort_vals_.get(), n_vali, num_users, gt_indptr_.get(), sort_kin_,
                                sort_kout_, sort_tmp_, stream);
        }
        t_aux_.end(slot, stream);
        BFH_HIP(hipStreamSynchronize(stream));
        stats.h2d_bytes += 8.0 * num_users + 4.0 * nnz + 12.0 * n_vali + 4.0 * all_rows_.size();
        stats.aux_ms += t_aux_.drain();
        bound_ = true;
    }

    int num_rows() const { return static_cast<int>(all_rows_.size()); }

    // factor matrices of the host forms -> HBM, zero-padded to ld = ceil(d / 8) * 8 (what bfh_topk_dot_topn does with them)
    struct Factors {
        const float *P, *Q, *Qb;
        int d, ld;
    };
    Factors upload(const float* P, int p_rows, int p_cols, const float* Q, int q_rows, int q_cols, const float* Qb, int qb_rows) {
        BFH_REQUIRE(P && Q && p_cols > 0, "null or empty factor matrix");
        BFH_REQUIRE(p_cols == q_cols, "P and Q must have the same number of columns");
        BFH_REQUIRE(qb_rows == 0 || (qb_rows == q_rows && Qb), "Qb must have one row per row of Q");
        refuse_bias(qb_rows);
        check_shapes(p_rows, q_rows);
        ensure();
        const int d = p_cols, ld = (d + 7) / 8 * 8;
        upload_padded(hP_, P, p_rows, d, ld, stream);
        upload_padded(hQ_, Q, q_rows, d, ld, stream);
        if (qb_rows) {
            hQb_.resize(std::max(hQb_.size(), static_cast<size_t>(q_rows)));
            BFH_HIP(hipMemcpyAsync(hQb_.get(), Qb, static_cast<size_t>(q_rows) * 4, hipMemcpyHostToDevice, stream));
        }
        BFH_HIP(hipStreamSynchronize(stream));
        stats.h2d_bytes += 4.0 * (static_cast<double>(p_rows) * d + static_cast<double>(q_rows) * d + (qb_rows ? q_rows : 0));
        return Factors{hP_.get(), hQ_.get(), qb_rows ? hQb_.get() : nullptr, d, ld};
    }
    void check_shapes(int p_rows, int q_rows) const {
        BFH_REQUIRE(bound_, "set_data has not been called");
        BFH_REQUIRE(p_rows == num_users_, "P must have one row per user of set_data");
        BFH_REQUIRE(q_rows == num_items_, "Q must have one row per item of set_data");
    }
    void check_device(const float* dP, const float* dQ, int p_rows, int q_rows, int d, int ld, const float* dQb, int qb_rows) const {
        check_shapes(p_rows, q_rows);
        BFH_REQUIRE(dP && dQ, "null device factor matrix");
        BFH_REQUIRE(d > 0 && ld % 8 == 0 && d <= ld, "factor matrices need a leading dimension that is a multiple of 8 and >= d");
        BFH_REQUIRE(qb_rows == 0 || (qb_rows == q_rows && dQb), "Qb must have one row per row of Q");
        refuse_bias(qb_rows);
    }
    void refuse_bias(int qb_rows) const {
        BFH_REQUIRE(!l2_ || qb_rows == 0, "score_func = l2: the L2 score has no item bias (qb_rows must be 0)");
    }

    // evaluate/base.py:44-128 over `rows` (NULL: every user with vali entries, ascending)
    void ranking(const Factors& f, const int32_t* rows, int n_rows, int topk, double* out, int32_t* out_keys) {
        BFH_REQUIRE(out, "null output");
        BFH_REQUIRE(topk > 0 && topk <= 16384, "topk must be in [1, 16384]");
        ensure();
        const int32_t* d_rows = d_all_rows_.get();
        int n = num_rows();
        if (rows) {
            BFH_REQUIRE(n_rows >= 0, "negative number of rows");
            for (int i = 0; i < n_rows; ++i)
                if (rows[i] < 0 || rows[i] >= num_users_) throw Error(BFH_ERR_INVALID, "row outside [0, num_users) at position " + std::to_string(i));
            n = n_rows;
            d_rows_.resize(std::max<size_t>(d_rows_.size(), std::max(n, 1)));
            if (n) BFH_HIP(hipMemcpyAsync(d_rows_.get(), rows, sizeof(int32_t) * n, hipMemcpyHostToDevice, stream));
            stats.h2d_bytes += 4.0 * n;
            d_rows = d_rows_.get();
        }
        for (int c = 0; c < kEvalCols; ++c) out[c] = 0.0;
        if (n == 0) return;
        if (table_topk_ != topk) {   // dcgs | idcgs of base.py:68-69, float64 on the host: 1 / log2(i + 2) and its running sum
            std::vector<double> t(static_cast<size_t>(topk) * 2);
            double run = 0.0;
            for (int i = 0; i < topk; ++i) {
                t[i] = 1.0 / std::log2(static_cast<double>(i + 2));
                run += t[i];
                t[topk + i] = run;
            }
            table_.resize(std::max(table_.size(), t.size()));
            BFH_HIP(hipMemcpyAsync(table_.get(), t.data(), t.size() * 8, hipMemcpyHostToDevice, stream));
            BFH_HIP(hipStreamSynchronize(stream));   // t is a local
            table_topk_ = topk;
        }
        lists_.resize(std::max(lists_.size(), static_cast<size_t>(n) * topk));
        rec_.resize(std::max(rec_.size(), static_cast<size_t>(n) * kEvalCols));
        sums_.resize(8);
        BFH_HIP(hipStreamSynchronize(stream));   // the rows are up before the engine's stream reads them
        const double before = engine_->stats.kernel_ms + engine_->stats.aux_ms;
        const int64_t merges = engine_->stats.merges, exchanges = engine_->stats.exchanges;
        topk_engine_rank_unseen(engine_, d_rows, n, f.P, f.Q, num_items_, f.d, f.ld, f.Qb, seen_indptr_.get(), seen_keys_.get(), topk, lists_.get(),
                                batch_);
        stats.kernel_ms += engine_->stats.kernel_ms + engine_->stats.aux_ms - before;
        stats.merges += engine_->stats.merges - merges;         // rows the fused path handed back to the dense path
        stats.exchanges += engine_->stats.exchanges - exchanges;   // rows with ties at the last place (block-level list selection)
        const int slot = t_metrics_.begin(stream);
        hipLaunchKernelGGL(eval_rank_metrics_kernel, dim3((n + 3) / 4), dim3(256), 0, stream, d_rows, n, lists_.get(), topk, seen_indptr_.get(),
                           gt_indptr_.get(), gt_keys_.get(), num_items_, table_.get(), table_.get() + topk, rec_.get());
        BFH_HIP(hipGetLastError());
        hipLaunchKernelGGL(eval_sum_kernel, dim3(1), dim3(512), 0, stream, rec_.get(), static_cast<int64_t>(n), kEvalCols, sums_.get());
        BFH_HIP(hipGetLastError());
        t_metrics_.end(slot, stream);
        double s[kEvalCols];
        BFH_HIP(hipMemcpyAsync(s, sums_.get(), sizeof(s), hipMemcpyDeviceToHost, stream));
        if (out_keys) BFH_HIP(hipMemcpyAsync(out_keys, lists_.get(), sizeof(int32_t) * n * topk, hipMemcpyDeviceToHost, stream));
        BFH_HIP(hipStreamSynchronize(stream));
        stats.d2h_bytes += sizeof(s) + (out_keys ? 4.0 * n * topk : 0.0);
        stats.optimizer_ms += t_metrics_.drain();
        stats.launches += 1;
        stats.samples += static_cast<int64_t>(s[4]);
        if (s[4] > 0.0) {   // base.py:123-126
            for (int c = 0; c < 4; ++c) out[c] = s[c] / s[4];
            out[4] = s[4];
        }
    }

    // evaluate/base.py:130-148
    void scores(const Factors& f, double* out) {
        BFH_REQUIRE(out, "null output");
        ensure();
        out[0] = out[1] = 0.0;
        if (n_vali_ == 0) return;
        rec_.resize(std::max(rec_.size(), static_cast<size_t>(n_vali_) * 2));
        part_.resize(std::max(part_.size(), static_cast<size_t>((n_vali_ + kChunkRecords - 1) / kChunkRecords) * 2));
        sums_.resize(8);
        const int slot = t_aux_.begin(stream);
        const int per_block = l2_ ? 32 : 16;   // triples per block: eval_score_kernel's lanes per triple
        hipLaunchKernelGGL((l2_ ? eval_score_kernel<true> : eval_score_kernel<false>), dim3(static_cast<unsigned>((n_vali_ + per_block - 1) / per_block)),
                           dim3(256), 0, stream, f.P, f.Q, f.Qb, f.d, f.ld, vali_row_.get(), vali_col_.get(), vali_val_.get(), n_vali_, rec_.get());
        BFH_HIP(hipGetLastError());
        const int64_t n_chunks = (n_vali_ + kChunkRecords - 1) / kChunkRecords;
        hipLaunchKernelGGL(eval_chunk_sum_kernel, dim3(static_cast<unsigned>(n_chunks)), dim3(256), 0, stream, rec_.get(), n_vali_, 2, part_.get());
        BFH_HIP(hipGetLastError());
        hipLaunchKernelGGL(eval_sum_kernel, dim3(1), dim3(512), 0, stream, part_.get(), n_chunks, 2, sums_.get());
        BFH_HIP(hipGetLastError());
        t_aux_.end(slot, stream);
        double s[2];
        BFH_HIP(hipMemcpyAsync(s, sums_.get(), sizeof(s), hipMemcpyDeviceToHost, stream));
        BFH_HIP(hipStreamSynchronize(stream));
        stats.d2h_bytes += sizeof(s);
        stats.aux_ms += t_aux_.drain();
        out[0] = std::sqrt(s[1] / static_cast<double>(n_vali_));   // base.py:145-146
        out[1] = s[0] / static_cast<double>(n_vali_);              // base.py:147
    }

    void set_mode(const std::string& name, int64_t v) {
        if (name == "batch") {
            BFH_REQUIRE(v >= 0 && v <= (int64_t(1) << 30), "batch must be >= 0");
            batch_ = static_cast<int>(v);
        } else if (name == "timing") {
            timing = v != 0;
            if (engine_) engine_->timing = timing;
        } else if (name == "fused") {
            fused_ = static_cast<int>(v);
            if (engine_) topk_engine_set_mode(engine_, name, v);
        } else if (name == "score_func") {   // as bfh_topk_set_mode: the ranking key, and the prediction of `scores`
            BFH_REQUIRE(v == 0 || v == 1, "score_func must be 0 (dot) or 1 (l2)");
            l2_ = v == 1;
            if (engine_) topk_engine_set_mode(engine_, name, v);
        } else if (name == "fast_select" || name == "fused_c0" || name == "wave_select") {
            ensure();
            topk_engine_set_mode(engine_, name, v);
        } else {
            throw Error(BFH_ERR_INVALID, "unknown mode '" + name + "'");
        }
    }

 private:
    HandleBase* engine_ = nullptr;
    bool bound_ = false;
    int num_users_ = 0, num_items_ = 0, batch_ = 0, table_topk_ = 0;
    bool l2_ = false;  // "score_func" = 1: the ranking by squared distance, predictions 1 - distance
    int fused_ = -1;   // the engine's "fused" rule: -1 = by size (default, as bfh_topk_dot_topn), 0 = the dense path, 1 = whenever d <= 128
    int64_t nnz_ = 0, n_vali_ = 0;
    std::vector<int32_t> all_rows_;
    DevBuf<int64_t> seen_indptr_, gt_indptr_;
    DevBuf<int32_t> seen_keys_, gt_keys_, vali_row_, vali_col_, d_all_rows_, d_rows_, lists_;
    DevBuf<float> vali_val_, sort_vals_, hP_, hQ_, hQb_;
    DevBuf<uint64_t> sort_kin_, sort_kout_;
    DevBuf<char> sort_tmp_;
    DevBuf<double> rec_, part_, sums_, table_;
    EventTimer t_metrics_, t_aux_;
};

}  // namespace bfh

using bfh::EvalHandle;
using bfh::guarded;

extern "C" {

BFH_ABI_LIFECYCLE(eval, EvalHandle)

int bfh_eval_set_data(void* h, int num_users, int num_items, const int64_t* seen_indptr, const int32_t* seen_keys, int64_t nnz,
                      const int32_t* vali_row, const int32_t* vali_col, const float* vali_val, int64_t n_vali) {
    return guarded<EvalHandle>(h, [&](EvalHandle& e) {
        e.set_data(num_users, num_items, seen_indptr, seen_keys, nnz, vali_row, vali_col, vali_val, n_vali);
    });
}
int bfh_eval_num_rows(void* h) {
    return guarded<EvalHandle>(h, [&](EvalHandle& e) { return e.num_rows(); });
}
int bfh_eval_ranking(void* h, const float* P, int p_rows, int p_cols, const float* Q, int q_rows, int q_cols, const float* Qb, int qb_rows,
                     const int32_t* rows, int n_rows, int topk, double* out, int32_t* out_keys) {
    return guarded<EvalHandle>(h, [&](EvalHandle& e) {
        if (topk <= 0 || topk > 16384) throw bfh::Error(BFH_ERR_INVALID, "topk must be in [1, 16384]");
        e.ranking(e.upload(P, p_rows, p_cols, Q, q_rows, q_cols, Qb, qb_rows), rows, n_rows, topk, out, out_keys);
    });
}
int bfh_eval_ranking_device(void* h, const float* dP, int p_rows, const float* dQ, int q_rows, int d, int ld, const float* dQb, int qb_rows,
                            const int32_t* rows, int n_rows, int topk, double* out, int32_t* out_keys) {
    return guarded<EvalHandle>(h, [&](EvalHandle& e) {
        e.check_device(dP, dQ, p_rows, q_rows, d, ld, dQb, qb_rows);
        e.ranking(EvalHandle::Factors{dP, dQ, qb_rows ? dQb : nullptr, d, ld}, rows, n_rows, topk, out, out_keys);
    });
}
int bfh_eval_scores(void* h, const float* P, int p_rows, int p_cols, const float* Q, int q_rows, int q_cols, const float* Qb, int qb_rows,
                    double* out) {
    return guarded<EvalHandle>(h, [&](EvalHandle& e) {
        e.scores(e.upload(P, p_rows, p_cols, Q, q_rows, q_cols, Qb, qb_rows), out);
    });
}
int bfh_eval_scores_device(void* h, const float* dP, int p_rows, const float* dQ, int q_rows, int d, int ld, const float* dQb, int qb_rows,
                           double* out) {
    return guarded<EvalHandle>(h, [&](EvalHandle& e) {
        e.check_device(dP, dQ, p_rows, q_rows, d, ld, dQb, qb_rows);
        e.scores(EvalHandle::Factors{dP, dQ, qb_rows ? dQb : nullptr, d, ld}, out);
    });
}
int bfh_eval_set_mode(void* h, const char* name, int64_t value) {
    return guarded<EvalHandle>(h, [&](EvalHandle& e) { e.set_mode(name ? name : "", value); });
}

}  // extern "C"
