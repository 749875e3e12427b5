// BPRMF fold-in on gfx950: rows for histories that are not in the model, by SGD against the FIXED item side (bfh_bpr_fold_in; included by
// bpr.hip alone).  The rule is in include/buffalo_hip.h; per step of history b
//     dq = Q[pos] - Q[neg];  x = p . dq (+ Qb[pos] - Qb[neg]);  g = table cell of x;  p += lr_t * (g * dq - reg_u * p)
// Only p moves, so nothing is shared between rows: no atomics on the model, no replicas, no store before the row is done.
//
// Layout.  A lane group of G lanes (16 at vdim <= 64, 32 at <= 128, 64 at <= 256) owns one history; lane `lig` holds columns 4 lig .. 4 lig + 3 of
// the row in registers from the first step to the last and moves 16 bytes of every gathered row.  A wave carries 64 / G groups that run the same
// loop in lockstep, each on its own row: one trip of the loop is one step of every group, and a group whose row is finished stores it and takes
// the next row from a ticket counter (the rows are handed out longest first), so a wave does not wait for its longest row.
//
// The (pos, neg) sequence does not depend on p.  The group therefore draws a WINDOW of G upcoming steps with its lanes in parallel -- lane l
// draws step w0 + l, attempt 0, and a rejected lane redoes its own draw with the next attempt (membership: binary search in the row's sorted
// keys, held in LDS up to kFoldKeysPerLane * G keys, read from global memory beyond) -- and gathers the rows of the next kFoldDepth steps into a
// register ring (Q[pos], Q[neg], the two biases).  What is left serial per step is: subtract -> 4 FMAs -> group sum -> table cell (LDS) -> update.
//
// The float32 order of a step (fixed, so a row's bits depend on its history, its row id and the model alone):
//     dq_k   = Q[pos, k] - Q[neg, k]                                   (columns >= d: 0)
//     part_l = fma(p3, dq3, fma(p2, dq2, fma(p1, dq1, p0 * dq0)))      (lane l, columns 4 l .. 4 l + 3)
//     x      = fold_group_sum(part): within a row of 16 lanes  part += ror 8;  += ror 4;  += ror 2;  += ror 1  (every lane adds the lane 8, 4, 2, 1
//              above it, cyclically); G = 32: + the other row of 16; G = 64: (row0 + row1) + (row2 + row3).  Every lane of the group ends with the same bits.
//     x     += Qb[pos] - Qb[neg]                                       (use_bias)
//     p_k    = p_k + lr_t * (g * dq_k - reg_u * p_k)                   every product and sum rounded on its own (no contraction)
#pragma once
#include "bpr_kernels.hpp"
#include "fold_group.hpp"

namespace bfh {

constexpr int kFoldDepth = 3;         // steps whose rows are in flight or in registers ahead of the one being taken
constexpr int kFoldKeysPerLane = 8;   // a row of up to kFoldKeysPerLane * G keys keeps them in LDS
constexpr uint32_t kFoldStream = 5;   // counter_draw stream id of the fold-in negatives
constexpr uint32_t kFoldMaxAttempts = 1u << 20;   // the trainer's cap (bpr_sample_negative): the host has refused rows that leave nothing to draw

static inline int64_t fold_lds_keys(int vdim) { return static_cast<int64_t>(kFoldKeysPerLane) * fold_group_of(vdim); }

struct BprFoldRow {   // one history, in the order the groups take them
    int64_t beg;      // first key
    int32_t n;        // keys
    int32_t out_row;  // position in the call: row of init / out
    uint32_t row_id;  // r_b of the draw counter
    uint32_t steps;   // iters * n * num_neg
};

struct BprFoldArgs {
    const float* Q;            // [Q_rows, vdim]
    const float* Qb;           // [Q_rows]
    const float* init;         // [n_rows, vdim] or nullptr: zeros
    float* out;                // [n_rows, vdim]; columns >= d are written 0
    float* dense;              // [n_rows, d] or nullptr: the same rows unpadded, what goes back to the caller in ONE copy
    const int32_t* keys;       // the call's keys
    const BprFoldRow* rows;    // [n_rows]
    const float* lr;           // [iters]: lr_t
    const float* exp_table;    // [1000]
    const int64_t* cum_table;  // [Q_rows] (sampling_power != 0)
    int64_t cum_total;
    int* ticket;               // next row to hand out (0 at launch)
    int n_rows, Q_rows, d, vdim, iters, num_neg, use_bias, verify_neg, uniform;
    float reg_u;
    uint32_t seed;
};

// the candidate of one attempt: the trainer's rule (bpr_draw_candidate) on stream kFoldStream
__device__ __forceinline__ int fold_candidate(const BprFoldArgs& a, uint64_t pos_idx, uint32_t slot, uint32_t epoch, uint32_t attempt) {
    uint32_t o0, o1;
    counter_draw(a.seed, kFoldStream, pos_idx, slot, epoch, attempt, o0, o1);
    if (a.uniform) return static_cast<int>((static_cast<uint64_t>(o0) * static_cast<uint32_t>(a.Q_rows)) >> 32);
    const uint64_t r64 = (static_cast<uint64_t>(o1) << 32) | o0;
    const int64_t r = static_cast<int64_t>(__umul64hi(r64, static_cast<uint64_t>(a.cum_total)));
    const int idx = static_cast<int>(lower_bound_dev<int64_t>(a.cum_table, a.Q_rows, r));
    return idx < a.Q_rows ? idx : a.Q_rows - 1;   // r < cum_total = the last entry: never taken on a table that ascends
}

struct FoldSlot {   // one step's gathered operands
    float4 qp, qn;
    float bp, bn;
};

template <int G>
__global__ __launch_bounds__(256) void bpr_fold_kernel(const BprFoldArgs a) {
#pragma clang fp contract(off)   // the order above is the contract; fused operations are written out
    constexpr int NG = 64 / G;
    constexpr int D = kFoldDepth;
    constexpr int KEYS = kFoldKeysPerLane * G;
    __shared__ float s_table[1000];
    __shared__ int32_t s_keys[4 * 64 * kFoldKeysPerLane];
    for (int i = threadIdx.x; i < 1000; i += 256) s_table[i] = a.exp_table[i];
    __syncthreads();

    const int lane = threadIdx.x & 63, lig = lane & (G - 1), grp0 = lane & ~(G - 1);
    int32_t* my_keys = s_keys + ((threadIdx.x >> 6) * NG + lane / G) * KEYS;
    const int col = lig * 4;
    const bool in_row = col < a.vdim;
    const bool valid[4] = {col < a.d, col + 1 < a.d, col + 2 < a.d, col + 3 < a.d};

    // the group's row (group-uniform values in every lane)
    bool has_row = false, in_lds = false, done = false;   // done: the counter had no row left for this group
    BprFoldRow row{0, 0, 0, 0u, 0u};
    const int32_t* gkeys = a.keys;
    uint32_t per_iter = 1;      // steps of one iteration: n * num_neg
    uint32_t s_exec = 0;        // the step to take next
    uint32_t left = 0;          // steps until lr_t changes
    int t_next = 0;             // index of lr_nxt
    float lr_cur = 0.f, lr_nxt = 0.f;
    uint32_t w0 = 0;            // the window holds steps [w0, w0 + G): lane lig has drawn step w0 + lig
    int w_pos = 0, w_neg = 0;
    float p[4] = {0.f, 0.f, 0.f, 0.f};
    FoldSlot ring[D];
#pragma unroll
    for (int k = 0; k < D; ++k) ring[k] = FoldSlot{make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f), 0.f, 0.f};

    // lane lig draws step w0 + lig of the row: its positive and the first accepted negative
    auto draw_window = [&](uint32_t first) {
        w0 = first;
        const uint32_t s = first + static_cast<uint32_t>(lig);
        w_pos = 0;
        w_neg = 0;
        if (s < row.steps) {
            const uint32_t t = s / per_iter, rem = s - t * per_iter;
            const uint32_t j = rem / static_cast<uint32_t>(a.num_neg), slot = rem - j * static_cast<uint32_t>(a.num_neg);
            w_pos = in_lds ? my_keys[j] : gkeys[j];
            const uint64_t pos_idx = (static_cast<uint64_t>(row.row_id) << 32) | j;
            for (uint32_t attempt = 0; attempt < kFoldMaxAttempts; ++attempt) {
                w_neg = fold_candidate(a, pos_idx, slot, t, attempt);
                if (!a.verify_neg || !fold_contains(my_keys, gkeys, in_lds, row.n, w_neg)) break;
            }
        }
    };
    // the operands of step s into `slot` (nothing past the row's last step)
    auto issue = [&](FoldSlot& slot, uint32_t s) {
        if (s >= row.steps) return;             // group-uniform
        if (s >= w0 + G) draw_window(s);        // steps are issued in order: s == w0 + G
        const int src = grp0 + static_cast<int>(s - w0);
        const int pos = __shfl(w_pos, src, 64), neg = __shfl(w_neg, src, 64);
        if (in_row) {
            slot.qp = *reinterpret_cast<const float4*>(a.Q + static_cast<size_t>(pos) * a.vdim + col);
            slot.qn = *reinterpret_cast<const float4*>(a.Q + static_cast<size_t>(neg) * a.vdim + col);
        }
        if (a.use_bias) {
            slot.bp = a.Qb[pos];
            slot.bn = a.Qb[neg];
        }
    };
    auto store_row = [&]() {
        if (in_row)
            *reinterpret_cast<float4*>(a.out + static_cast<size_t>(row.out_row) * a.vdim + col) =
                make_float4(valid[0] ? p[0] : 0.f, valid[1] ? p[1] : 0.f, valid[2] ? p[2] : 0.f, valid[3] ? p[3] : 0.f);
        if (a.dense) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (valid[e]) a.dense[static_cast<size_t>(row.out_row) * a.d + col + e] = p[e];
        }
    };

    for (;;) {
#pragma unroll
        for (int k = 0; k < D; ++k) {   // unrolled: the ring slot of a trip is a compile-time index
            if (!done && (!has_row || s_exec >= row.steps)) {
                // ---- the group's row is done (or it has none yet): store it, take the next ----
                if (has_row) store_row();
                int idx = 0;
                if (lig == 0) idx = atomicAdd(a.ticket, 1);
                idx = __shfl(idx, grp0, 64);
                has_row = idx < a.n_rows;
                done = !has_row;
                if (has_row) {
                    row = a.rows[idx];
                    gkeys = a.keys + row.beg;
                    in_lds = row.n <= KEYS;
                    per_iter = static_cast<uint32_t>(row.n) * static_cast<uint32_t>(a.num_neg);
                    if (in_lds) {
                        wave_lds_sync();   // the searches of the previous row are done before its keys go
                        for (int i = lig; i < row.n; i += G) my_keys[i] = gkeys[i];
                        wave_lds_sync();
                    }
                    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (a.init && in_row) o = *reinterpret_cast<const float4*>(a.init + static_cast<size_t>(row.out_row) * a.vdim + col);
                    p[0] = valid[0] ? o.x : 0.f; p[1] = valid[1] ? o.y : 0.f; p[2] = valid[2] ? o.z : 0.f; p[3] = valid[3] ? o.w : 0.f;
                    s_exec = 0;
                    left = per_iter;
                    lr_cur = a.lr[0];
                    t_next = a.iters > 1 ? 1 : 0;
                    lr_nxt = a.lr[t_next];
                    if (row.steps > 0) {
                        draw_window(0);
#pragma unroll
                        for (int i = 0; i < D; ++i) issue(ring[(k + i) % D], static_cast<uint32_t>(i));
                    }
                }
            }
            if (has_row && s_exec < row.steps) {
                // ---- one step: the serial chain ----
                const FoldSlot& sl = ring[k];
                const float dq[4] = {valid[0] ? sl.qp.x - sl.qn.x : 0.f, valid[1] ? sl.qp.y - sl.qn.y : 0.f, valid[2] ? sl.qp.z - sl.qn.z : 0.f,
                                     valid[3] ? sl.qp.w - sl.qn.w : 0.f};
                const float part = __builtin_fmaf(p[3], dq[3], __builtin_fmaf(p[2], dq[2], __builtin_fmaf(p[1], dq[1], p[0] * dq[0])));
                float x = fold_group_sum<G>(part);
                if (a.use_bias) x += sl.bp - sl.bn;
                float g;   // bpr_logit's cells (bpr.cc:124-131), the table read from LDS
                if (6.0f < x) g = 0.0f;
                else if (x < -6.0f) g = 1.0f;
                else {
                    const int cell = static_cast<int>((x + 6.0f) * 83.0f);
                    g = s_table[cell < 0 ? 0 : cell > 999 ? 999 : cell];
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) p[e] = p[e] + lr_cur * (g * dq[e] - a.reg_u * p[e]);
                ++s_exec;
                if (--left == 0) {   // the next iteration's rate; the one after it is fetched now
                    left = per_iter;
                    lr_cur = lr_nxt;
                    t_next = t_next + 1 < a.iters ? t_next + 1 : t_next;
                    lr_nxt = a.lr[t_next];
                }
                issue(ring[k], s_exec + D - 1);   // refill the slot with the step D - 1 behind the next one
            }
            if (__builtin_amdgcn_ballot_w64(!done) == 0) return;   // every group of the wave has found the counter exhausted
        }
    }
}

}  // namespace bfh
