// WARP fold-in on gfx950: rows for histories that are not in the model, by the trainer's trial loop against the FIXED item side
// (bfh_warp_fold_in; included by warp.hip alone).  The rule is in include/buffalo_hip.h.  Inside one pass p is frozen: the positives of a
// history run their trial loops independently, their gradients are summed, one optimizer step and one projection follow.  The serial chain
// of a history is therefore `iters` long, and the work inside a pass is parallel -- unlike BPRMF's fold-in, where every step moves p.
//
// Work split.  One block of 256 threads owns one history for all its passes; blocks take histories longest first from a ticket counter.
// A lane group of G lanes (16 at vdim <= 64, 32 at <= 128, 64 at <= 256; lane l holds columns 4 l .. 4 l + 3) takes one positive at a time
// and runs its whole trial loop by itself; the block runs NGB = 4 * 64 / G positives at once, positive j on group j mod NGB.  Every group
// holds its own register copy of p, of the optimizer state and of the pass's gradient sum, so that after the reduction every group takes
// the same step redundantly and nothing of a row travels between passes.  The barriers are block-uniform: two around the ticket and the
// key staging of a history, one per pass after the groups have written their gradient sums (the sums are double-buffered by pass parity).
//
// Trial loop of a group: G candidates per window, one attempt per lane; membership by binary search in the row's sorted keys (in LDS up to
// kWarpFoldLdsKeys keys, staged once per history; read from global memory beyond); a ballot of the unseen ones, masked to the group's
// lanes; they are scored in draw order with the trainer's 1 / 2 / 4 speculation (kWarpSpec): up to four candidate rows loaded as one float4
// per lane each, their partial scores group-summed, then decided one after another -- the trial counter is the reference's whatever was
// speculated.
//
// The float32 order (fixed, so a row's bits are a function of its keys, its row id, init, the options and Q alone):
//     part_l  = fma(a3, b3, fma(a2, b2, fma(a1, b1, a0 * b0)))      dot: a = p, b = q;  l2: a = b = p - q, and the part is negated
//     score   = fold_group_sum(part)                                (fold_group.hpp; every lane of the group receives the same bits)
//     term_k  = (Phi * (qi_k - qj_k)) - reg_u * p_k                 l2: ((Phi * 2) * (qi_k - qj_k)) - reg_u * p_k
//     a group adds the terms of its accepted positives into its accumulator in ascending j;
//     the NGB accumulators a_0 .. a_(NGB-1) are summed through LDS by the tree  a_i += a_(i+s)  for s = 1, 2, 4 .. (i a multiple of 2 s),
//     by every lane for its own columns;  then opt_step4 (sgd_opt_step.hpp), nrm = fold_group_sum(sum of the lane's p_k^2), p_k /= max(1, sqrt(nrm)).
// No matrix instructions: every history has its own p and its own candidates -- a gather plus matrix-vector products without operand reuse.
#pragma once
#include "warp_kernels.hpp"
#include "fold_group.hpp"
#include "sgd_opt_step.hpp"

namespace bfh {

constexpr int kWarpFoldLdsKeys = 8192;      // a history of up to this many keys keeps them in LDS (32 KB)
constexpr uint32_t kWarpFoldStream = 6;     // counter_draw stream id of the fold-in candidates

struct WarpFoldRow {   // one history, in the order the blocks take them
    int64_t beg;       // first key
    int32_t n;         // keys
    int32_t out_row;   // position in the call: row of init / out / counts
    uint32_t row_id;   // r_b of the draw counter
    uint32_t pad;
};

struct WarpFoldArgs {
    const float* Q;              // [Q_rows, vdim]
    const float* init;           // [n_rows, vdim] or nullptr: zeros
    float* out;                  // [n_rows, vdim]; columns >= d are written 0
    float* dense;                // [n_rows, d] or nullptr: the same rows unpadded, what goes back to the caller in ONE copy
    const int32_t* keys;         // the call's keys
    const WarpFoldRow* rows;     // [n_rows]
    const OptConsts* steps;      // [iters]: the optimizer's constants at iteration count t
    int* ticket;                 // next history to hand out (0 at launch)
    unsigned long long* counts;  // [2 * n_rows] or nullptr: scored negatives, accepted positives (0 at launch)
    int n_rows, Q_rows, d, vdim, iters, max_trial, l2, pcn;
    float reg_u;
    double threshold;
    uint32_t seed;
};

// the lane's part of a score (the fma chain of the header comment); q is zero in the columns >= d
__device__ __forceinline__ float warp_fold_part(const float (&p)[4], const float (&q)[4], bool l2) {
#pragma clang fp contract(off)
    if (!l2) return __builtin_fmaf(p[3], q[3], __builtin_fmaf(p[2], q[2], __builtin_fmaf(p[1], q[1], p[0] * q[0])));
    const float df[4] = {p[0] - q[0], p[1] - q[1], p[2] - q[2], p[3] - q[3]};
    return -__builtin_fmaf(df[3], df[3], __builtin_fmaf(df[2], df[2], __builtin_fmaf(df[1], df[1], df[0] * df[0])));
}

template <int G, bool ADAM>
__global__ __launch_bounds__(256) void warp_fold_kernel(const WarpFoldArgs a) {
#pragma clang fp contract(off)   // the order above is the contract; fused operations are written out
    constexpr int NGB = 4 * 64 / G;
    __shared__ int32_t s_keys[kWarpFoldLdsKeys];
    __shared__ float4 s_acc[2][NGB][G];   // the groups' gradient sums of a pass, by pass parity
    __shared__ int s_cnt[2][NGB];         // ... and their accepted positives
    __shared__ int s_idx;

    const int lane = threadIdx.x & 63, lig = lane & (G - 1), grp0 = lane & ~(G - 1);
    const int grp = threadIdx.x / G;      // group of the block: 0 .. NGB - 1
    const int col = lig * 4;
    const bool in_row = col < a.vdim;
    const bool valid[4] = {col < a.d, col + 1 < a.d, col + 2 < a.d, col + 3 < a.d};
    const bool l2 = a.l2 != 0;
    const unsigned long long gmask = G == 64 ? ~0ull : ((1ull << G) - 1ull);

    // a row of Q as the lane's four columns, zero beyond d
    auto load_q = [&](float (&q)[4], int item) {
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (in_row) o = *reinterpret_cast<const float4*>(a.Q + static_cast<size_t>(item) * a.vdim + col);
        q[0] = valid[0] ? o.x : 0.f; q[1] = valid[1] ? o.y : 0.f; q[2] = valid[2] ? o.z : 0.f; q[3] = valid[3] ? o.w : 0.f;
    };

    for (;;) {
        // ---- the block's next history ----
        if (threadIdx.x == 0) s_idx = atomicAdd(a.ticket, 1);
        __syncthreads();
        const int idx = s_idx;
        if (idx >= a.n_rows) break;   // block-uniform
        const WarpFoldRow row = a.rows[idx];
        const int32_t* gkeys = a.keys + row.beg;
        const bool in_lds = row.n <= kWarpFoldLdsKeys;
        if (in_lds)
            for (int i = threadIdx.x; i < row.n; i += 256) s_keys[i] = gkeys[i];
        __syncthreads();              // the keys are staged; every thread has read s_idx

        float p[4] = {0.f, 0.f, 0.f, 0.f};
        if (a.init && in_row) {
            const float4 o = *reinterpret_cast<const float4*>(a.init + static_cast<size_t>(row.out_row) * a.vdim + col);
            p[0] = valid[0] ? o.x : 0.f; p[1] = valid[1] ? o.y : 0.f; p[2] = valid[2] ? o.z : 0.f; p[3] = valid[3] ? o.w : 0.f;
        }
        float4 mom = make_float4(0.f, 0.f, 0.f, 0.f), vel = mom;
        unsigned long long scored = 0, accepted = 0;   // of this group's positives, over the passes

        const int passes = row.n > 0 ? a.iters : 0;    // a history without keys keeps its start row
        for (int t = 0; t < passes; ++t) {
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            int cnt = 0;
            for (int j = grp; j < row.n; j += NGB) {
                // ---- the trial loop of positive j (warp.cc:133-147): group-uniform control flow ----
                const int pos = in_lds ? s_keys[j] : gkeys[j];
                float qi[4], qj[4] = {0.f, 0.f, 0.f, 0.f};
                load_q(qi, pos);
                const float ui = fold_group_sum<G>(warp_fold_part(p, qi, l2));
                const uint64_t pos_idx = (static_cast<uint64_t>(row.row_id) << 32) | static_cast<uint32_t>(j);
                int kcount = 0, bsz = 1;          // counted candidates scored so far; rows the next step scores: 1, 2, 4, 4 ...
                bool found = false, done = false;
                for (uint32_t a0 = 0; a0 < kWarpAttemptCap && !done; a0 += G) {
                    uint32_t o0, o1;
                    counter_draw(a.seed, kWarpFoldStream, pos_idx, 0u, static_cast<uint32_t>(t), a0 + lig, o0, o1);
                    const int cand = static_cast<int>((static_cast<uint64_t>(o0) * static_cast<uint32_t>(a.Q_rows)) >> 32);
                    const bool seen = fold_contains(s_keys, gkeys, in_lds, row.n, cand);
                    unsigned long long unseen = (__ballot(!seen) >> grp0) & gmask;
                    while (unseen != 0ull && !done) {
                        int cl[kWarpSpec];
                        int nb = 0;
#pragma unroll
                        for (int s = 0; s < kWarpSpec; ++s) {
                            cl[s] = 0;
                            if (s < bsz && unseen != 0ull) {
                                const int l = __builtin_ctzll(unseen);
                                unseen &= unseen - 1ull;
                                if constexpr (G == 64) cl[s] = __builtin_amdgcn_readlane(cand, l);
                                else cl[s] = __shfl(cand, grp0 + l, 64);
                                nb = s + 1;
                            }
                        }
                        float cr[kWarpSpec][4], sc[kWarpSpec];
#pragma unroll
                        for (int s = 0; s < kWarpSpec; ++s)
                            if (s < nb) load_q(cr[s], cl[s]);
#pragma unroll
                        for (int s = 0; s < kWarpSpec; ++s)
                            if (s < nb) sc[s] = fold_group_sum<G>(warp_fold_part(p, cr[s], l2));
#pragma unroll
                        for (int s = 0; s < kWarpSpec; ++s) {
                            if (s < nb && !done) {
                                if (1 + 2 * kcount > a.max_trial) {   // `while (trial <= max_trial)` fails
                                    done = true;
                                } else {
                                    kcount += 1;
                                    scored += 1;
                                    if (static_cast<double>(ui - sc[s]) < a.threshold) {
                                        found = true;
                                        done = true;
#pragma unroll
                                        for (int e = 0; e < 4; ++e) qj[e] = cr[s][e];
                                    }
                                }
                            }
                        }
                        if (bsz < kWarpSpec) bsz <<= 1;
                    }
                    if (!done && 1 + 2 * kcount > a.max_trial) done = true;
                }
                const int trial = 2 * kcount;
                if (!found || trial >= a.max_trial) continue;   // warp.cc:148-149
                const float Phi = warp_phi(a.Q_rows, row.n, trial);
                const float w = l2 ? Phi * 2 : Phi;             // warp.cc:30-52
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float ud = w * (qi[e] - qj[e]);
                    const float rp = a.reg_u * p[e];
                    acc[e] = acc[e] + (ud - rp);
                }
                cnt += 1;
                accepted += 1;
            }
            // ---- the NGB sums through LDS, the same tree in every lane ----
            const int par = t & 1;
            s_acc[par][grp][lig] = make_float4(acc[0], acc[1], acc[2], acc[3]);
            if (lig == 0) s_cnt[par][grp] = cnt;
            __syncthreads();
            float4 part[NGB];
            int total = 0;
#pragma unroll
            for (int i = 0; i < NGB; ++i) {
                part[i] = s_acc[par][i][lig];
                total += s_cnt[par][i];
            }
#pragma unroll
            for (int s = 1; s < NGB; s <<= 1) {
#pragma unroll
                for (int i = 0; i + s < NGB; i += 2 * s) {
                    part[i].x = part[i].x + part[i + s].x; part[i].y = part[i].y + part[i + s].y;
                    part[i].z = part[i].z + part[i + s].z; part[i].w = part[i].w + part[i + s].w;
                }
            }
            // ---- one optimizer step and the projection, by every group on its own copy ----
            float4 x = make_float4(p[0], p[1], p[2], p[3]), g = part[0];
            float nrm = 0.f;
            opt_step4<ADAM>(x, g, mom, vel, a.pcn && total != 0, static_cast<float>(total), a.steps[t], nrm);
            nrm = fold_group_sum<G>(nrm);
            const float dn = fmaxf(1.0f, sqrtf(nrm));
            p[0] = x.x / dn; p[1] = x.y / dn; p[2] = x.z / dn; p[3] = x.w / dn;
        }

        if (grp == 0) {   // every group holds the same row: the first stores it
            if (in_row) *reinterpret_cast<float4*>(a.out + static_cast<size_t>(row.out_row) * a.vdim + col) = make_float4(p[0], p[1], p[2], p[3]);
            if (a.dense) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (valid[e]) a.dense[static_cast<size_t>(row.out_row) * a.d + col + e] = p[e];
            }
        }
        if (a.counts && lig == 0) {
            if (scored) atomicAdd(a.counts + 2 * static_cast<size_t>(row.out_row), scored);
            if (accepted) atomicAdd(a.counts + 2 * static_cast<size_t>(row.out_row) + 1, accepted);
        }
    }
}

}  // namespace bfh
