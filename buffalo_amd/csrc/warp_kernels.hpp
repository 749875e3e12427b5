// WARP on gfx950: the device code of warp.hip -- WarpConsts, the pre-pass, the rejection-sampling trial kernel and the loss kernel.
// The reference semantics are named in warp.hip.
//
// Kernel shape (wave64): a wave owns `chunk` consecutive nnz positions, keeps P[u] in registers
// (K = vdim/64 dwords per lane) across the user's run, and for every positive
//   * takes the first S unseen candidate negatives from a pre-pass (warp_presample_kernel: one thread per positive
//     in CSR order draws Philox candidates and tests them against the user's sorted key run -- "seen" negatives are
//     not counted, warp.cc:137-138 -- so the dependent binary-search chain is off the wave's critical path and runs in
//     cached key runs); beyond S it draws 64 candidates at once (one Philox draw per lane) and tests them in parallel,
//   * scores unseen candidates in draw order, 1/2/4 rows per step (speculation grows when early
//     candidates do not violate the margin), emulating the reference's trial counter exactly
//     (Q-10: the k-th counted candidate is scored at trial = 2k),
//   * accumulates gradP in registers per run; the item-side rows go through the sorted gather of sgd_base.hpp
//     (or, accum_two_pass = 0, fp32 atomics).
// P and Q are frozen during the epoch (only gradients change), so results are independent of the
// order in which waves run, up to fp32 summation order.
#pragma once
#include "sgd_base.hpp"
#include "sgd_row.hpp"

namespace bfh {

enum WarpCounter { kWarpScored, kWarpAccepted, kWarpLoaded, kWarpCounters };   // the slots of WarpConsts::cnt

struct WarpConsts {
    float reg_u, reg_i, reg_j;
    double threshold;
    int max_trial, l2, pcn;
    int chunk;
    int64_t total;
    double* loss_out;        // [0] partial loss sum
    unsigned long long* cnt; // [kWarpScored] scored negatives, [kWarpAccepted] accepted positives, [kWarpLoaded] candidate rows fetched (scored + speculated)
    // two-pass accumulation (sgd_base.hpp GatherParams): record Phi and the violating negative of every accepted
    // positive (Q_rows: rejected); the two item-side gradient rows are summed by grad_gather_kernel
    int two_pass;
    float2* uc_out;          // [total] (user as int bits, Phi; Phi = -1: rejected) -- the fused list of sgd_base.hpp GatherParams::uc
    uint32_t* neg_out;       // [total]
    // pre-drawn unseen candidates (warp_presample_kernel): cand[t * S + k] = k-th unseen draw of positive t (-1: the attempt
    // cap was reached first), next_attempt[t] = the attempt the in-kernel sampler continues from
    const int32_t* cand;
    const int32_t* next_attempt;
};

constexpr uint32_t kWarpAttemptCap = 64 * 64;   // draws per positive before giving up on "seen" candidates (the reference never does)
constexpr int kWarpSpec = 4;                    // max candidate rows scored per step

// the sampler's position counter of the chunk's positive t: global over chunks and shards
__device__ __forceinline__ uint64_t warp_gpos(const SgdParams& p, int64_t t) { return static_cast<uint64_t>(p.nnz_offset + p.shift + t); }

// user u's sorted key run [ubeg, uend), as positions of the chunk
__device__ __forceinline__ int64_t warp_user_begin(const SgdParams& p, int u) { return (u == 0 ? 0 : p.indptr[u - 1]) - p.shift; }
__device__ __forceinline__ int64_t warp_user_end(const SgdParams& p, int u) { return p.indptr[u] - p.shift; }

// the candidate of one attempt: a pure function of (seed, global nnz position, epoch, attempt)
__device__ __forceinline__ int warp_candidate(const SgdParams& p, uint64_t gpos, uint32_t attempt) {
    uint32_t o0, o1;
    counter_draw(p.seed, 1u, gpos, 0u, p.epoch, attempt, o0, o1);
    return static_cast<int>((static_cast<uint64_t>(o0) * static_cast<uint32_t>(p.Q_rows)) >> 32);
}

template <int S>
__global__ __launch_bounds__(256) void warp_presample_kernel(SgdParams p, int64_t total, int32_t* __restrict__ cand, int32_t* __restrict__ next_attempt) {
    const int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (t >= total) return;
    const int u = p.rows[t];
    const int64_t ubeg = warp_user_begin(p, u), uend = warp_user_end(p, u);
    const uint64_t gpos = warp_gpos(p, t);
    int k = 0;
    uint32_t a = 0;
    for (; a < kWarpAttemptCap && k < S; ++a) {
        const int c = warp_candidate(p, gpos, a);
        if (!sorted_contains(p.keys, ubeg, uend, c)) cand[t * S + k++] = c;
    }
    for (; k < S; ++k) cand[t * S + k] = -1;
    next_attempt[t] = static_cast<int32_t>(a);
}

// warp.cc:21-28
template <int K>
__device__ __forceinline__ float warp_score_part(const Row<K>& u, const Row<K>& i, bool l2) {
    float s = 0.f;
    if (!l2) {
#pragma unroll
        for (int k = 0; k < K; ++k) s += u.v[k] * i.v[k];
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float df = u.v[k] - i.v[k];
            s -= df * df;
        }
    }
    return s;
}

// The trial loop of one positive (warp.cc:133-147): seen draws are not counted, the k-th counted candidate is scored at trial = 2k (Q-10)
template <int K>
struct WarpTrial {
    int kcount = 0;        // counted (unseen) candidates scored so far
    bool found = false, done = false;
    int neg = 0;           // the violating negative, its score and its row
    float uj = 0.f;
    Row<K> qj;
    int bsz = 1;           // candidate rows the next step scores: 1, 2, 4, 4 ...
    __device__ __forceinline__ bool exhausted(int max_trial) const { return 1 + 2 * kcount > max_trial; }   // `while (trial <= max_trial)` fails
    __device__ __forceinline__ int trial() const { return found ? 2 * kcount : 2 * kcount + 1; }
};

// One batch of the pre-drawn ladder: candidates B0 .. B0 + BS - 1 of positive j (lane j's my_c) at compile-time register indices, so that
// my_c stays in registers; a -1 (the attempt cap was reached first) ends the batch.  `score` scores up to kWarpSpec candidates.
template <int B0, int BS, int K, int S, typename Score>
__device__ __forceinline__ void warp_score_predrawn(const WarpTrial<K>& tr, const int (&my_c)[S], int j, Score& score) {
    if constexpr (B0 < S) {
        if (tr.done) return;
        int cl[kWarpSpec];
        int nb = 0;
#pragma unroll
        for (int s = 0; s < kWarpSpec; ++s) {
            cl[s] = 0;
            if (s < BS && B0 + s < S) {
                const int cc = __builtin_amdgcn_readlane(my_c[B0 + s < S ? B0 + s : 0], j);
                if (cc >= 0 && nb == s) { cl[s] = cc; nb = s + 1; }
            }
        }
        if (nb > 0) score(cl, nb);
    }
}

// The in-kernel sampler: one draw per lane (lane's attempt), a ballot of the unseen ones, up to tr.bsz of them per scoring step in draw order
template <int K, typename Score>
__device__ __forceinline__ void warp_draw_and_score(const WarpTrial<K>& tr, const SgdParams& p, uint64_t gpos, int64_t ubeg, int64_t uend,
                                                    uint32_t attempt, Score& score) {
    const int cand = warp_candidate(p, gpos, attempt);
    const bool seen = attempt >= kWarpAttemptCap || sorted_contains(p.keys, ubeg, uend, cand);
    unsigned long long unseen = __ballot(!seen);
    while (unseen != 0ull && !tr.done) {
        int cl[kWarpSpec];
        int nb = 0;
        unsigned long long m = unseen;
#pragma unroll
        for (int s = 0; s < kWarpSpec; ++s) {
            cl[s] = 0;
            if (s < tr.bsz && m != 0ull) {
                const int l = __builtin_ctzll(m);
                m &= m - 1ull;
                cl[s] = __builtin_amdgcn_readlane(cand, l);
                nb = s + 1;
            }
        }
        unseen = m;
        score(cl, nb);
    }
}

// Phi = log(max(1, int((Q_rows - |seen| - 1) / trial)))  (warp.cc:151)
__device__ __forceinline__ float warp_phi(int Q_rows, int64_t nseen, int trial) {
    const int64_t ratio = (static_cast<int64_t>(Q_rows) - nseen - 1) / trial;
    return static_cast<float>(log(static_cast<double>(ratio > 1 ? ratio : 1)));
}

// S: candidates per positive taken from the pre-pass (0: none, every candidate is drawn in the kernel)
template <int K, int S>
__global__ __launch_bounds__(256) void warp_update_kernel(SgdParams p, WarpConsts c) {
    const int lane = threadIdx.x & 63;
    const int wpb = blockDim.x >> 6;
    const int64_t wave0 = static_cast<int64_t>(blockIdx.x) * wpb + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t nwaves = static_cast<int64_t>(gridDim.x) * wpb;
    const int vdim = p.vdim;
    const int64_t n_work = (c.total + c.chunk - 1) / c.chunk;
    const bool l2 = c.l2 != 0;

    int cur_u = -1;
    Row<K> pu, gacc;
    double loss = 0.0;
    unsigned long long scored = 0, accepted = 0, loaded = 0;

    auto flush_user = [&]() {
        if (cur_u < 0) return;
        atomic_add_row<K>(gacc, p.gradP + static_cast<size_t>(cur_u) * vdim, lane, vdim);
        cur_u = -1;
    };

    for (int64_t w = wave0; w < n_work; w += nwaves) {
        const int64_t t_beg = w * c.chunk;
        const int64_t t_end = (t_beg + c.chunk < c.total) ? t_beg + c.chunk : c.total;
        for (int64_t t0 = t_beg; t0 < t_end; t0 += 64) {
            const int64_t t = t0 + lane;
            int my_u = 0, my_pos = 0;
            if (t < t_end) {
                my_u = p.rows[t];
                my_pos = p.keys[t];
            }
            const int n_here = static_cast<int>((t_end - t0) < 64 ? (t_end - t0) : 64);
            float my_phi = -1.f;                                    // two-pass: lane j keeps positive j's Phi (-1: rejected) / negative,
            uint32_t my_nego = static_cast<uint32_t>(p.Q_rows);    // stored coalesced after the walk
            int my_c[S > 0 ? S : 1];
            int my_next = 0;
            if constexpr (S > 0) {
#pragma unroll
                for (int s4 = 0; s4 < S; s4 += 4) {
                    int4 v = make_int4(-1, -1, -1, -1);
                    if (t < t_end) v = *reinterpret_cast<const int4*>(c.cand + t * S + s4);
                    my_c[s4] = v.x; my_c[s4 + 1] = v.y; my_c[s4 + 2] = v.z; my_c[s4 + 3] = v.w;
                }
                if (t < t_end) my_next = c.next_attempt[t];
            }
            for (int j = 0; j < n_here; ++j) {
                const int u = __builtin_amdgcn_readlane(my_u, j);
                const int pos = __builtin_amdgcn_readlane(my_pos, j);
                if (u != cur_u) {
                    flush_user();
                    cur_u = u;
                    load_row<K>(pu, p.P + static_cast<size_t>(u) * vdim, lane, vdim);
#pragma unroll
                    for (int k = 0; k < K; ++k) gacc.v[k] = 0.f;
                }
                const int64_t ubeg = warp_user_begin(p, u), uend = warp_user_end(p, u);
                const uint64_t gpos = warp_gpos(p, t0 + j);
                Row<K> qi;
                load_row<K>(qi, p.Q + static_cast<size_t>(pos) * vdim, lane, vdim);
                const float ui = wave_sum(warp_score_part<K>(pu, qi, l2));

                // ---------------- trial loop (warp.cc:133-147, Q-10) ----------------
                WarpTrial<K> tr;
                // score up to nb candidates (in draw order): load the rows together, then decide one after the other
                auto score = [&](const int (&cl)[kWarpSpec], int nb) {
                    Row<K> cr[kWarpSpec];
                    float sc[kWarpSpec];
#pragma unroll
                    for (int s = 0; s < kWarpSpec; ++s)
                        if (s < nb) load_row<K>(cr[s], p.Q + static_cast<size_t>(cl[s]) * vdim, lane, vdim);
#pragma unroll
                    for (int s = 0; s < kWarpSpec; ++s)
                        if (s < nb) sc[s] = wave_sum(warp_score_part<K>(pu, cr[s], l2));
#pragma unroll
                    for (int s = 0; s < kWarpSpec; ++s) {
                        if (s < nb && !tr.done) {
                            if (tr.exhausted(c.max_trial)) {  // `while (trial <= max_trial)` fails
                                tr.done = true;
                            } else {
                                tr.kcount += 1;
                                scored += 1;
                                if (static_cast<double>(ui - sc[s]) < c.threshold) {
                                    tr.found = true;
                                    tr.done = true;
                                    tr.neg = cl[s];
                                    tr.uj = sc[s];
                                    tr.qj = cr[s];
                                }
                            }
                        }
                    }
                    loaded += nb;
                    if (tr.bsz < kWarpSpec) tr.bsz <<= 1;
                };
                uint32_t a0 = 0;       // attempt the in-kernel sampler starts from
                if constexpr (S > 0) {
                    // pre-drawn candidates: batches of 1, 2, 4, 4 ...
                    a0 = static_cast<uint32_t>(__builtin_amdgcn_readlane(my_next, j));
                    warp_score_predrawn<0, 1>(tr, my_c, j, score);
                    warp_score_predrawn<1, 2>(tr, my_c, j, score);
                    warp_score_predrawn<3, 4>(tr, my_c, j, score);
                    warp_score_predrawn<7, 4>(tr, my_c, j, score);
                    if (!tr.done && tr.exhausted(c.max_trial)) tr.done = true;
                }
                for (; a0 < kWarpAttemptCap && !tr.done; a0 += 64) {  // the reference never gives up on "seen" draws
                    warp_draw_and_score(tr, p, gpos, ubeg, uend, a0 + lane, score);
                    if (!tr.done && tr.exhausted(c.max_trial)) tr.done = true;
                }
                const int trial = tr.trial();
                if (!tr.found || trial >= c.max_trial) continue;  // warp.cc:148-149

                const float Phi = warp_phi(p.Q_rows, uend - ubeg, trial);
                Row<K> gi, gj;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    float ud, idv, jdv;
                    if (!l2) {  // warp.cc:30-40
                        ud = Phi * (qi.v[k] - tr.qj.v[k]);
                        idv = Phi * pu.v[k];
                        jdv = -idv;
                    } else {    // warp.cc:42-52 (Q-11)
                        ud = Phi * 2 * (qi.v[k] - tr.qj.v[k]);
                        idv = Phi * (pu.v[k] - qi.v[k]);
                        jdv = -Phi * (pu.v[k] - tr.qj.v[k]);
                    }
                    gacc.v[k] += ud - c.reg_u * pu.v[k];
                    gi.v[k] = idv - c.reg_i * qi.v[k];
                    gj.v[k] = jdv - c.reg_j * tr.qj.v[k];
                }
                if (c.two_pass) {
                    if (lane == j) {
                        my_phi = Phi;
                        my_nego = static_cast<uint32_t>(tr.neg);
                    }
                    if (c.pcn && lane == 0) atomicAdd(p.cntP + u, 1);
                } else {
                    atomic_add_row<K>(gi, p.gradQ + static_cast<size_t>(pos) * vdim, lane, vdim);
                    atomic_add_row<K>(gj, p.gradQ + static_cast<size_t>(tr.neg) * vdim, lane, vdim);
                    if (c.pcn && lane == 0) {
                        atomicAdd(p.cntP + u, 1);
                        atomicAdd(p.cntQ + pos, 1);
                        atomicAdd(p.cntQ + tr.neg, 1);
                    }
                }
                loss += static_cast<double>(tr.uj - ui) + c.threshold;
                accepted += 1;
            }
            if (c.two_pass && t < t_end) {
                c.uc_out[t] = make_float2(__builtin_bit_cast(float, my_u), my_phi);
                c.neg_out[t] = my_nego;
            }
        }
        flush_user();
    }
    flush_user();
    if (lane == 0) {
        if (loss != 0.0) atomicAdd(c.loss_out, loss);
        if (scored) atomicAdd(c.cnt + kWarpScored, scored);
        if (accepted) atomicAdd(c.cnt + kWarpAccepted, accepted);
        if (loaded) atomicAdd(c.cnt + kWarpLoaded, loaded);
    }
}

// CWARP::compute_loss warp.cc:205-226: fraction of sampled triples that violate the margin.
__global__ void warp_loss_kernel(const float* __restrict__ P, const float* __restrict__ Q, const int32_t* __restrict__ users,
                                 const int32_t* __restrict__ pos, const int32_t* __restrict__ neg, int n, int vdim, int l2,
                                 double threshold, unsigned long long* out) {
    const int lane = threadIdx.x & 63;
    const int w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (w >= n) return;
    const float* pu = P + static_cast<size_t>(users[w]) * vdim;
    const float* qi = Q + static_cast<size_t>(pos[w]) * vdim;
    const float* qj = Q + static_cast<size_t>(neg[w]) * vdim;
    float a = 0.f, b = 0.f;
    for (int e = lane; e < vdim; e += 64) {
        if (!l2) {
            a += pu[e] * qi[e];
            b += pu[e] * qj[e];
        } else {
            const float d1 = pu[e] - qi[e], d2 = pu[e] - qj[e];
            a -= d1 * d1;
            b -= d2 * d2;
        }
    }
    const float xi = wave_sum(a), xj = wave_sum(b);
    if (lane == 0 && (static_cast<double>(xi) - static_cast<double>(xj)) < threshold) atomicAdd(out, 1ull);
}

}  // namespace bfh
