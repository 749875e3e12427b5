// BPRMF on gfx950: the device code of bpr.hip -- BprConsts, the row helpers, the user-major update kernel, the loss kernel and
// the kernels of the per-XCD replicas (policy 2, shared with the item-major walk of bpr_item_major.hpp).
//
// Reference semantics: CBPRMF::worker (/root/reference/lib/algo_impl/bpr/bpr.cc:72-188); see bpr.hip.
//
// Kernel shape (wave64):
//   * the chunk's nnz positions are cut into work items of `chunk` consecutive positions; a wave
//     owns a work item (perfect load balance on heavy-tailed degrees, coalesced key/row-id loads);
//   * per 64 positions the lanes sample negatives in parallel (Philox counter draws, verify_neg by
//     binary search in the user's sorted key run);
//   * the wave then walks the 64 triples with the next triple's item rows prefetched; a dot product
//     is a few FMAs per lane + a DPP row reduction -- no LDS, no barrier;
//   * P[u] lives in registers across the user's run (one load + one store per run instead of per
//     triple);
//   * item rows are shared by every wave on the chip.  The 8 XCDs have private, mutually
//     non-coherent L2s, so "just store the row" silently forks Q into 8 copies (measured: 14
//     concurrent waves on a 400-item table lose 9/10 of the learning signal).  Two coherent forms:
//       - write-through Hogwild (policy 0): rows are float4 per lane, read with `buffer_load_dwordx4
//         sc1` and written with `buffer_store_dwordx4 sc1` (device scope: bypass L1, write through
//         L2), i.e. lock-free racy read-modify-write like the CPU reference, visible chip-wide;
//       - fp32 hardware atomics (policy 1): K = vdim/64 dwords per lane (element k*64+lane) so one
//         `global_atomic_add_f32` covers two full cache lines; no update is ever lost.
//     Measured on MI355X (scripts/micro/atomics.hip): uniform 512-B row atomics run at
//     2.6 G rows/s and a single hot row at 24 ns per update, write-through rows at ~2.3 G rows/s;
//     on a small catalogue write-through loses most colliding updates (NDCG 0.04 vs 0.27 on the
//     400-item planted test), so atomics are this walk's default.  Policy 2 runs it on per-XCD replicas of Q
//     (plain stores through the XCD's own L2, merged by the delta rule) with the popular rows on atomics.
#pragma once
#include "sgd_base.hpp"

namespace bfh {

struct BprConsts {
    float lr, reg_u, reg_i, reg_j, reg_b;
    double lr_d, reg_b_d;   // the bias statements of the reference are scalar C++ in double (bpr.cc:81, 99, 162, 168)
    int use_bias, update_i, update_j, verify_neg, uniform, num_neg, pcn, compute_loss, atomic, sequential;
    int64_t cum_total;
    const float* exp_table;
    double* loss_out;
    int chunk;
    int neg_limit;        // study knob: uniform negatives are folded into [0, neg_limit) (0: off) -- what the walk does when the negatives' rows fit an L2
    // injected triples (bfh_bpr_update_triples)
    const int32_t* inj_u;
    const int32_t* inj_p;
    const int32_t* inj_n;
    int64_t total;  // number of (position, slot) items
    int64_t work_begin, work_end;  // work items [begin, end) of this launch (a segment of the call)
    // policy 2: one private copy of the item factors per XCD (see xcd_* kernels below)
    float* rep_Q;
    float* rep_Qb;
    int64_t rep_stride, rep_bstride;
    const uint8_t* hot;   // [Q_rows] 1 = row stays in the chip-wide matrix and is updated with atomics
    int fresh;            // re-read replica rows right before storing them
    // adam / adagrad, two-pass accumulation (sgd_base.hpp GatherParams): this kernel only records the logit and the
    // negative of every triple; the item-side gradient rows are summed by grad_gather_kernel
    int two_pass;
    float2* uc_out;       // [total] (user as int bits, logit): the fused list of sgd_base.hpp GatherParams::uc
    uint32_t* neg_out;    // [total]
};

// new bias = (float)(b + alpha * (+-logit - reg_b * b)) with the product and sums in double, as the reference's scalar statement rounds
__device__ __forceinline__ float bias_step(float b, float signed_logit, double lr, double reg_b) {
    return static_cast<float>(static_cast<double>(b) + lr * (static_cast<double>(signed_logit) - reg_b * static_cast<double>(b)));
}


// The XCD this wave runs on (0..7), from the hardware register: the address of a wave's item-factor
// replica depends on it, so it must be the truth, not a guess from blockIdx.
__device__ __forceinline__ int xcc_id() {
    unsigned x;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(x));
    return static_cast<int>(x & 7u);
}

// CBPRMF::build_exp_table bpr.cc:57-63 + lookup bpr.cc:124-131 (Q-2: integer 1000/6/2 == 83)
__device__ __forceinline__ float bpr_logit(float x, const float* __restrict__ table) {
    if (6.0f < x) return 0.0f;
    if (x < -6.0f) return 1.0f;
    const int idx = __builtin_amdgcn_readfirstlane(static_cast<int>((x + 6.0f) * 83.0f));
    return table[idx];
}

// the candidate of one attempt: a pure function of (seed, global nnz position, slot, epoch, attempt)
__device__ __forceinline__ int bpr_draw_candidate(const SgdParams& p, const BprConsts& c, uint64_t gpos, uint32_t slot, uint32_t attempt) {
    uint32_t o0, o1;
    counter_draw(p.seed, 0u, gpos, slot, p.epoch, attempt, o0, o1);
    if (c.uniform) {
        const int neg = static_cast<int>((static_cast<uint64_t>(o0) * static_cast<uint32_t>(p.Q_rows)) >> 32);
        return c.neg_limit > 0 ? neg % c.neg_limit : neg;
    }
    const uint64_t r64 = (static_cast<uint64_t>(o1) << 32) | o0;
    const int64_t r = static_cast<int64_t>(__umul64hi(r64, static_cast<uint64_t>(c.cum_total)));
    return static_cast<int>(lower_bound_dev<int64_t>(p.cum_table, p.Q_rows, r));  // Q-4: lower_bound
}

// `first_attempt`: the attempts before it are known to be rejected (bpr_presample_exceptions_kernel)
__device__ __forceinline__ int bpr_sample_negative(const SgdParams& p, const BprConsts& c, uint64_t gpos, uint32_t slot,
                                                   int64_t ubeg, int64_t uend, uint32_t first_attempt = 0) {
    int neg = 0;
    for (uint32_t attempt = first_attempt; attempt < (1u << 20); ++attempt) {  // the reference loops forever (bpr.cc:106-117)
        neg = bpr_draw_candidate(p, c, gpos, slot, attempt);
        if (!c.verify_neg || !sorted_contains(p.keys, ubeg, uend, neg)) break;
    }
    return neg;
}

template <int K>
struct Row {
    float v[K];
};

template <int K>
__device__ __forceinline__ void load_row(Row<K>& r, const float* __restrict__ base, int lane, int vdim) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int e = k * 64 + lane;
        r.v[k] = (e < vdim) ? base[e] : 0.0f;
    }
}
// same map, every dword loaded past the CU's L1 (global_load_dword sc1): what another CU of this
// XCD stored is in the L2, not in this CU's L1
template <int K>
__device__ __forceinline__ void load_row_coh(Row<K>& r, const float* base, int lane, int vdim) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int e = k * 64 + lane;
        r.v[k] = (e < vdim) ? __hip_atomic_load(base + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0f;
    }
}
template <int K>
__device__ __forceinline__ void store_row(const Row<K>& r, float* __restrict__ base, int lane, int vdim) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int e = k * 64 + lane;
        if (e < vdim) base[e] = r.v[k];
    }
}
template <int K>
__device__ __forceinline__ void atomic_add_row(const Row<K>& r, float* __restrict__ base, int lane, int vdim) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int e = k * 64 + lane;
        if (e < vdim) atomic_add_f32(base + e, r.v[k]);
    }
}

// the b128 buffer builtins traffic in their own 128-bit type: always go through bit_cast (an
// implicit conversion to an ext_vector splats the low dword!)
using b128_t = decltype(__builtin_amdgcn_raw_buffer_load_b128(__amdgpu_buffer_rsrc_t(), 0, 0, 0));
struct f32q { float v[4]; };

// Row I/O.  V4 == false: element k*64+lane (dword per lane).  V4 == true: K = 4*KV, lane holds the
// 4 consecutive floats (kv*64+lane)*4 .. +3, moved with 16-byte buffer instructions whose bounds
// check (num_records = row bytes) masks the lanes beyond vdim; COH selects sc1 (device-coherent).
template <int K, bool V4, bool COH>
__device__ __forceinline__ void row_load(Row<K>& r, const float* __restrict__ base, int lane, int vdim) {
    if constexpr (V4) {
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, vdim * 4, 0x00020000);
#pragma unroll
        for (int kv = 0; kv < K / 4; ++kv) {
            const b128_t raw = COH ? __builtin_amdgcn_raw_buffer_load_b128(rs, (kv * 64 + lane) * 16, 0, 16)
                                   : __builtin_amdgcn_raw_buffer_load_b128(rs, (kv * 64 + lane) * 16, 0, 0);
            const f32q v = __builtin_bit_cast(f32q, raw);
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4) r.v[kv * 4 + c4] = v.v[c4];
        }
    } else {
        load_row<K>(r, base, lane, vdim);
    }
}
template <int K, bool V4, bool COH>
__device__ __forceinline__ void row_store(const Row<K>& r, float* __restrict__ base, int lane, int vdim) {
    if constexpr (V4) {
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(base, 0, vdim * 4, 0x00020000);
#pragma unroll
        for (int kv = 0; kv < K / 4; ++kv) {
            f32q v;
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4) v.v[c4] = r.v[kv * 4 + c4];
            const b128_t raw = __builtin_bit_cast(b128_t, v);
            if (COH) __builtin_amdgcn_raw_buffer_store_b128(raw, rs, (kv * 64 + lane) * 16, 0, 16);
            else __builtin_amdgcn_raw_buffer_store_b128(raw, rs, (kv * 64 + lane) * 16, 0, 0);
        }
    } else {
        store_row<K>(r, base, lane, vdim);
    }
}
template <int K, bool V4>
__device__ __forceinline__ void row_atomic_add(const Row<K>& r, float* __restrict__ base, int lane, int vdim) {
    if constexpr (V4) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int e = ((k >> 2) * 64 + lane) * 4 + (k & 3);
            if (e < vdim) atomic_add_f32(base + e, r.v[k]);
        }
    } else {
        atomic_add_row<K>(r, base, lane, vdim);
    }
}
// float4 rows with the non-temporal hint on top (aux bit 1): load past the L1 (sc1) as row_load<.., COH>, store plain
template <int K>
__device__ __forceinline__ void row_load_nt(Row<K>& r, const float* __restrict__ base, int lane, int vdim) {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, vdim * 4, 0x00020000);
#pragma unroll
    for (int kv = 0; kv < K / 4; ++kv) {
        const f32q v = __builtin_bit_cast(f32q, __builtin_amdgcn_raw_buffer_load_b128(rs, (kv * 64 + lane) * 16, 0, 18));
#pragma unroll
        for (int c4 = 0; c4 < 4; ++c4) r.v[kv * 4 + c4] = v.v[c4];
    }
}
template <int K>
__device__ __forceinline__ void row_store_nt(const Row<K>& r, float* __restrict__ base, int lane, int vdim) {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(base, 0, vdim * 4, 0x00020000);
#pragma unroll
    for (int kv = 0; kv < K / 4; ++kv) {
        f32q v;
#pragma unroll
        for (int c4 = 0; c4 < 4; ++c4) v.v[c4] = r.v[kv * 4 + c4];
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(b128_t, v), rs, (kv * 64 + lane) * 16, 0, 2);
    }
}
// device-coherent scalar (bias) access for the write-through policy
__device__ __forceinline__ float coh_load(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void coh_store(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// SGD: true -> Hogwild SGD branch (bpr.cc:157-172); false -> gradient accumulation branch for
// adam/adagrad (bpr.cc:138-156,175-181).  PIPE: prefetch the next triple's item rows.
// INJECT: triples come from arrays instead of CSR + sampler.  V4: float4 layout + sc1 item-row I/O.
template <int K, bool SGD, bool PIPE, bool INJECT, bool V4>
__global__ __launch_bounds__(256) void bpr_update_kernel(SgdParams p, BprConsts c) {
    const int lane = threadIdx.x & 63;
    const int wpb = blockDim.x >> 6;
    const int64_t wave0 = static_cast<int64_t>(blockIdx.x) * wpb + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t nwaves = static_cast<int64_t>(gridDim.x) * wpb;
    const int vdim = p.vdim;
    // item factors this wave works on: the chip-wide matrix, or (policy 2) the replica owned by
    // the wave's XCD -- only waves of that XCD ever touch it, so its L2 is the point of coherence
    // and plain stores are visible to every other wave that can read the row
    float* Qbase = p.Q;
    float* Qbbase = p.Qb;
    bool rep = false;
    if constexpr (SGD) {
        if (c.atomic == 2) {
            const int x = xcc_id();
            Qbase = c.rep_Q + static_cast<size_t>(x) * c.rep_stride;
            Qbbase = c.rep_Qb + static_cast<size_t>(x) * c.rep_bstride;
            rep = true;
        }
    }

    // policy 2 keeps the popular ("hot") rows in the chip-wide matrix: (pol bit set) <=> atomics on p.Q
    auto q_of = [&](int item, bool hot) -> float* { return (hot ? p.Q : Qbase) + static_cast<size_t>(item) * vdim; };
    auto qb_of = [&](int item, bool hot) -> float* { return (hot ? p.Qb : Qbbase) + item; };
    // item rows and biases are read past the L1 whenever another CU may have plain-stored them
    auto qload = [&](Row<K>& r, const float* base) {
        if constexpr (V4) row_load<K, true, true>(r, base, lane, vdim);
        else if (rep) load_row_coh<K>(r, base, lane, vdim);
        else load_row<K>(r, base, lane, vdim);
    };
    auto bload = [&](const float* ptr) -> float { return (V4 || rep) ? coh_load(ptr) : *ptr; };

    int cur_u = -1;
    bool cur_excl = true;
    Row<K> pu, p0;     // current / as-loaded user row (SGD) or accumulated / unused (accumulate)
    Row<K> gacc;       // accumulate mode: gradient of P[u] gathered over the run
    double loss = 0.0;

    auto flush_user = [&]() {
        if (cur_u < 0) return;
        if (SGD) {
            float* Pu = p.P + static_cast<size_t>(cur_u) * vdim;
            if (cur_excl) {
                row_store<K, V4, false>(pu, Pu, lane, vdim);   // the run is owned by this wave
            } else {
                Row<K> dlt;
#pragma unroll
                for (int k = 0; k < K; ++k) dlt.v[k] = pu.v[k] - p0.v[k];
                row_atomic_add<K, V4>(dlt, Pu, lane, vdim);
            }
        } else {
            row_atomic_add<K, V4>(gacc, p.gradP + static_cast<size_t>(cur_u) * vdim, lane, vdim);
        }
        cur_u = -1;
    };

    for (int64_t w = c.work_begin + wave0; w < c.work_end; w += nwaves) {
        const int64_t t_beg = w * c.chunk;
        const int64_t t_end = (t_beg + c.chunk < c.total) ? t_beg + c.chunk : c.total;
        for (int64_t t0 = t_beg; t0 < t_end; t0 += 64) {
            // ---------------- lane-parallel: fetch (u,pos) and sample the negative ----------------
            const int64_t t = t0 + lane;
            const bool valid = t < t_end;
            int my_u = 0, my_pos = 0, my_neg = 0, my_excl = 1, my_pol = 3;  // bit0: pos row atomic, bit1: neg row atomic
            if (valid) {
                if (INJECT) {
                    my_u = c.inj_u[t];
                    my_pos = c.inj_p[t];
                    my_neg = c.inj_n[t];
                    my_excl = c.sequential;
                } else {
                    const int64_t pos_idx = t / c.num_neg;           // chunk-local nnz position
                    const uint32_t slot = static_cast<uint32_t>(t % c.num_neg);
                    my_u = p.rows[pos_idx];
                    my_pos = p.keys[pos_idx];
                    const int64_t ubeg = (my_u == 0 ? 0 : p.indptr[my_u - 1]) - p.shift;
                    const int64_t uend = p.indptr[my_u] - p.shift;
                    my_neg = bpr_sample_negative(p, c, static_cast<uint64_t>(p.nnz_offset + p.shift + pos_idx), slot, ubeg, uend);
                    // does this wave own the user's whole run?  (then P[u] needs no atomics)
                    my_excl = c.sequential || (ubeg * c.num_neg >= t_beg && uend * c.num_neg <= t_end);
                }
                if (c.sequential || c.atomic != 1) my_pol = 0;   // sequential: one wave, plain stores are exact
                if (rep && c.hot) my_pol = (c.hot[my_pos] ? 1 : 0) | (c.hot[my_neg] ? 2 : 0);
            }
            const int n_here = static_cast<int>((t_end - t0) < 64 ? (t_end - t0) : 64);
            float my_coef = 0.f;   // two-pass accumulation: lane j keeps triple j's logit, stored coalesced after the walk
            if (!SGD && !INJECT && c.two_pass && valid) c.neg_out[t] = static_cast<uint32_t>(my_neg);

            Row<K> qi, qj, qi_n, qj_n;
            float bi = 0.f, bj = 0.f, bi_n = 0.f, bj_n = 0.f;
            int pos = __builtin_amdgcn_readlane(my_pos, 0);
            int neg = __builtin_amdgcn_readlane(my_neg, 0);
            if (PIPE) {
                const int pol0 = __builtin_amdgcn_readlane(my_pol, 0);
                const bool h_i = rep && (pol0 & 1), h_j = rep && (pol0 & 2);
                qload(qi, q_of(pos, h_i));
                qload(qj, q_of(neg, h_j));
                if (c.use_bias) { bi = bload(qb_of(pos, h_i)); bj = bload(qb_of(neg, h_j)); }
            }
            for (int j = 0; j < n_here; ++j) {
                const int u = __builtin_amdgcn_readlane(my_u, j);
                const int excl = __builtin_amdgcn_readlane(my_excl, j);
                const int pol = __builtin_amdgcn_readlane(my_pol, j);
                const bool at_i = (pol & 1) != 0, at_j = (pol & 2) != 0;
                pos = __builtin_amdgcn_readlane(my_pos, j);
                neg = __builtin_amdgcn_readlane(my_neg, j);
                float* Qi = q_of(pos, rep && at_i);
                float* Qj = q_of(neg, rep && at_j);
                float* Bi = qb_of(pos, rep && at_i);
                float* Bj = qb_of(neg, rep && at_j);
                int pos_n = 0, neg_n = 0;
                bool hn_i = false, hn_j = false;
                if (PIPE) {
                    if (j + 1 < n_here) {
                        pos_n = __builtin_amdgcn_readlane(my_pos, j + 1);
                        neg_n = __builtin_amdgcn_readlane(my_neg, j + 1);
                        const int pol_n = __builtin_amdgcn_readlane(my_pol, j + 1);
                        hn_i = rep && (pol_n & 1);
                        hn_j = rep && (pol_n & 2);
                        qload(qi_n, q_of(pos_n, hn_i));
                        qload(qj_n, q_of(neg_n, hn_j));
                        if (c.use_bias) {
                            bi_n = bload(qb_of(pos_n, hn_i));
                            bj_n = bload(qb_of(neg_n, hn_j));
                        }
                    }
                } else {
                    qload(qi, Qi);
                    qload(qj, Qj);
                    if (c.use_bias) { bi = bload(Bi); bj = bload(Bj); }
                }
                if (u != cur_u) {
                    flush_user();
                    cur_u = u;
                    cur_excl = excl != 0;
                    row_load<K, V4, false>(pu, p.P + static_cast<size_t>(u) * vdim, lane, vdim);
                    if (SGD) {
                        p0 = pu;
                    } else {
#pragma unroll
                        for (int k = 0; k < K; ++k) gacc.v[k] = 0.f;
                    }
                }
                // ---------------- score + sigmoid table (bpr.cc:119-131) ----------------
                float part = 0.f;
#pragma unroll
                for (int k = 0; k < K; ++k) part += pu.v[k] * (qi.v[k] - qj.v[k]);
                float x = wave_sum(part);
                if (c.use_bias) x += (bi - bj);
                const float logit = bpr_logit(x, c.exp_table);
                if (c.compute_loss) loss += static_cast<double>(log1pf(__expf(-fminf(fmaxf(x, -6.f), 6.f))));

                if (SGD) {
                    // bpr.cc:157-171 incl. Q-1: the user step sees the already-updated item rows
                    Row<K> di, dj;
                    // pos == neg can only happen with verify_neg=false or injected triples; the
                    // reference then updates the one row twice in sequence (bpr.cc:159-169)
                    const bool same = pos == neg;
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        const float idv = logit * pu.v[k];
                        di.v[k] = c.update_i ? c.lr * (idv - c.reg_i * qi.v[k]) : 0.f;
                        qi.v[k] += di.v[k];
                        if (same) qj.v[k] = qi.v[k];
                        dj.v[k] = c.update_j ? c.lr * (-idv - c.reg_j * qj.v[k]) : 0.f;
                        qj.v[k] += dj.v[k];
                        if (same) qi.v[k] = qj.v[k];
                        pu.v[k] += c.lr * (logit * (qi.v[k] - qj.v[k]) - c.reg_u * pu.v[k]);
                    }
                    // replica rows: optionally re-read the row right before the store, so that the window in
                    // which another wave's update of the same row can be overwritten is one L2 round trip
                    // instead of the prefetch distance (the step itself was computed from the prefetched row)
                    const bool fr_i = rep && c.fresh && c.update_i && !at_i, fr_j = rep && c.fresh && c.update_j && !at_j && !same;
                    Row<K> fi, fj;
                    if (fr_i) qload(fi, Qi);
                    if (fr_j) qload(fj, Qj);
                    if (c.update_i) {
                        if (at_i) row_atomic_add<K, V4>(di, Qi, lane, vdim);
                        else if (fr_i) {
#pragma unroll
                            for (int k = 0; k < K; ++k) fi.v[k] += di.v[k];
                            row_store<K, V4, false>(fi, Qi, lane, vdim);
                        }
                        else if (rep) row_store<K, V4, false>(qi, Qi, lane, vdim);
                        else row_store<K, V4, true>(qi, Qi, lane, vdim);
                    }
                    if (c.update_j) {
                        if (at_j) row_atomic_add<K, V4>(dj, Qj, lane, vdim);
                        else if (fr_j) {
#pragma unroll
                            for (int k = 0; k < K; ++k) fj.v[k] += dj.v[k];
                            row_store<K, V4, false>(fj, Qj, lane, vdim);
                        }
                        else if (rep) row_store<K, V4, false>(qj, Qj, lane, vdim);
                        else row_store<K, V4, true>(qj, Qj, lane, vdim);
                    }
                    if (c.use_bias && lane == 0) {
                        // bpr.cc:162, 168 are scalar statements with `double alpha`, `double reg_b`: evaluated in double, stored as float
                        const float bi_new = c.update_i ? bias_step(bi, logit, c.lr_d, c.reg_b_d) : bi;
                        if (same) bj = bi_new;
                        const float bj_new = bias_step(bj, -logit, c.lr_d, c.reg_b_d);
                        if (c.update_i) {
                            if (at_i) atomic_add_f32(Bi, bi_new - bi);
                            else if (V4 && !rep) coh_store(Bi, bi_new);
                            else *Bi = bi_new;
                        }
                        if (c.update_j) {
                            if (at_j) atomic_add_f32(Bj, bj_new - bj);
                            else if (V4 && !rep) coh_store(Bj, bj_new);
                            else *Bj = bj_new;
                        }
                    }
                } else {
                    // bpr.cc:138-156: P, Q are frozen during the epoch; gradients are summed
                    Row<K> gi, gj;
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        const float idv = logit * pu.v[k];
                        gacc.v[k] += logit * (qi.v[k] - qj.v[k]);
                        gi.v[k] = idv;
                        gj.v[k] = -idv;
                    }
                    if (!INJECT && c.two_pass) {
                        if (lane == j) my_coef = logit;
                        if (c.pcn && lane == 0 && ((t0 + j) % c.num_neg) == c.num_neg - 1) atomicAdd(p.cntP + u, 1);
                    } else {
                    if (c.update_i) row_atomic_add<K, V4>(gi, p.gradQ + static_cast<size_t>(pos) * vdim, lane, vdim);
                    if (c.update_j) row_atomic_add<K, V4>(gj, p.gradQ + static_cast<size_t>(neg) * vdim, lane, vdim);
                    if (lane == 0) {
                        if (c.use_bias) {
                            if (c.update_i) atomic_add_f32(p.gradQb + pos, logit);
                            if (c.update_j) atomic_add_f32(p.gradQb + neg, -logit);
                        }
                        if (c.pcn) {  // Q-9 counting rules (bpr.cc:139-143, 175-181)
                            atomicAdd(p.cntQ + neg, 1);
                            const bool last_slot = INJECT ? true : (((t0 + j) % c.num_neg) == c.num_neg - 1);
                            if (last_slot) {
                                atomicAdd(p.cntP + u, 1);
                                atomicAdd(p.cntQ + pos, 1);
                            }
                        }
                    }
                    }
                }
                if (PIPE) {
                    if (j + 1 < n_here) {
                        qi = qi_n; qj = qj_n; bi = bi_n; bj = bj_n;
                        if (SGD && (!at_i || !at_j) && (pos_n == pos || pos_n == neg || neg_n == pos || neg_n == neg)) {
                            // plain-store rows: the prefetch raced with this wave's own stores -> reload
                            qload(qi, q_of(pos_n, hn_i));
                            qload(qj, q_of(neg_n, hn_j));
                            if (c.use_bias) {
                                bi = bload(qb_of(pos_n, hn_i));
                                bj = bload(qb_of(neg_n, hn_j));
                            }
                        }
                    }
                }
            }
            if (!SGD && !INJECT && c.two_pass && valid) c.uc_out[t] = make_float2(__builtin_bit_cast(float, my_u), my_coef);   // logit >= 0: never "rejected"
        }
        if (!c.sequential) flush_user();
    }
    flush_user();
    if (c.compute_loss && lane == 0 && loss != 0.0) atomicAdd(c.loss_out, loss);
}

// CBPRMF::compute_loss bpr.cc:227-244: mean log(1+exp(-(x_ui - x_uj))) in double; a wave per sample.
__global__ void bpr_loss_kernel(const float* __restrict__ P, const float* __restrict__ Q, const float* __restrict__ Qb,
                                const int32_t* __restrict__ users, const int32_t* __restrict__ pos,
                                const int32_t* __restrict__ neg, int n, int vdim, int use_bias, double* out) {
    const int lane = threadIdx.x & 63;
    const int w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (w >= n) return;
    const float* pu = P + static_cast<size_t>(users[w]) * vdim;
    const float* qi = Q + static_cast<size_t>(pos[w]) * vdim;
    const float* qj = Q + static_cast<size_t>(neg[w]) * vdim;
    float a = 0.f, b = 0.f;
    for (int e = lane; e < vdim; e += 64) {
        a += pu[e] * qi[e];
        b += pu[e] * qj[e];
    }
    float xi = wave_sum(a), xj = wave_sum(b);  // CBPRMF::distance returns float precision
    if (use_bias) { xi += Qb[pos[w]]; xj += Qb[neg[w]]; }
    if (lane == 0) {
        const double x = static_cast<double>(xi) - static_cast<double>(xj);
        atomicAdd(out, log(1.0 + exp(-x)));
    }
}

// ------------------------------------------------------------------------------------------------
// Policy 2: per-XCD replicas of the item factors.
//
// The 8 XCDs' L2s are not coherent with each other, and the only chip-wide coherent update of a
// shared row -- an fp32 atomic per dword, executed one dword per clock per channel -- caps the
// update kernel at half the HBM roofline.  Inside ONE XCD the L2 is the point of coherence: plain
// stores are visible to every wave of that XCD (item rows are loaded with sc1, i.e. past the CU's
// L1).  So every XCD trains on its own copy of Q/Qb with the CPU reference's literal Hogwild
// read-modify-write (bpr.cc:157-172), and the copies are reconciled every `xcd_sync_updates`
// updates with the rule buffalo_amd/dist.py applies between GPUs: Q <- S + sum_x (Q_x - S), where
// S is the state at the previous reconciliation.  A launch boundary writes the L2s back, so the
// merge kernel sees every replica's final state.  An update is therefore never lost between XCDs
// (it arrives at the next merge); within an XCD two waves racing on one row behave like two CPU
// threads racing on it.
// ------------------------------------------------------------------------------------------------
constexpr int kXcdReplicas = 8;

template <typename T>
__global__ __launch_bounds__(256) void xcd_broadcast_kernel(const T* __restrict__ S, T* __restrict__ rep, int64_t n, int64_t stride, int copies) {
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const T v = S[i];
        for (int x = 0; x < copies; ++x) rep[x * stride + i] = v;
    }
}

// the same for the rows whose flag equals `only` (P: the users that have replicas)
template <typename T>
__global__ __launch_bounds__(256) void xcd_broadcast_rows_kernel(const T* __restrict__ S, T* __restrict__ rep, int64_t n, int64_t stride, int copies,
                                                                  const uint8_t* __restrict__ flag, int row_len, int only) {
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        if (flag[i / row_len] != only) continue;
        const T v = S[i];
        for (int x = 0; x < copies; ++x) rep[x * stride + i] = v;
    }
}

__device__ __forceinline__ float4 f4_sub(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
__device__ __forceinline__ float4 f4_add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 f4_fma(float sc, float4 a, float4 b) { return make_float4(sc * a.x + b.x, sc * a.y + b.y, sc * a.z + b.z, sc * a.w + b.w); }
__device__ __forceinline__ float f4_sub(float a, float b) { return a - b; }
__device__ __forceinline__ float f4_add(float a, float b) { return a + b; }
__device__ __forceinline__ float f4_fma(float sc, float a, float b) { return sc * a + b; }

// S <- S + scale * sum_x (rep_x - base); the replicas are refreshed unless this was the last segment.
// Hot rows live in S itself (updated there with atomics) and are skipped; `row_len` = elements per row.
// `base` is what the replicas started the segment from: S itself (policy 2, null), or a ninth copy when S
// also receives atomic steps during the segment (policy 3: the register-resident rows are flushed into S).
// `hot` (per row, or null): with `only` == 0 rows whose flag is non-zero are skipped (the item rows that live chip-wide); with
// `only` != 0 exactly the rows whose flag equals it are merged (P: the users that have replicas, ImQueues::hot_user == 2).
template <typename T>
__global__ __launch_bounds__(256) void xcd_merge_kernel(T* __restrict__ S, T* __restrict__ rep, int64_t n, int64_t stride, float scale,
                                                         int write_replicas, const uint8_t* __restrict__ hot, int row_len, T* __restrict__ base,
                                                         int only = 0, const float* __restrict__ W = nullptr) {
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        if (hot && (only ? hot[i / row_len] != only : hot[i / row_len] != 0)) continue;
        const T s_now = S[i];
        const T s0 = base ? base[i] : s_now;
        T r[kXcdReplicas];
#pragma unroll
        for (int x = 0; x < kXcdReplicas; ++x) r[x] = rep[x * stride + i];
        T acc = f4_sub(r[0], s0);
#pragma unroll
        for (int x = 1; x < kXcdReplicas; ++x) acc = f4_add(acc, f4_sub(r[x], s0));
        const T out = f4_fma(W ? scale * W[i / row_len] : scale, acc, s_now);
        S[i] = out;
        if (write_replicas) {
#pragma unroll
            for (int x = 0; x < kXcdReplicas; ++x) rep[x * stride + i] = out;
            if (base) base[i] = out;
        }
    }
}

// Per-row weight of the merge's sum (the rule of exchange_weight_kernel, sgd_kernels.hpp, applied between the XCDs of one GPU): a
// replica row receives m steps between two merges; with curvature k each contracts the row towards its local equilibrium by
// exp(-lr k), so n replicas that started from the same state combine like ONE run of n m steps when their summed deltas are scaled
// by w = (1 - exp(-n x)) / (n (1 - exp(-x))), x = lr k m  (w -> 1: independent steps, SUM; w -> 1/n: n estimates of one move, MEAN).
// Items: only the NEGATIVE steps of a row land in its replicas (the positive item lives in registers and is flushed into S).
// m is an expectation; steps are whole: a row that saw at most one step over all replicas (n m <= 1) cannot have overshot, so the
// saturation is counted from the second step on, x = lr k (m - 1/n) -- w = 1 exactly for the cold tail (and for conflict-free tests).
__device__ __forceinline__ double xcd_sat_weight(double a, double m, int n) {
    const double x = a * (m - 1.0 / n);
    return (n > 1 && x > 1e-9) ? -expm1(-n * x) / (n * -expm1(-x)) : 1.0;
}
__global__ void xcd_item_weight_kernel(const int64_t* __restrict__ cum, int64_t cum_total, int rows, double neg_steps, double neg_uniform, double lr,
                                       double kq, double kb, int n, float* __restrict__ Wq, float* __restrict__ Wb) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    double pneg = neg_uniform;
    if (cum) pneg = static_cast<double>(cum[i] - (i ? cum[i - 1] : 0)) / static_cast<double>(cum_total);
    const double m = neg_steps * pneg / n;      // negative steps of row i per replica between two merges
    Wq[i] = static_cast<float>(xcd_sat_weight(lr * kq, m, n));
    Wb[i] = static_cast<float>(xcd_sat_weight(lr * kb, m, n));
}
// Users that have replicas: every step of the user lands in them, spread over n queues (im_keys_kernel's rule: all nq, or for
// spread mode 3 the smallest power of two r with deg < heavy_deg * r).
__global__ void xcd_user_weight_kernel(const int64_t* __restrict__ indptr, int first_row, int rows, double steps_per_entry, double lr, double kp, int nq,
                                       int spread_mode, int64_t heavy_deg, float* __restrict__ Wp) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= rows) return;
    const int g = first_row + u;
    const int64_t deg = indptr[g] - (g ? indptr[g - 1] : 0);
    int n = nq;
    if (spread_mode == 3 && heavy_deg > 0) {
        n = 2;
        while (n < nq && deg >= heavy_deg * n) n <<= 1;
        if (n > nq) n = nq;
    }
    Wp[g] = static_cast<float>(xcd_sat_weight(lr * kp, static_cast<double>(deg) * steps_per_entry / n, n));
}

// How often is every item row updated?  One int atomic per index (once per resident CSR).
__global__ void item_count_kernel(const int32_t* __restrict__ idx, int64_t n, int* __restrict__ cnt) {
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * blockDim.x)
        atomicAdd(cnt + idx[i], 1);
}

// A row is hot when the expected number of OTHER waves of the same XCD holding it between their load
// and their store -- updates_i / updates_total * (item rows in flight per XCD) -- reaches tau: those
// rows would lose that fraction of their updates to racing plain stores (a CPU Hogwild thread pool
// sits at a few percent on the head items).  updates_i = positives_i * pos_mult + triples * P(neg = i).
__global__ void xcd_hot_kernel(const int* __restrict__ cnt, const int64_t* __restrict__ cum, int64_t cum_total, int rows, double pos_mult,
                               double triples, double neg_uniform, double inflight, double tau, uint8_t* __restrict__ hot) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    double pneg = neg_uniform;
    if (cum) pneg = static_cast<double>(cum[i] - (i ? cum[i - 1] : 0)) / static_cast<double>(cum_total);
    const double upd = cnt[i] * pos_mult + triples * pneg;
    hot[i] = (upd * inflight >= tau * 2.0 * triples) ? 1 : 0;
}

}  // namespace bfh
