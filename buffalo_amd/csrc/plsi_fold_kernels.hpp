// pLSI row steps and the fold-in kernel (included by plsi.hip alone).
//
// Two things live here:
//   * the steps on ONE row that the training kernels of plsi.hip and the fold-in kernel both run -- the entry walk of a lane group
//     (`plsi_walk_entries`), the butterfly over the groups of a wave (`plsi_team_sum`) and the row normalisation (`plsi_normalize_row`).
//     They are written once, so a folded row and a trained row are the same instructions in the same order: the same bits.
//   * `plsi_fold_kernel`: all EM steps of a batch of new rows in one launch, the word side Q held fixed (bfh_plsi_fold_in).
//
// Fold-in, per history b with entries (c_j, v_j) and start row p(0):
//     acc_k  = sum_j max(p(t-1)_k * Q[c_j, k], 1e-10f) / norm_j * v_j        norm_j = sum_k max(...)
//     p(t)_k = (acc_k + a1) / sum_k (acc_k + a1)                              a1 = alpha1 / float(d)
// which is one P half-step of the trainer followed by its row normalisation, with Q put back: the row stays in registers from the first
// step to the last, Q rows are gathered with 16-byte loads every step, the result is stored once.  The summation order is the trainer's and a
// function of the row's length alone: a SHORT row is walked front to back by one lane group; any other row is cut into segments of kPlsiSeg
// entries, each walked by the 64 / G groups of a wave round-robin and combined by the xor butterfly, and the segments' partial rows are added
// in segment order.  Here ONE wave walks all segments of its row one after the other (the trainer spreads them over waves and adds slabs),
// so a row never leaves its wave, and after the butterfly every group of the wave holds the same sums and normalises them redundantly.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace bfh {

constexpr int kPlsiSeg = 2048;   // entries of one segment of a split owner

struct PlsiItem {
    int32_t owner;
    int32_t dest;   // half-step: -1: the owner's row of own_new, otherwise a slab index; fold-in: unused (-1)
    int64_t beg, end;
};

template <int G>
__device__ __forceinline__ float plsi_group_sum(float v) {
#pragma unroll
    for (int m = 1; m < G; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// entries in flight per lane group
template <int C>
struct PlsiUnroll {
    static constexpr int value = C == 1 ? 4 : 2;
};

// One lane group over entries first, first + stride, ... < end of (keys, vals): acc += max(own * other[key], 1e-10) / norm * v per entry, in that
// order; lacc -= log(norm) * v (LOSS builds).  Lane `lig` of the group holds columns (c * G + lig) * 4 .. + 3 of chunk c.
template <int G, int C, bool LOSS>
__device__ __forceinline__ void plsi_walk_entries(const float (&own)[C][4], const bool (&valid)[C][4], const bool (&in_row)[C], float (&acc)[C][4], double& lacc,
                                                  const float* other_old, const int32_t* keys, const float* vals, int64_t first, int64_t end, int stride,
                                                  int vdim, int lig) {
#pragma clang fp contract(off)   // every fused operation below is written out: the compiler's choice would differ from kernel to kernel
    constexpr int U = PlsiUnroll<C>::value;
    for (int64_t j = first; j < end; j += static_cast<int64_t>(stride) * U) {
        int32_t key[U];
        float v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {   // a slot past the end adds exactly +0 (v = 0) from row 0
            const int64_t jj = j + static_cast<int64_t>(u) * stride;
            const bool ok = jj < end;
            key[u] = ok ? keys[jj] : 0;
            v[u] = ok ? vals[jj] : 0.f;
        }
        float4 o[U][C];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int c = 0; c < C; ++c) {
                o[u][c] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (in_row[c]) o[u][c] = *reinterpret_cast<const float4*>(other_old + static_cast<size_t>(key[u]) * vdim + (c * G + lig) * 4);
            }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float lat[C][4];
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float ov[4] = {o[u][c].x, o[u][c].y, o[u][c].z, o[u][c].w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    lat[c][e] = valid[c][e] ? fmaxf(own[c][e] * ov[e], 1e-10f) : 0.f;
                    s += lat[c][e];
                }
            }
            s = plsi_group_sum<G>(s);
            const float scale = v[u] / s;
#pragma unroll
            for (int c = 0; c < C; ++c)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[c][e] = __builtin_fmaf(lat[c][e], scale, acc[c][e]);
            if (LOSS) lacc = __builtin_fma(-static_cast<double>(logf(s)), static_cast<double>(v[u]), lacc);
        }
    }
}

// The 64 / G groups of a wave hold disjoint entries of one segment: xor butterfly, commutative at every stage, so every lane ends with the same bits
template <int G, int C>
__device__ __forceinline__ void plsi_team_sum(float (&acc)[C][4]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int m = G; m < 64; m <<= 1)
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[c][e] += __shfl_xor(acc[c][e], m, 64);
}

// plsi.cc:113-116 on the row a lane group holds: x += add; x /= sum(x) over the columns < d (the others become 0 before the division)
template <int G, int C>
__device__ __forceinline__ void plsi_normalize_row(float (&x)[C][4], int d, int lig, float add) {
#pragma clang fp contract(off)
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int col = (c * G + lig) * 4;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            x[c][e] = col + e < d ? x[c][e] + add : 0.f;
            s += x[c][e];
        }
    }
    s = plsi_group_sum<G>(s);
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) x[c][e] = x[c][e] / s;
}

// ---- fold-in --------------------------------------------------------------------------------------------------------------------------------

struct PlsiFoldArgs {
    const float* Q;          // [Q_rows, vdim], the old model's word side
    const float* init;       // [n_rows, vdim] start rows, or nullptr: every column < d starts at `uniform`
    float* out;              // [n_rows, vdim]; columns >= d are written 0
    double* loss;            // [n_rows] (LOSS builds): -sum_j log(norm_j) v_j of the last step
    const int32_t* keys;
    const float* vals;
    const PlsiItem* items;   // short rows first (one lane group each), then the others (one wave each)
    int n_short, n_team, d, vdim, iters;
    float a1, uniform;       // alpha1 / float(d), 1.0f / float(d): host values, the ones the trainer's callers have
};

// One EM step of the row the lane group (short) or the wave (team) holds: p <- normalised sums from p.  -> the row's loss term of this step.
template <int G, int C, bool LOSS>
__device__ __forceinline__ double plsi_fold_step(const PlsiFoldArgs& a, const PlsiItem& it, bool team, int grp, int lig, float (&p)[C][4],
                                                 const bool (&valid)[C][4], const bool (&in_row)[C]) {
#pragma clang fp contract(off)
    constexpr int NG = 64 / G;
    float acc[C][4];
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[c][e] = 0.f;
    double lacc = 0.0;
    if (!team) {
        plsi_walk_entries<G, C, LOSS>(p, valid, in_row, acc, lacc, a.Q, a.keys, a.vals, it.beg, it.end, 1, a.vdim, lig);
    } else {
        for (int64_t s0 = it.beg; s0 < it.end; s0 += kPlsiSeg) {   // wave-uniform: the segments in order
            const int64_t s1 = s0 + kPlsiSeg < it.end ? s0 + kPlsiSeg : it.end;
            float part[C][4];
#pragma unroll
            for (int c = 0; c < C; ++c)
#pragma unroll
                for (int e = 0; e < 4; ++e) part[c][e] = 0.f;
            plsi_walk_entries<G, C, LOSS>(p, valid, in_row, part, lacc, a.Q, a.keys, a.vals, s0 + grp, s1, NG, a.vdim, lig);
            plsi_team_sum<G, C>(part);
#pragma unroll
            for (int c = 0; c < C; ++c)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[c][e] = s0 == it.beg ? part[c][e] : acc[c][e] + part[c][e];
        }
        if (LOSS) {
#pragma unroll
            for (int m = G; m < 64; m <<= 1) lacc += __shfl_xor(lacc, m, 64);
        }
    }
    plsi_normalize_row<G, C>(acc, a.d, lig, a.a1);
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) p[c][e] = acc[c][e];
    return lacc;
}

// Wave w < ceil(n_short / NG): its NG lane groups take NG short rows; the waves behind take one row each.  No float atomic, no LDS.
template <int G, int C, bool LOSS>
__global__ __launch_bounds__(256) void plsi_fold_kernel(const PlsiFoldArgs a) {
    constexpr int NG = 64 / G;
    const int lane = threadIdx.x & 63, lig = lane & (G - 1), grp = lane / G;
    const int w = static_cast<int>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    const int n_short_waves = (a.n_short + NG - 1) / NG;
    if (w >= n_short_waves + a.n_team) return;   // wave-uniform
    const bool team = w >= n_short_waves;
    const int idx = team ? a.n_short + (w - n_short_waves) : w * NG + grp;
    const bool active = team || idx < a.n_short;
    PlsiItem it{0, -1, 0, 0};   // an idle group walks nothing and stores nothing
    if (active) it = a.items[idx];

    bool in_row[C];
    bool valid[C][4];
    float p[C][4];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int col = (c * G + lig) * 4;
        in_row[c] = col < a.vdim;
        float4 o = make_float4(a.uniform, a.uniform, a.uniform, a.uniform);
        if (a.init && in_row[c]) o = *reinterpret_cast<const float4*>(a.init + static_cast<size_t>(it.owner) * a.vdim + col);
        const float ov[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            valid[c][e] = col + e < a.d;
            p[c][e] = valid[c][e] ? ov[e] : 0.f;
        }
    }
    for (int t = 1; t < a.iters; ++t) (void)plsi_fold_step<G, C, false>(a, it, team, grp, lig, p, valid, in_row);
    const double loss = plsi_fold_step<G, C, LOSS>(a, it, team, grp, lig, p, valid, in_row);

    if (active && (!team || grp == 0)) {
        float* out = a.out + static_cast<size_t>(it.owner) * a.vdim;
#pragma unroll
        for (int c = 0; c < C; ++c)   // the padding columns are 0 even where the row is 0 / 0 (alpha1 = 0 and no entries)
            if (in_row[c])
                *reinterpret_cast<float4*>(out + (c * G + lig) * 4) =
                    make_float4(valid[c][0] ? p[c][0] : 0.f, valid[c][1] ? p[c][1] : 0.f, valid[c][2] ? p[c][2] : 0.f, valid[c][3] ? p[c][3] : 0.f);
        if (LOSS && lig == 0) a.loss[it.owner] = loss;
    }
}

}  // namespace bfh
