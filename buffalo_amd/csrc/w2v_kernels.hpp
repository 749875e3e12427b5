// Word2Vec (skip-gram, negative sampling) on gfx950 -- the kernels of w2v.hip.
//
// Lane map of the update.  A pair (input word W[j], output rows W[i] + negatives) is owned by a LANE GROUP of G lanes: G = 16 at
// vdim <= 64 (four groups per wave), 32 at vdim <= 128, the whole wave above that (vdim <= 256).  A lane holds four elements of a row.
// Which four depends on how the rows are written (template flag ATOMIC, the "hogwild_atomic" mode):
//   ATOMIC = false  elements 4 * l .. 4 * l + 3 of lane l: one 16-byte device-coherent load / store per lane and row;
//   ATOMIC = true   elements l, G + l, 2 G + l, 3 G + l: every global_atomic_add_f32 wave-instruction then covers one contiguous
//                   4 * G-byte segment per group instead of every fourth dword of a whole row (a strided add would leave the L2 as four
//                   times as many 64-byte atomic requests); the loads are the matching coherent dword loads.
// Everything between load and store is the same code on the four registers.  Products are formed with contraction off before they
// are added, so a setting gives the same bits under every schedule that has no conflicts.
// A group walks the pairs of ITS work item one after the other, in stream order; the groups of the grid work on different items
// at the same time (Hogwild).  "sequential": group 0 of a single wave walks every item in order.
#pragma once
#include "common.hpp"

// no fused multiply-add from here on: a product is rounded before it is added (the reference's float statements; and what makes
// `row + g * l0` by a plain store and by an atomic add the same bits)
#pragma clang fp contract(off)

namespace bfh {

constexpr int kW2vTable = 1000;           // EXP_TABLE_SIZE of the reference
constexpr uint32_t kW2vStreamSub = 2u;     // counter_draw stream ids (buffalo_hip.h lists the layout)
constexpr uint32_t kW2vStreamWin = 3u;
constexpr uint32_t kW2vStreamNeg = 4u;
constexpr uint32_t kW2vMaxRetry = 0xffffu;

// a run of consecutive centres [c0, c1) of the sentence whose kept words are [kb, ke); offsets into the chunk's kept arrays
struct W2vItem {
    int64_t kb, ke, c0, c1;
    double alpha;
};

struct W2vModel {
    float* L0;
    float* L1;
    const int32_t* dist;
    const float* table;   // [kW2vTable] in global memory; the update kernels copy it into LDS
    int V, vdim, window, num_neg, compute_loss;
    uint32_t seed, epoch;
};

// ------------------------------------------------------------------------------------------------
// step a: subsampling.  One wave per sentence, 64 words per trip, order kept by ballot ranks.
// The kept words of a sentence start at the sentence's own offset in the chunk: kept[kb .. sent_end[s]).
// ------------------------------------------------------------------------------------------------
struct W2vSubArgs {
    const int32_t* seq;        // the chunk's words
    const int64_t* ends;       // END offsets of the chunk's sentences (global, as in the caller's indptr)
    int64_t shifted;           // global offset of the chunk's first word
    int num_sents;
    const int32_t* index;      // [index_size] 0 = out of vocabulary, else word id + 1
    int index_size;
    const uint32_t* scale;
    int window;
    uint32_t seed, epoch;
    int32_t* kept;
    int64_t* kept_pos;
    int32_t* window_b;
    int64_t* sent_end;         // chunk-relative END of every sentence's kept run
    int* bad;
};

__global__ __launch_bounds__(256) void w2v_subsample_kernel(const W2vSubArgs a) {
    const int lane = threadIdx.x & 63;
    const int waves = static_cast<int>(gridDim.x) * 4;
    for (int s = static_cast<int>(blockIdx.x) * 4 + (threadIdx.x >> 6); s < a.num_sents; s += waves) {
        const int64_t beg = (s == 0 ? a.shifted : a.ends[s - 1]) - a.shifted, end = a.ends[s] - a.shifted;
        int64_t count = 0;
        for (int64_t t0 = beg; t0 < end; t0 += 64) {
            const int64_t t = t0 + lane;
            bool keep = false;
            int32_t id = 0;
            const uint64_t pos = static_cast<uint64_t>(a.shifted + t);
            if (t < end) {
                const int32_t w = a.seq[t];
                if (w < 0 || w >= a.index_size) *a.bad = 1;
                else if (a.index[w] != 0) {
                    id = a.index[w] - 1;
                    uint32_t o0, o1;
                    counter_draw(a.seed, kW2vStreamSub, pos, 0u, a.epoch, 0u, o0, o1);
                    keep = a.scale[id] > o0;   // w2v.cc:232 drops the word when scale <= r1
                }
            }
            const uint64_t mask = __ballot(keep);
            if (keep) {
                const int64_t out = beg + count + __popcll(mask & ((1ull << lane) - 1ull));
                uint32_t o0, o1;
                counter_draw(a.seed, kW2vStreamWin, pos, 0u, a.epoch, 0u, o0, o1);
                a.kept[out] = id;
                a.kept_pos[out] = static_cast<int64_t>(pos);
                a.window_b[out] = static_cast<int32_t>((static_cast<uint64_t>(o0) * static_cast<uint32_t>(a.window)) >> 32);
            }
            count += __popcll(mask);
        }
        if (lane == 0) a.sent_end[s] = beg + count;
    }
}

// step b, device part: pairs of every sentence = sum over its kept centres of the window's width (w2v.cc:240-245); one wave per sentence
__global__ __launch_bounds__(256) void w2v_pair_count_kernel(const int64_t* __restrict__ ends, int64_t shifted, int num_sents,
                                                             const int64_t* __restrict__ sent_end, const int32_t* __restrict__ window_b, int window,
                                                             int64_t* __restrict__ pairs) {
    const int lane = threadIdx.x & 63;
    const int waves = static_cast<int>(gridDim.x) * 4;
    for (int s = static_cast<int>(blockIdx.x) * 4 + (threadIdx.x >> 6); s < num_sents; s += waves) {
        const int64_t kb = (s == 0 ? shifted : ends[s - 1]) - shifted, n = sent_end[s] - kb;
        int cnt = 0;
        for (int64_t i = lane; i < n; i += 64) {
            const int64_t b = window_b[kb + i];
            const int64_t lo = max(static_cast<int64_t>(0), i - window + b), hi = min(n, i + window + 1 - b);
            cnt += static_cast<int>(hi - lo - 1);
        }
        int64_t total = cnt;   // a lane sees at most ceil(n / 64) * 254 pairs
        for (int m = 1; m < 64; m <<= 1) total += __shfl_xor(total, m, 64);
        if (lane == 0) pairs[s] = total;
    }
}

// ------------------------------------------------------------------------------------------------
// step c: the update
// ------------------------------------------------------------------------------------------------
using w2v_b128_t = decltype(__builtin_amdgcn_raw_buffer_load_b128(__amdgpu_buffer_rsrc_t(), 0, 0, 0));
struct W2vQuad { float v[4]; };

// sum over the G lanes of a group; every lane of the group receives the same bits
template <int G>
__device__ __forceinline__ float w2v_group_sum(float v) {
    if constexpr (G == 64) return wave_sum(v);
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xf, 0xf, false));  // row_ror:8
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x124, 0xf, 0xf, false));  // row_ror:4
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x122, 0xf, 0xf, false));  // row_ror:2
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x121, 0xf, 0xf, false));  // row_ror:1
    if constexpr (G == 32) v += __shfl_xor(v, 16, 64);
    return v;
}

// device-coherent row I/O (sc1: past the CU's L1, written through the L2), as the BPRMF walk moves its shared item rows
template <int G, bool ATOMIC>
__device__ __forceinline__ void w2v_row_load(W2vQuad& r, const float* base, int lig, int vdim) {
    if constexpr (ATOMIC) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int e = k * G + lig;
            r.v[k] = e < vdim ? __hip_atomic_load(base + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
        }
    } else {   // the descriptor's range check (num_records = the row's bytes) gives the lanes beyond vdim zeros
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, vdim * 4, 0x00020000);
        r = __builtin_bit_cast(W2vQuad, __builtin_amdgcn_raw_buffer_load_b128(rs, lig * 16, 0, 16));
    }
}
// row += delta, where `row` holds the bits this group loaded: atomics add delta in memory, plain stores write row + delta
template <int G, bool ATOMIC>
__device__ __forceinline__ void w2v_row_add(const W2vQuad& row, const W2vQuad& delta, float* base, int lig, int vdim) {
    if constexpr (ATOMIC) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int e = k * G + lig;
            if (e < vdim) atomic_add_f32(base + e, delta.v[k]);
        }
    } else {
        W2vQuad n;
#pragma unroll
        for (int k = 0; k < 4; ++k) n.v[k] = row.v[k] + delta.v[k];
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(base, 0, vdim * 4, 0x00020000);
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(w2v_b128_t, n), rs, lig * 16, 0, 16);
    }
}

// one pair of update_parameter (w2v.cc:274-320): begin -> visit per output row -> end
struct W2vPair {
    W2vQuad l0, work;
    double loss;
};

template <int G, bool ATOMIC>
__device__ __forceinline__ void w2v_pair_begin(W2vPair& p, const W2vModel& m, int input, int lig) {
    w2v_row_load<G, ATOMIC>(p.l0, m.L0 + static_cast<size_t>(input) * m.vdim, lig, m.vdim);
#pragma unroll
    for (int k = 0; k < 4; ++k) p.work.v[k] = 0.f;
}

template <int G, bool ATOMIC>
__device__ __forceinline__ void w2v_pair_visit(W2vPair& p, const W2vModel& m, const float* s_table, int out_row, bool target, double alpha, int lig) {
    float* base = m.L1 + static_cast<size_t>(out_row) * m.vdim;
    W2vQuad row;
    w2v_row_load<G, ATOMIC>(row, base, lig, m.vdim);
    const float part = (row.v[0] * p.l0.v[0] + row.v[1] * p.l0.v[1]) + (row.v[2] * p.l0.v[2] + row.v[3] * p.l0.v[3]);
    const float f = w2v_group_sum<G>(part);   // the same bits in every lane of the group
    const float label = target ? 1.f : 0.f;
    float g;
    if (f > 6.f) g = label - 1.f;
    else if (f < -6.f) g = label;
    else g = label - s_table[min(max(static_cast<int>((f + 6.f) * 83.f), 0), kW2vTable - 1)];   // the clamp only matters for a NaN dot
    if (m.compute_loss) {   // w2v.cc:304-309
        const double eps = static_cast<double>(1e-8f);
        p.loss -= target ? log(static_cast<double>(g) + eps) : log(1.0 - static_cast<double>(g) + eps);
    }
    g = static_cast<float>(static_cast<double>(g) * alpha);   // `g *= alpha` with a float g and a double alpha
    W2vQuad delta;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        p.work.v[k] = p.work.v[k] + g * row.v[k];
        delta.v[k] = g * p.l0.v[k];
    }
    w2v_row_add<G, ATOMIC>(row, delta, base, lig, m.vdim);
}

template <int G, bool ATOMIC>
__device__ __forceinline__ void w2v_pair_end(const W2vPair& p, const W2vModel& m, int input, int lig) {
    w2v_row_add<G, ATOMIC>(p.l0, p.work, m.L0 + static_cast<size_t>(input) * m.vdim, lig, m.vdim);
}

// negative `k` of the pair (centre position pos, slot): lower_bound(dist, V, r3), redrawn while it is the target (w2v.cc:248-256)
__device__ __forceinline__ int w2v_draw_negative(const W2vModel& m, uint64_t pos, uint32_t slot, uint32_t k, int target, int& redraws) {
    const uint32_t total = static_cast<uint32_t>(m.dist[m.V - 1]);
    int neg = 0;
    for (uint32_t retry = 0;; ++retry) {
        uint32_t o0, o1;
        counter_draw(m.seed, kW2vStreamNeg, pos, slot, m.epoch, (k << 16) | retry, o0, o1);
        const int32_t r3 = static_cast<int32_t>((static_cast<uint64_t>(o0) * total) >> 32);
        neg = static_cast<int>(lower_bound_dev<int32_t>(m.dist, m.V, r3));
        if (neg != target || retry == kW2vMaxRetry) break;   // the reference loops forever
        ++redraws;
    }
    return neg;
}

struct W2vUpdateArgs {
    W2vModel m;
    const W2vItem* items;
    int64_t num_items;
    const int32_t* kept;
    const int64_t* kept_pos;
    const int32_t* window_b;
    double* item_loss;      // [num_items]
    int64_t* item_redraws;  // [num_items]
    int sequential;
};

template <int G, bool ATOMIC>
__global__ __launch_bounds__(256) void w2v_update_kernel(const W2vUpdateArgs a) {
    constexpr int NG = 64 / G;
    __shared__ float s_table[kW2vTable];
    for (int t = threadIdx.x; t < kW2vTable; t += blockDim.x) s_table[t] = a.m.table[t];
    __syncthreads();
    const int lane = threadIdx.x & 63, lig = lane & (G - 1), grp = lane / G;
    const W2vModel& m = a.m;
    int64_t item, stride;
    if (a.sequential) {   // launched as one wave
        item = grp == 0 ? 0 : a.num_items;
        stride = 1;
    } else {
        item = (static_cast<int64_t>(blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6)) * NG + grp;
        stride = static_cast<int64_t>(gridDim.x) * (blockDim.x >> 6) * NG;
    }
    for (; item < a.num_items; item += stride) {
        const W2vItem it = a.items[item];
        const int64_t n = it.ke - it.kb;
        W2vPair p;
        p.loss = 0.0;
        int redraws = 0;
        for (int64_t c = it.c0; c < it.c1; ++c) {
            const int64_t i = c - it.kb;
            const int target = a.kept[c];
            const uint64_t pos = static_cast<uint64_t>(a.kept_pos[c]);
            const int64_t b = a.window_b[c];
            const int64_t lo = max(static_cast<int64_t>(0), i - m.window + b), hi = min(n, i + m.window + 1 - b);
            for (int64_t j = lo; j < hi; ++j) {
                if (j == i) continue;
                const int input = a.kept[it.kb + j];
                const uint32_t slot = static_cast<uint32_t>(j - i + m.window);
                w2v_pair_begin<G, ATOMIC>(p, m, input, lig);
                w2v_pair_visit<G, ATOMIC>(p, m, s_table, target, true, it.alpha, lig);
                // the first 16 lanes of the group draw 16 negatives side by side, then the group visits them in order
                for (int k0 = 0; k0 < m.num_neg; k0 += 16) {
                    const int kn = min(16, m.num_neg - k0);
                    int mine = 0, mine_redraws = 0;
                    if ((lig & 15) < kn) mine = w2v_draw_negative(m, pos, slot, static_cast<uint32_t>(k0 + (lig & 15)), target, mine_redraws);
                    if (lig < kn) redraws += mine_redraws;
                    for (int k = 0; k < kn; ++k) {
                        const int neg = __shfl(mine, grp * G + k, 64);
                        w2v_pair_visit<G, ATOMIC>(p, m, s_table, neg, false, it.alpha, lig);
                    }
                }
                w2v_pair_end<G, ATOMIC>(p, m, input, lig);
            }
        }
        int64_t r = redraws;
#pragma unroll
        for (int msk = 1; msk < G; msk <<= 1) r += __shfl_xor(r, msk, 64);
        if (lig == 0) {
            a.item_loss[item] = p.loss;
            a.item_redraws[item] = r;
        }
    }
}

// bfh_w2v_update_pairs: explicit pairs, in order, through the same update code; one wave, group 0
struct W2vPairsArgs {
    W2vModel m;
    int64_t n;
    const int32_t* inputs;
    const int32_t* outputs;   // [n, n_out], target first
    int n_out;
    double alpha;
    double* loss;
};
template <int G, bool ATOMIC>
__global__ __launch_bounds__(64) void w2v_pairs_kernel(const W2vPairsArgs a) {
    __shared__ float s_table[kW2vTable];
    for (int t = threadIdx.x; t < kW2vTable; t += blockDim.x) s_table[t] = a.m.table[t];
    __syncthreads();
    const int lane = threadIdx.x & 63, lig = lane & (G - 1);
    if (lane >= G) return;
    W2vPair p;
    p.loss = 0.0;
    for (int64_t q = 0; q < a.n; ++q) {
        const int input = a.inputs[q];
        w2v_pair_begin<G, ATOMIC>(p, a.m, input, lig);
        for (int k = 0; k < a.n_out; ++k) w2v_pair_visit<G, ATOMIC>(p, a.m, s_table, a.outputs[q * a.n_out + k], k == 0, a.alpha, lig);
        w2v_pair_end<G, ATOMIC>(p, a.m, input, lig);
    }
    if (lane == 0) a.loss[0] = p.loss;
}

// out[0] = sum of loss[0, n), out_r[0] = sum of redraws[0, n), both in a fixed order (thread t adds t, t + 256, ...; then a tree); one block
__global__ __launch_bounds__(256) void w2v_item_sum_kernel(const double* __restrict__ loss, const int64_t* __restrict__ redraws, int64_t n,
                                                           double* __restrict__ out, int64_t* __restrict__ out_r) {
    __shared__ double sh[256];
    __shared__ int64_t shr[256];
    double s = 0.0;
    int64_t r = 0;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        s += loss[i];
        r += redraws[i];
    }
    sh[threadIdx.x] = s;
    shr[threadIdx.x] = r;
    __syncthreads();
    for (int m = 128; m > 0; m >>= 1) {
        if (static_cast<int>(threadIdx.x) < m) {
            sh[threadIdx.x] += sh[threadIdx.x + m];
            shr[threadIdx.x] += shr[threadIdx.x + m];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[0] = sh[0];
        out_r[0] = shr[0];
    }
}

}  // namespace bfh
