// The device code of the SGD base (BPRMF and WARP): row ids of a staged chunk, the epoch-end optimizer pass, the item-side
// gradient gather and the elementwise kernels of the rank exchange, each with its launcher.  Included by sgd_base.hip only.
#pragma once
#include "sgd_base.hpp"

namespace bfh {

// ------------------------------------------------------------------------------------------------
// fill_rows: row id of every nnz of a chunk (cf. fill_rows_kernel, /root/reference/lib/cuda/bpr/
// bpr.cu:22-33, which runs one thread per block).  One thread per nnz, binary search in indptr.
// ------------------------------------------------------------------------------------------------
__global__ void fill_rows_kernel(const int64_t* __restrict__ indptr, int start_x, int next_x, int64_t shift, int64_t n,
                                 int32_t* __restrict__ rows) {
    const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int64_t g = shift + t;
    // first row u in [start_x, next_x) with indptr[u] > g
    int lo = start_x, hi = next_x;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (indptr[mid] <= g) lo = mid + 1;
        else hi = mid;
    }
    rows[t] = lo;
}

static void launch_fill_rows(const int64_t* indptr, int start_x, int next_x, int64_t shift, int64_t n, int32_t* rows, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(fill_rows_kernel, dim3(blocks_of(n)), dim3(256), 0, s, indptr, start_x, next_x, shift, n, rows);
    BFH_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------
// Epoch-end optimizer pass: SGDAlgorithm::update_parameters / update_adam / update_adagrad
// (/root/reference/lib/algo.cc:365-465) fused with CWARP's unit-ball projection
// (/root/reference/lib/algo_impl/warp/warp.cc:192-201).  Pure streaming: (3 or 4) arrays read +
// written once.  Quirks kept: grad keeps the transformed step (Q-6), FEPS outside the sqrt (Q-5).
// A row is handled by G = 64/RPW lanes, float4 per lane.
// ------------------------------------------------------------------------------------------------
struct OptConsts {
    float reg2, lr, b1, omb1, b2, omb2, c1, c2;
};

__device__ __forceinline__ float group_sum(float v, int G) {
    for (int s = 1; s < G; s <<= 1) v += __shfl_xor(v, s, 64);
    return v;
}

template <bool ADAM>
__device__ __forceinline__ void opt_step4(float4& x, float4& g, float4& m, float4& v, bool has_cnt, float cntf,
                                          const OptConsts& k, float& nrm) {
    const float FEPS = 1e-10f;
    float* xp = reinterpret_cast<float*>(&x);
    float* gp = reinterpret_cast<float*>(&g);
    float* vp = reinterpret_cast<float*>(&v);
    float* mp = reinterpret_cast<float*>(&m);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float ge = gp[e];
        if (has_cnt) ge = ge / cntf;
        ge = ge - xp[e] * k.reg2;
        if (ADAM) {
            mp[e] = k.b1 * mp[e] + k.omb1 * ge;
            vp[e] = k.b2 * vp[e] + k.omb2 * (ge * ge);
            const float m_hat = mp[e] / k.c1;
            const float v_hat = vp[e] / k.c2;
            ge = m_hat / (sqrtf(v_hat) + FEPS);
        } else {
            vp[e] = vp[e] + ge * ge;
            ge = ge / (sqrtf(vp[e]) + FEPS);
        }
        gp[e] = ge;
        xp[e] = xp[e] + k.lr * ge;
        nrm += xp[e] * xp[e];
    }
}

template <bool ADAM, bool PROJECT>
__global__ __launch_bounds__(256) void sgd_update_rows_kernel(float* __restrict__ X, float* __restrict__ grad,
                                                               float* __restrict__ mom, float* __restrict__ vel,
                                                               const int* __restrict__ cnt, int rows, int vdim, int G,
                                                               OptConsts k) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int rpw = 64 / G;
    const int row = wave * rpw + lane / G;
    const int gl = lane % G;
    const bool active = row < rows;
    float nrm = 0.f;
    float cntf = 1.f;
    bool has_cnt = false;
    if (active && cnt) {
        const int c = cnt[row];
        has_cnt = c != 0;
        cntf = static_cast<float>(c);
    }
    if (vdim <= G * 4) {
        // one float4 per lane: the row stays in registers between the step and the projection
        const bool has = active && gl * 4 < vdim;
        const size_t o = static_cast<size_t>(active ? row : 0) * vdim + gl * 4;
        float4 x = make_float4(0, 0, 0, 0), g = x, v = x, m = x;
        if (has) {
            x = *reinterpret_cast<float4*>(X + o);
            g = *reinterpret_cast<float4*>(grad + o);
            v = *reinterpret_cast<float4*>(vel + o);
            if (ADAM) m = *reinterpret_cast<float4*>(mom + o);
            opt_step4<ADAM>(x, g, m, v, has_cnt, cntf, k, nrm);
            *reinterpret_cast<float4*>(grad + o) = g;
            *reinterpret_cast<float4*>(vel + o) = v;
            if (ADAM) *reinterpret_cast<float4*>(mom + o) = m;
        }
        if (PROJECT) {
            nrm = group_sum(nrm, G);
            const float dn = fmaxf(1.0f, sqrtf(nrm));
            x.x /= dn; x.y /= dn; x.z /= dn; x.w /= dn;
        }
        if (has) *reinterpret_cast<float4*>(X + o) = x;
        return;
    }
    // vdim > 256: G == 64, several float4 per lane; projection needs a second pass over the row
    if (active) {
        for (int c = gl * 4; c < vdim; c += G * 4) {
            const size_t o = static_cast<size_t>(row) * vdim + c;
            float4 x = *reinterpret_cast<float4*>(X + o);
            float4 g = *reinterpret_cast<float4*>(grad + o);
            float4 v = *reinterpret_cast<float4*>(vel + o);
            float4 m = make_float4(0, 0, 0, 0);
            if (ADAM) m = *reinterpret_cast<float4*>(mom + o);
            opt_step4<ADAM>(x, g, m, v, has_cnt, cntf, k, nrm);
            *reinterpret_cast<float4*>(grad + o) = g;
            *reinterpret_cast<float4*>(vel + o) = v;
            if (ADAM) *reinterpret_cast<float4*>(mom + o) = m;
            *reinterpret_cast<float4*>(X + o) = x;
        }
    }
    if (PROJECT) {
        nrm = group_sum(nrm, G);
        if (active) {
            const float dn = fmaxf(1.0f, sqrtf(nrm));
            for (int c = gl * 4; c < vdim; c += G * 4) {
                const size_t o = static_cast<size_t>(row) * vdim + c;
                float4 x = *reinterpret_cast<float4*>(X + o);
                x.x /= dn; x.y /= dn; x.z /= dn; x.w /= dn;
                *reinterpret_cast<float4*>(X + o) = x;
            }
        }
    }
}

// bias column Qb[I,1]: thread per item (lib/algo.cc:415-419, 448-452)
template <bool ADAM>
__global__ void sgd_update_bias_kernel(float* __restrict__ X, float* __restrict__ grad, float* __restrict__ mom,
                                       float* __restrict__ vel, const int* __restrict__ cnt, int rows, bool use_bias,
                                       OptConsts k) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    const float FEPS = 1e-10f;
    float g = grad[i];
    if (cnt && cnt[i]) g = g / static_cast<float>(cnt[i]);  // Q-9: divided even without use_bias
    if (use_bias) {
        g = g - X[i] * k.reg2;
        if (ADAM) {
            const float m = k.b1 * mom[i] + k.omb1 * g;
            const float v = k.b2 * vel[i] + k.omb2 * (g * g);
            mom[i] = m;
            vel[i] = v;
            g = (m / k.c1) / (sqrtf(v / k.c2) + FEPS);
        } else {
            const float v = vel[i] + g * g;
            vel[i] = v;
            g = g / (sqrtf(v) + FEPS);
        }
        X[i] = X[i] + k.lr * g;
    }
    grad[i] = g;
}

// ------------------------------------------------------------------------------------------------
// grad_gather_kernel: the item side of gradient accumulation (see GatherParams in sgd_base.hpp).
// A wave owns kGatherChunk consecutive incidences of the item-sorted list.  Per 64 incidences the lanes
// fetch (item, index) coalesced and the (user, coefficient) record of the triple with one 8-byte gather;
// the wave then walks them with UN user rows in flight (dword per lane: element k*64+lane, so every load and
// every flushed atomic covers whole 128-B lines), sums  c * P[u]  in registers while the item stays the same
// and pushes the run with one atomic row add.  Bound: HBM / Infinity-Cache gathers of 4*vdim bytes per incidence.
// ------------------------------------------------------------------------------------------------
constexpr int kGatherChunk = 256;

template <int K, int UN, bool QTERM>
__global__ __launch_bounds__(256) void grad_gather_kernel(GatherParams g) {
    const int lane = threadIdx.x & 63;
    const int wpb = blockDim.x >> 6;
    const int64_t wave0 = static_cast<int64_t>(blockIdx.x) * wpb + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t nwaves = static_cast<int64_t>(gridDim.x) * wpb;
    const int vdim = g.vdim;
    const int64_t n_work = (g.n + kGatherChunk - 1) / kGatherChunk;
    for (int64_t w = wave0; w < n_work; w += nwaves) {
        const int64_t k_beg = w * kGatherChunk;
        const int64_t k_end = (k_beg + kGatherChunk < g.n) ? k_beg + kGatherChunk : g.n;
        int cur = -1, cnt = 0;
        float csum = 0.f;
        float acc[K];
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] = 0.f;
        auto flush = [&]() {
            if (cur >= 0 && cnt > 0) {
                float* dst = g.gradQ + static_cast<size_t>(cur) * vdim;
                const float qs = g.a * csum + g.b * static_cast<float>(cnt);
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const int e = k * 64 + lane;
                    if (e < vdim) {
                        float v = g.sign * acc[k];
                        if (QTERM) v += qs * g.Q[static_cast<size_t>(cur) * vdim + e];
                        atomic_add_f32(dst + e, v);
                    }
                }
                if (lane == 0) {
                    if (g.gradQb) atomic_add_f32(g.gradQb + cur, g.sign * csum);
                    if (g.cntQ) atomicAdd(g.cntQ + cur, cnt);
                }
            }
#pragma unroll
            for (int k = 0; k < K; ++k) acc[k] = 0.f;
            csum = 0.f;
            cnt = 0;
        };
        for (int64_t k0 = k_beg; k0 < k_end; k0 += 64) {
            const int64_t kk = k0 + lane;
            int my_item = -1, my_u = -1;
            float my_c = 0.f;
            if (kk < k_end) {
                const uint32_t it = g.inc_key[kk];
                if (it < static_cast<uint32_t>(g.Q_rows)) {
                    const int32_t idx = g.inc_idx[kk];
                    bool any = false;
                    // one 8-byte gather carries the user and the coefficient (negative = rejected: BPR / WARP coefficients are >= 0 by
                    // construction -- sigmoid / log of a count; a NaN of a diverged model is NOT negative and propagates like in the reference)
                    const int64_t base = g.pos_list ? static_cast<int64_t>(idx) * g.num_neg : static_cast<int64_t>(idx);
                    const int slots = g.pos_list ? g.num_neg : 1;
                    for (int sl = 0; sl < slots; ++sl) {
                        const float2 v = g.uc[base + sl];
                        if (!(v.y < 0.f)) {
                            my_c += v.y;
                            my_u = __builtin_bit_cast(int, v.x);
                            any = true;
                        }
                    }
                    if (any) my_item = static_cast<int>(it);
                }
            }
            const int n_here = static_cast<int>((k_end - k0) < 64 ? (k_end - k0) : 64);
            for (int j0 = 0; j0 < n_here; j0 += UN) {
                float r[UN][K];
#pragma unroll
                for (int s = 0; s < UN; ++s) {
                    const int u = __builtin_amdgcn_readlane(my_u, (j0 + s) & 63);
                    if (u >= 0) {
                        const float* src = g.P + static_cast<size_t>(u) * vdim;
#pragma unroll
                        for (int k = 0; k < K; ++k) {
                            const int e = k * 64 + lane;
                            r[s][k] = e < vdim ? src[e] : 0.f;
                        }
                    }
                }
#pragma unroll
                for (int s = 0; s < UN; ++s) {
                    const int u = __builtin_amdgcn_readlane(my_u, (j0 + s) & 63);
                    if (u >= 0) {
                        const int item = __builtin_amdgcn_readlane(my_item, (j0 + s) & 63);
                        if (item != cur) {
                            flush();
                            cur = item;
                        }
                        const float c = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, my_c), (j0 + s) & 63));
#pragma unroll
                        for (int k = 0; k < K; ++k) acc[k] += c * r[s][k];
                        csum += c;
                        cnt += 1;
                    }
                }
            }
        }
        flush();
    }
}

// idx[t] = t  (the payload of the incidence sorts: entry t of the unsorted list)
__global__ __launch_bounds__(256) void incidence_iota_kernel(int64_t n, int32_t* __restrict__ idx_out) {
    const int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (t >= n) return;
    idx_out[t] = static_cast<int32_t>(t);
}

// per_coordinate_normalize counts of a list that is not gathered (update_i / update_j == false still count: bpr.cc:139-143, 175-181)
__global__ __launch_bounds__(256) void incidence_count_kernel(const uint32_t* __restrict__ item, int64_t n, int q_rows, int* __restrict__ cnt) {
    const int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (t < n && item[t] < static_cast<uint32_t>(q_rows)) atomicAdd(cnt + item[t], 1);
}

static void launch_incidence_iota(int64_t n, int32_t* idx_out, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(incidence_iota_kernel, dim3(blocks_of(n)), dim3(256), 0, s, n, idx_out);
    BFH_HIP(hipGetLastError());
}

static void launch_incidence_count(const uint32_t* item, int64_t n, int q_rows, int* cnt, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(incidence_count_kernel, dim3(blocks_of(n)), dim3(256), 0, s, item, n, q_rows, cnt);
    BFH_HIP(hipGetLastError());
}

template <int K, int UN>
static void launch_grad_gather_k(const GatherParams& g, dim3 grid, hipStream_t s) {
    if (g.a != 0.f || g.b != 0.f) hipLaunchKernelGGL((grad_gather_kernel<K, UN, true>), grid, dim3(256), 0, s, g);
    else hipLaunchKernelGGL((grad_gather_kernel<K, UN, false>), grid, dim3(256), 0, s, g);
}

static void launch_grad_gather(const GatherParams& g, int64_t max_waves, hipStream_t s) {
    if (g.n <= 0) return;
    const int64_t n_work = (g.n + kGatherChunk - 1) / kGatherChunk;
    const int64_t waves = std::max<int64_t>(1, std::min(max_waves, n_work));
    const dim3 grid(static_cast<unsigned>((waves + 3) / 4));
    const int K = (g.vdim + 63) / 64;
    if (K <= 1) launch_grad_gather_k<1, 8>(g, grid, s);
    else if (K <= 2) launch_grad_gather_k<2, 8>(g, grid, s);
    else if (K <= 4) launch_grad_gather_k<4, 8>(g, grid, s);
    else if (K <= 8) launch_grad_gather_k<8, 4>(g, grid, s);
    else launch_grad_gather_k<16, 2>(g, grid, s);
    BFH_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------
// Delta exchange between ranks (see sgd_exchange.hpp).  Elementwise streaming kernels over one segment of
// the exchanged pair (the matrix, or its bias column).
// ------------------------------------------------------------------------------------------------
// S = X - Z  (what this rank changed since the state Z every rank agrees on)
__global__ __launch_bounds__(256) void delta_begin_kernel(const float* __restrict__ X, const float* __restrict__ Z, float* __restrict__ S, int64_t n) {
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * 256) S[i] = X[i] - Z[i];
}
// Z <- Z + w R: the agreed state advances by the combined deltas -- the same arithmetic on every rank, so Z stays
// bit-identical.  w (per row, exchange_weight_kernel) interpolates between the SUM of the ranks' deltas (rows that
// received few updates in the interval: the deltas are independent steps) and their MEAN (rows every rank has driven to
// its local equilibrium: the deltas are N estimates of the same move).  X: if this rank kept working since `begin`
// (progressed) its own delta is replaced by the combination, X += w R - S; otherwise X <- Z exactly, which makes the
// replicas bit-identical after a flush.
__global__ __launch_bounds__(256) void delta_finish_kernel(float* __restrict__ X, float* __restrict__ Z, const float* __restrict__ S,
                                                           const float* __restrict__ R, const float* __restrict__ W, int row_len, int64_t n,
                                                           int progressed) {
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * 256) {
        const float r = W[i / row_len] * R[i];
        const float zn = Z[i] + r;
        X[i] = progressed ? X[i] + (r - S[i]) : zn;
        Z[i] = zn;
    }
}
// Row i receives m = upd[i] * share updates per rank in one exchange interval (upd = updates of the row per epoch over all
// ranks, share = this rank's part of the epoch inside the interval).  Under SGD a coordinate with curvature k contracts
// towards its equilibrium by exp(-x), x = lr * k * m; n deltas that started from the same state therefore combine like ONE
// run of n m updates when scaled by  w = (1 - exp(-n x)) / (n (1 - exp(-x))):  w -> 1 for cold rows (the deltas are
// independent steps: SUM), w -> 1/n for saturated ones (n estimates of the same move: MEAN).  Two curvatures: the item
// bias sees the logistic loss itself (k_b = 1/4 at most), a factor row sees reg + sigma' |p|^2 (k_q ~ the regulariser
// while the factors are small).  Measured against the single-process run at BASELINE scale, 8 ranks
// (profiles/r02_local_sgd_study_*): the plain sum leaves |Qb| 4.5x and |Q| 2x too large (lr 0.002) or diverges (lr 0.05);
// with the weights and 4 exchange points per epoch loss, |P|, |Q|, |Qb| land within 0.01 / 0.1 / 3.5 / 1.5 %.
__global__ void exchange_weight_kernel(const int* __restrict__ gcnt, const int64_t* __restrict__ cum, int64_t cum_total, int rows, double pos_scale,
                                       double neg_total, double neg_uniform, const float* __restrict__ summed, double stiff_q, double stiff_b,
                                       int n_ranks, float* __restrict__ W, float* __restrict__ Wb) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    // the ranks' interval sizes and learning rates, summed by the same all-reduce as the deltas: their means are the same
    // numbers on every rank, so W -- and with it Z -- stays bit-identical across the ranks
    const double share = neg_total > 0 ? static_cast<double>(summed[0]) / n_ranks / neg_total : 0.0;
    const double lr = static_cast<double>(summed[1]) / n_ranks;
    double pneg = neg_uniform;
    if (cum) pneg = static_cast<double>(cum[i] - (i ? cum[i - 1] : 0)) / static_cast<double>(cum_total);
    const double m = (gcnt[i] * pos_scale + neg_total * pneg) * share;
    auto weight = [&](double x) { return (n_ranks > 1 && x > 1e-9) ? -expm1(-n_ranks * x) / (n_ranks * -expm1(-x)) : 1.0; };
    W[i] = static_cast<float>(weight(lr * stiff_q * m));
    Wb[i] = static_cast<float>(weight(lr * stiff_b * m));
}
__global__ void exchange_scalars_kernel(float* __restrict__ S, float interval, float lr) {
    S[0] = interval; S[1] = lr; S[2] = 0.f; S[3] = 0.f;
}
// X = Z + R  (gradients: state after the last optimizer step + every rank's accumulation since)
__global__ __launch_bounds__(256) void delta_apply_kernel(float* __restrict__ X, const float* __restrict__ Z, const float* __restrict__ R, int64_t n) {
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * 256) X[i] = Z[i] + R[i];
}

// grid of the grid-stride delta kernels: capped, unlike blocks_of
static inline dim3 stream_grid(int64_t n) { return dim3(static_cast<unsigned>(std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 4096)))); }

}  // namespace bfh
