// eALS fold-in on gfx950 -- the kernels.  EalsHandle::fold_in (eals_handle.hpp) launches them; the rule is stated at bfh_eals_fold_in in
// include/buffalo_hip.h: the coordinate descent of CEALS::update_P_ (eals.cc:199-233) on a row that is not in P, against fixed Q, C and S.
//
// A fold-in runs `iters` sweeps over the same few item rows and nobody reads a mirror, so a history's rows Q[k_j] are gathered ONCE, kept
// on the CU transposed as [dimension][entry], and every sweep runs from there (eals_fold_resident_kernel); the two sums that do not depend
// on p -- b_d = sum_j w_j v_j q_jd and g_d = sum_j m_j q_jd^2 + S_dd + reg -- are formed once per history, so a coordinate step is one pass
// over the entries (m_j f_j q_jd), two reductions issued together (that sum, and p . S[:, d] with the lanes over e) and one division:
//     p_d = (b_d - sum_j m_j f_j q_jd - p . S[:, d] + p_d S_dd) / g_d
// This is eals.cc's step with the numerator's p-free part taken out of the loop, hence another rounding order than the trainer's.
// Histories that do not fit stream their rows in blocks of 16 dimensions as eals_update_long_kernel does (eals_fold_stream_kernel).
// All sums are fixed trees (or one thread's loop in entry order) and nothing is atomic but the ticket: a row's bits depend on its own
// entries and on vdim, never on the batch.
#pragma once
#include "eals_kernels.hpp"
#include "fold_group.hpp"

namespace bfh {

struct EalsFoldParams {
    const float* Q;          // [Q_rows, vdim], pad columns zero
    const float* Cw;         // item weights c_i
    const float* S;          // [vdim, vdim] = sum_i c_i q_i q_i^T
    const int64_t* indptr;   // END offsets of the call's histories
    const int32_t* keys;
    const float* vals;
    float* rows;             // [n_rows, vdim]: init (or zeros) on entry, the folded rows on return; pad columns zero
    int d, vdim, iters, has_init;
    float alpha, reg;
    const int32_t* row_list; // the histories of this launch ...
    int n_list;              // ... and how many
    int* ticket;             // streamed kernel
};

// ---- the classes: a history's class follows from its own length and vdim alone ----
constexpr int EALS_FOLD_LDS = 64 * 1024;     // bytes of LDS per block: two blocks and more per CU (160 KB) at every vdim
constexpr int EALS_FOLD_BLOCK_EPL = 2;       // entries per lane of the block form
constexpr int EALS_FOLD_BLOCK_MAX = 256 * EALS_FOLD_BLOCK_EPL;
// floats of one lane group that holds `cap` entries: qt [vdim][cap | 1] | w v [cap] | m [cap] | p, b, g, diag S [vdim] each | red [2][4]
__host__ __device__ constexpr int eals_fold_group_floats(int vdim, int cap) { return vdim * (cap | 1) + 2 * cap + 4 * vdim + 8; }
// the longest history the block form keeps resident at this vdim (476 at vdim 32, 243 at 64, 121 at 128, 58 at 256, 11 at 1024)
__host__ __device__ constexpr int eals_fold_resident_max(int vdim) {
    const int cap = (EALS_FOLD_LDS / 4 - 5 * vdim - 8) / (vdim + 2);
    return cap < EALS_FOLD_BLOCK_MAX ? cap : EALS_FOLD_BLOCK_MAX;
}
// G = 16, 32, 64: 64 / G histories per one-wave block, an entry per lane; G = 256: one history per 256-thread block
template <int G>
struct EalsFoldShape {
    static constexpr int TB = G == 256 ? 256 : 64;
    static constexpr int NG = TB / G;
    static constexpr int EPL = G == 256 ? EALS_FOLD_BLOCK_EPL : 1;
    static constexpr int NS = G == 16 ? 12 : G == 32 ? 7 : 4;   // elements of a column of S per lane (vdim <= 192 / 224 / 224 fit; G = 256: vdim <= 1024)
};
// does the one-wave block of G-lane groups fit the budget at this vdim?
static inline bool eals_fold_wave_fits(int G, int vdim) { return (64 / G) * eals_fold_group_floats(vdim, G) * 4 <= EALS_FOLD_LDS; }
// -> 16 / 32 / 64 / 256: the resident kernel's group width, or 0: streamed
static inline int eals_fold_class(int64_t n, int vdim) {
    for (int G = 16; G <= 64; G *= 2)
        if (n <= G && eals_fold_wave_fits(G, vdim)) return G;
    return n <= eals_fold_resident_max(vdim) ? 256 : 0;
}

template <int G>
__device__ __forceinline__ void eals_fold_sync() {
    if constexpr (G == 256) __syncthreads();
    else wave_lds_sync();
}

// Histories whose item rows fit in LDS.  Staging, once: the rows Q[k_j] by 16-byte loads, consecutive lanes along a row, stored transposed as
// qt[e][j] with an odd entry pitch (the stores of one instruction then spread over the banks instead of hitting one); b and g with the lanes
// over the dimensions (a lane walks its dimension's entries in order: no reduction); vhat = init . q with the lanes over the entries.
// Sweeps: everything in LDS and registers, only the column S[:, d] comes from global memory, loaded one step ahead.
template <int G>
__global__ __launch_bounds__(EalsFoldShape<G>::TB) void eals_fold_resident_kernel(EalsFoldParams p, int cap) {
    using Sh = EalsFoldShape<G>;
    constexpr int EPL = Sh::EPL, NS = Sh::NS;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, grp = tid / G, lg = tid % G;
    const int vdim = p.vdim, D = p.d, pitch = cap | 1;
    float* qt = lds + static_cast<size_t>(grp) * eals_fold_group_floats(vdim, cap);
    float* wvs = qt + static_cast<size_t>(vdim) * pitch;
    float* ms = wvs + cap;
    float* ps = ms + cap;
    float* bs = ps + vdim;
    float* gs = bs + vdim;
    float* sd = gs + vdim;
    float* red = sd + vdim;
    const int item = blockIdx.x * Sh::NG + grp;
    const bool live = item < p.n_list;
    const int x = live ? p.row_list[item] : 0;
    const int64_t beg = live ? row_begin(p.indptr, x) : 0;
    const int n = live ? static_cast<int>(p.indptr[x] - beg) : 0;   // n <= cap: the host's classification
    float* prow = p.rows + static_cast<size_t>(x) * vdim;

    // ---- staging ----
    float m[EPL], vh[EPL];
    bool ok[EPL];
#pragma unroll
    for (int s = 0; s < EPL; ++s) {
        const int j = lg + G * s;
        ok[s] = j < n;
        const float v = ok[s] ? p.vals[beg + j] : 0.f;
        const float w = 1.f + p.alpha * v;
        m[s] = ok[s] ? w - p.Cw[p.keys[beg + j]] : 0.f;
        vh[s] = 0.f;
        if (ok[s]) { wvs[j] = w * v; ms[j] = m[s]; }
    }
    for (int e = lg; e < vdim; e += G) {
        ps[e] = live ? prow[e] : 0.f;
        sd[e] = p.S[static_cast<size_t>(e) * vdim + e];
    }
    const int c4 = vdim / 4;
    for (int f = lg; f < n * c4; f += G) {
        const int j = f / c4, c = f - j * c4;
        const float4 v = reinterpret_cast<const float4*>(p.Q + static_cast<size_t>(p.keys[beg + j]) * vdim)[c];
        float* dst = qt + static_cast<size_t>(4 * c) * pitch + j;
        dst[0] = v.x; dst[pitch] = v.y; dst[2 * pitch] = v.z; dst[3 * pitch] = v.w;
    }
    eals_fold_sync<G>();
    for (int e = lg; e < vdim; e += G) {
        const float* qe = qt + static_cast<size_t>(e) * pitch;
        float b = 0.f, g = 0.f;
        for (int j = 0; j < n; ++j) {
            const float q = qe[j];
            b += wvs[j] * q;
            g += ms[j] * q * q;
        }
        bs[e] = b;
        gs[e] = g + sd[e] + p.reg;
    }
    if (p.has_init) {
#pragma unroll
        for (int s = 0; s < EPL; ++s) {
            const int j = lg + G * s;
            float acc = 0.f;
            if (ok[s])
                for (int e = 0; e < D; ++e) acc += ps[e] * qt[static_cast<size_t>(e) * pitch + j];
            vh[s] = acc;
        }
    }
    eals_fold_sync<G>();

    // ---- sweeps ----
    float sc[NS], sn[NS];
#pragma unroll
    for (int r = 0; r < NS; ++r) {
        const int e = lg + G * r;
        sn[r] = e < vdim ? p.S[e] : 0.f;
    }
    for (int it = 0; it < p.iters; ++it) {
        for (int d = 0; d < D; ++d) {
            const float* snext = p.S + static_cast<size_t>(d + 1 < D ? d + 1 : 0) * vdim;   // S is symmetric: row d = column d
            float dot = 0.f;
#pragma unroll
            for (int r = 0; r < NS; ++r) {
                const int e = lg + G * r;
                sc[r] = sn[r];
                sn[r] = e < vdim ? snext[e] : 0.f;
                if (e < vdim) dot += ps[e] * sc[r];
            }
            const float pd = ps[d];
            const float* qd = qt + static_cast<size_t>(d) * pitch;
            float es = 0.f, f[EPL], q[EPL];
#pragma unroll
            for (int s = 0; s < EPL; ++s) {
                q[s] = ok[s] ? qd[lg + G * s] : 0.f;
                f[s] = vh[s] - pd * q[s];
                es += m[s] * f[s] * q[s];
            }
            if constexpr (G == 256) {
                es = wave_sum(es);
                dot = wave_sum(dot);
                if ((tid & 63) == 0) { red[tid >> 6] = es; red[4 + (tid >> 6)] = dot; }
                __syncthreads();
                es = (red[0] + red[1]) + (red[2] + red[3]);
                dot = (red[4] + red[5]) + (red[6] + red[7]);
            } else {
                es = fold_group_sum<G>(es);
                dot = fold_group_sum<G>(dot);
            }
            const float pn = (bs[d] - es - dot + pd * sd[d]) / gs[d];   // the same bits in every lane of the group
            if constexpr (G != 256) wave_lds_sync();
            if (lg == 0) ps[d] = pn;
            eals_fold_sync<G>();   // (G = 256: also closes the reads of red)
#pragma unroll
            for (int s = 0; s < EPL; ++s) vh[s] = f[s] + pn * q[s];
        }
    }
    if (live)
        for (int e = lg; e < D; e += G) prow[e] = ps[e];
}

// Histories that do not fit: one block per history, ticketed longest first.  `scratch`: per history (2 + EALS_DB) * cap floats at
// (2 + EALS_DB) * row_off[item], cap = its length rounded up to 64: m | vhat | Q[key][16 b + dd] as [dd][entry].  Every entry belongs to
// one thread for the whole call, so the scratch needs no barrier.  First pass: b, g (and vhat from init) in blocks of 16 dimensions;
// then the sweeps as eals_update_long_kernel walks them: the 64-byte segment of every entry once per block, a step's closing fold
// carried into the next step's pass.  No mirror, no map.
template <int BS>
__global__ __launch_bounds__(BS) void eals_fold_stream_kernel(EalsFoldParams p, float* __restrict__ scratch, const int64_t* __restrict__ row_off) {
    constexpr int NW = BS / 64;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int D = p.d, vdim = p.vdim;
    float* ps = lds;
    float* bs = ps + vdim;
    float* gs = bs + vdim;
    float* sd = gs + vdim;
    float* red = sd + vdim;   // [2 * EALS_DB][NW]
    while (true) {
        const int item = eals_ticket_block(p.ticket, reinterpret_cast<int*>(red), tid);
        if (item >= p.n_list) break;
        const int x = p.row_list[item];
        const int64_t beg = row_begin(p.indptr, x), n = p.indptr[x] - beg;
        const int64_t cap = ((n + 63) / 64) * 64;
        float* const ms = scratch + static_cast<size_t>(row_off[item]) * (2 + EALS_DB);
        float* const vhs = ms + cap;
        float* const yb = vhs + cap;
        float* prow = p.rows + static_cast<size_t>(x) * vdim;
        __syncthreads();   // everyone has read the ticket out of red
        for (int e = tid; e < vdim; e += BS) {
            ps[e] = prow[e];
            sd[e] = p.S[static_cast<size_t>(e) * vdim + e];
        }
        for (int64_t i = tid; i < n; i += BS) {
            ms[i] = (1.f + p.alpha * p.vals[beg + i]) - p.Cw[p.keys[beg + i]];
            vhs[i] = 0.f;
        }
        __syncthreads();
        for (int db = 0; db < D; db += EALS_DB) {   // b, g, vhat: 16 dimensions per pass over the row
            float pb[EALS_DB], pg[EALS_DB];
#pragma unroll
            for (int dd = 0; dd < EALS_DB; ++dd) pb[dd] = pg[dd] = 0.f;
            for (int64_t i = tid; i < n; i += BS) {
                const float v = p.vals[beg + i], wvv = (1.f + p.alpha * v) * v, mm = ms[i];
                const float4* src = reinterpret_cast<const float4*>(p.Q + static_cast<size_t>(p.keys[beg + i]) * vdim + db);
                float acc = 0.f;
#pragma unroll
                for (int q4 = 0; q4 < EALS_DB / 4; ++q4) {
                    const float4 y4 = src[q4];
                    const float y[4] = {y4.x, y4.y, y4.z, y4.w};
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        pb[4 * q4 + t] += wvv * y[t];
                        pg[4 * q4 + t] += mm * y[t] * y[t];
                        acc += ps[db + 4 * q4 + t] * y[t];
                    }
                }
                if (p.has_init) vhs[i] += acc;
            }
#pragma unroll
            for (int dd = 0; dd < EALS_DB; ++dd) {
                const float b = wave_sum(pb[dd]), g = wave_sum(pg[dd]);
                if (lane == 0) { red[dd * NW + wv] = b; red[(EALS_DB + dd) * NW + wv] = g; }
            }
            __syncthreads();
            if (tid < 2 * EALS_DB) {
                float sum = 0.f;
                for (int w2 = 0; w2 < NW; ++w2) sum += red[tid * NW + w2];
                const int e = db + (tid & (EALS_DB - 1));
                if (tid < EALS_DB) bs[e] = sum;
                else gs[e] = sum + sd[e] + p.reg;
            }
            __syncthreads();
        }
        for (int it = 0; it < p.iters; ++it) {
            for (int db = 0; db < D; db += EALS_DB) {
                for (int64_t i = tid; i < n; i += BS) {
                    const float4* src = reinterpret_cast<const float4*>(p.Q + static_cast<size_t>(p.keys[beg + i]) * vdim + db);
#pragma unroll
                    for (int q4 = 0; q4 < EALS_DB / 4; ++q4) {
                        const float4 v = src[q4];
                        yb[(4 * q4 + 0) * cap + i] = v.x; yb[(4 * q4 + 1) * cap + i] = v.y;
                        yb[(4 * q4 + 2) * cap + i] = v.z; yb[(4 * q4 + 3) * cap + i] = v.w;
                    }
                }
                float pend = 0.f;   // the previous step's new coordinate, still to be folded into vhat
                const int nd = D - db < EALS_DB ? D - db : EALS_DB;
                for (int dd = 0; dd < nd; ++dd) {
                    const int d = db + dd;
                    const float pd = ps[d];
                    const float* yd_ = yb + static_cast<size_t>(dd) * cap;
                    const float* yp_ = yb + static_cast<size_t>(dd > 0 ? dd - 1 : 0) * cap;
                    float es = 0.f;
                    for (int64_t i = tid; i < n; i += BS) {
                        const float yd = yd_[i];
                        float vh = vhs[i];
                        if (dd > 0) vh += pend * yp_[i];
                        const float vf = vh - pd * yd;
                        es += ms[i] * vf * yd;
                        vhs[i] = vf;
                    }
                    float dot = eals_dot_S(ps, p.S, d, vdim, D, tid, BS);
                    es = wave_sum(es);
                    dot = wave_sum(dot);
                    if (lane == 0) { red[wv] = es; red[NW + wv] = dot; }
                    __syncthreads();
                    es = dot = 0.f;
#pragma unroll
                    for (int w2 = 0; w2 < NW; ++w2) { es += red[w2]; dot += red[NW + w2]; }
                    const float pn = (bs[d] - es - dot + pd * sd[d]) / gs[d];
                    if (tid == 0) ps[d] = pn;
                    __syncthreads();   // ps[d] is out, red is free
                    pend = pn;
                }
                const float* yl_ = yb + static_cast<size_t>(nd - 1) * cap;   // close the block: the last step's fold
                for (int64_t i = tid; i < n; i += BS) vhs[i] += pend * yl_[i];
            }
        }
        for (int e = tid; e < D; e += BS) prow[e] = ps[e];
    }
}

}  // namespace bfh
