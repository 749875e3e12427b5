// eALS (element-wise ALS, He et al. SIGIR'16) on gfx950 -- the kernels.  The handle that launches them is in eals_handle.hpp.
//
// Reference semantics: CEALS (/root/reference/lib/algo_impl/eals/eals.cc:33-281) behind CyEALS's surface
// (/root/reference/buffalo/algo/_eals.pyx:23-67); SURVEY.md section 8(f) rank 4.  Coordinate descent over the
// latent dimensions of every row, driven by a cache of the predictions vhat of the observed entries that
// is kept in BOTH orientations and linked by index maps (eals.cc:49-100).
//
// Device formulation: one wave per row (one 1024-thread block above 4096 entries).  The row's entries sit one per lane (up to 4 per lane
// in registers: key, value, vhat, weight; longer rows keep vhat in HBM and a transposed 16-dimension slice of the gathered rows in a
// scratch slot); for every dimension d the lanes form the numerator / denominator terms of eals.cc:196-213 against the gathered column
// element Y[key][d], three wave reductions finish the step (the p.S[:,d] product rides on the numerator), the new coordinate is broadcast
// through LDS and folded back into vhat.  The mirrored cache of the other orientation is written once per row at the end instead of
// twice per (entry, dimension): nobody reads it before the other half-epoch and both copies receive the same +-pq sequence, so the
// stored values are identical.  Arrays are the reference's CPU layout ([rows, d], unpadded); the device copies are padded to vdim so
// the MFMA Gramian kernel of the ALS path serves S^p = P^T P and S^q = sum_i C_i q_i q_i^T.
#pragma once
#include "als_kernels.hpp"

namespace bfh {

struct EalsParams {
    float* X;               // side being updated [rows, vdim]
    const float* Y;         // other side
    const float* Cw;        // item weights c_i [items]
    const float* S;         // [vdim, vdim]: axis 0 -> sum_i C_i q q^T, axis 1 -> P^T P
    const int64_t* indptr;  // END offsets of this orientation
    const int32_t* keys;
    const float* vals;
    float* own;             // vhat cache of this orientation
    float* other;           // vhat cache of the other orientation
    const int64_t* map;     // own position -> other position
    int d, vdim, axis;
    float alpha, reg;
    int* ticket;
    const int32_t* row_list;   // rows this launch works on (light, mid or heavy rows of the orientation)
    int n_list;
};

constexpr int EALS_REG = 4;    // entries per lane kept in registers (rows up to 256 entries)
constexpr int EALS_DB = 16;    // dimensions per block: 16 floats = the 64-byte sector a 4-byte gather of Y[key][d] pulls anyway
constexpr int EALS_LIGHT = 64 * EALS_REG;
constexpr int EALS_HEAVY = 4096;   // above: one 1024-thread block per row; (EALS_LIGHT, EALS_HEAVY]: one wave per row, both over HBM scratch

// Round 3: the coordinate of dimension d needs Y[key][d] of EVERY entry of the row -- a 4-byte gather that costs a 64-byte sector, 128
// times per entry at d = 128: the epoch was bound by 16x its useful traffic (131 ms on the ML-20M shape).  Both kernels now walk the
// dimensions in blocks of 16: the 64-byte segment Y[key][16 b .. 16 b + 15] of every entry is fetched ONCE per block (registers for
// rows up to 256 entries; otherwise transposed into a per-row scratch [16][n] that the 16 steps then read coalesced), and the entry
// constants w - c_i (a second sector gather per step on the user side) once per row.

// ---- the steps both update kernels share ----

// this thread's part of x . S[:, d] (S symmetric): elements first, first + stride, ...
__device__ __forceinline__ float eals_dot_S(const float* xs, const float* S, int d, int vdim, int D, int first, int stride) {
    float dot = 0.f;
    for (int e = first; e < D; e += stride) dot += xs[e] * S[static_cast<size_t>(d) * vdim + e];
    return dot;
}

// The new coordinate from the row's reduced sums: num / den over the entries, dot = x . S[:, d], sdd = S[d][d], xd the old coordinate.
// num and den are closed in place: taken by value, the light kernel's 16 unrolled steps compile to another branch layout (3,199
// instructions and 183 registers instead of 3,135 and 181; profiles/eals_refactor.txt section 2).
__device__ __forceinline__ float eals_new_coordinate(float& num, float& den, float dot, float xd, float sdd, float cx, int axis, float reg) {
    if (axis == 0) {   // eals.cc:214-215
        num += -dot + xd * sdd;
        den += sdd + reg;
    } else {           // eals.cc:261-262
        num += -cx * (dot - xd * sdd);
        den += cx * sdd + reg;
    }
    return num / den;
}

// the next item of the launch's row list: one fetch per wave, or one per block broadcast through `slot` (LDS)
__device__ __forceinline__ int eals_ticket_wave(int* ticket, int lane) {
    int item = 0;
    if (lane == 0) item = atomicAdd(ticket, 1);
    return __builtin_amdgcn_readfirstlane(item);
}
__device__ __forceinline__ int eals_ticket_block(int* ticket, int* slot, int tid) {
    __syncthreads();
    if (tid == 0) *slot = atomicAdd(ticket, 1);
    __syncthreads();
    return *slot;
}

// barrier of the thread group that works on one row: a wave (BS = 64) or a block
template <int BS>
__device__ __forceinline__ void eals_group_sync() {
    if constexpr (BS == 64) wave_lds_sync();
    else __syncthreads();
}

// rows up to EALS_LIGHT entries: one wave per row, everything in registers
__global__ __launch_bounds__(256) void eals_update_kernel(EalsParams p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float* xs = lds + wv * p.vdim;
    const int D = p.d, vdim = p.vdim;
    while (true) {
        const int item = eals_ticket_wave(p.ticket, lane);
        if (item >= p.n_list) break;
        const int x = p.row_list[item];
        const int64_t beg = row_begin(p.indptr, x), end = p.indptr[x];
        float* xrow = p.X + static_cast<size_t>(x) * vdim;
        wave_lds_sync();
        for (int e = lane; e < vdim; e += 64) xs[e] = xrow[e];
        wave_lds_sync();
        const float cx = p.axis == 1 ? p.Cw[x] : 0.f;
        int rk[EALS_REG];
        float rv[EALS_REG], rh[EALS_REG], rw[EALS_REG], rm[EALS_REG];   // value, vhat, w = 1 + alpha v, w - c
        bool ok[EALS_REG];
#pragma unroll
        for (int s = 0; s < EALS_REG; ++s) {
            const int64_t ind = beg + s * 64 + lane;
            ok[s] = ind < end;
            rk[s] = ok[s] ? p.keys[ind] : 0;
            rv[s] = ok[s] ? p.vals[ind] : 0.f;
            rh[s] = ok[s] ? p.own[ind] : 0.f;
            rw[s] = 1.f + p.alpha * rv[s];
            rm[s] = rw[s] - (p.axis == 0 ? (ok[s] ? p.Cw[rk[s]] : 0.f) : cx);
        }
        for (int db = 0; db < D; db += EALS_DB) {
            float yb[EALS_REG][EALS_DB];
#pragma unroll
            for (int s = 0; s < EALS_REG; ++s) {
                const float4* src = reinterpret_cast<const float4*>(p.Y + static_cast<size_t>(rk[s]) * vdim + db);
#pragma unroll
                for (int q4 = 0; q4 < EALS_DB / 4; ++q4) {
                    const float4 v = ok[s] ? src[q4] : make_float4(0.f, 0.f, 0.f, 0.f);
                    yb[s][4 * q4] = v.x; yb[s][4 * q4 + 1] = v.y; yb[s][4 * q4 + 2] = v.z; yb[s][4 * q4 + 3] = v.w;
                }
            }
#pragma unroll
            for (int dd = 0; dd < EALS_DB; ++dd) {
                const int d = db + dd;
                if (d < D) {
                    const float xd = xs[d];
                    float num = 0.f, den = 0.f;
#pragma unroll
                    for (int s = 0; s < EALS_REG; ++s) {
                        const float yd = yb[s][dd];
                        const float pq = xd * yd;
                        const float vf = rh[s] - pq;
                        if (ok[s]) {
                            num += (rw[s] * rv[s] - rm[s] * vf) * yd;
                            den += rm[s] * yd * yd;
                        }
                        rh[s] = vf;
                    }
                    float dot = eals_dot_S(xs, p.S, d, vdim, D, lane, 64);
                    num = wave_sum(num);
                    den = wave_sum(den);
                    dot = wave_sum(dot);
                    const float xn = eals_new_coordinate(num, den, dot, xd, p.S[static_cast<size_t>(d) * vdim + d], cx, p.axis, p.reg);
                    wave_lds_sync();
                    if (lane == 0) xs[d] = xn;
                    wave_lds_sync();
#pragma unroll
                    for (int s = 0; s < EALS_REG; ++s) rh[s] += xn * yb[s][dd];
                }
            }
        }
        for (int e = lane; e < D; e += 64) xrow[e] = xs[e];
#pragma unroll
        for (int s = 0; s < EALS_REG; ++s) {
            const int64_t ind = beg + s * 64 + lane;
            if (ind < end) {
                p.own[ind] = rh[s];
                p.other[p.map[ind]] = rh[s];
            }
        }
    }
}

// Rows above EALS_LIGHT entries.  BS = 64: one wave per row (ticketed, longest first); BS = 1024: one block per row, the per-dimension
// sums combined through LDS -- three barriers per dimension instead of a 131 K-entry row crawling through one wave.
// `scratch`: per thread group (1 + EALS_DB) * cap floats: w - c of every entry | Y[key][16 b + dd] as [dd][entry].
// vhat lives in HBM (coalesced); a step's closing update vhat += x_new * y is folded into the NEXT step's pass (the same two
// roundings in the same order), so every dimension costs one pass over the row: 24 bytes per entry instead of 220.
// `row_off` (BS = 1024): the scratch of list item k starts at (1 + EALS_DB) * row_off[k] floats and is as long as the row (rounded up
// to 64 entries) -- a slot of the longest row's size per block would cost gigabytes for the few 10^5-entry rows of a real catalogue.
template <int BS>
__global__ __launch_bounds__(BS) void eals_update_long_kernel(EalsParams p, float* __restrict__ scratch, int64_t cap, const int64_t* __restrict__ row_off) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* xs = lds;                 // [vdim]
    float* red = lds + p.vdim;       // [3][16]  (BS = 1024)
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int D = p.d, vdim = p.vdim;
    float* wmc = scratch + static_cast<size_t>(blockIdx.x) * (1 + EALS_DB) * cap;
    while (true) {
        int item;
        if constexpr (BS == 64) item = eals_ticket_wave(p.ticket, lane);
        else item = eals_ticket_block(p.ticket, reinterpret_cast<int*>(red), tid);
        if (item >= p.n_list) break;
        const int x = p.row_list[item];
        const int64_t beg = row_begin(p.indptr, x), end = p.indptr[x];
        const int64_t n = end - beg;
        if (row_off) {   // this row's own slot
            cap = ((n + 63) / 64) * 64;
            wmc = scratch + static_cast<size_t>(row_off[item]) * (1 + EALS_DB);
        }
        float* const yb_ = wmc + cap;
        float* xrow = p.X + static_cast<size_t>(x) * vdim;
        eals_group_sync<BS>();
        for (int e = tid; e < vdim; e += BS) xs[e] = xrow[e];
        const float cx = p.axis == 1 ? p.Cw[x] : 0.f;
        for (int64_t i = tid; i < n; i += BS) {
            const float w = 1.f + p.alpha * p.vals[beg + i];
            wmc[i] = w - (p.axis == 0 ? p.Cw[p.keys[beg + i]] : cx);
        }
        eals_group_sync<BS>();
        for (int db = 0; db < D; db += EALS_DB) {
            for (int64_t i = tid; i < n; i += BS) {   // the block's 64-byte segment of every entry, transposed into [dd][entry]
                const float4* src = reinterpret_cast<const float4*>(p.Y + static_cast<size_t>(p.keys[beg + i]) * vdim + db);
#pragma unroll
                for (int q4 = 0; q4 < EALS_DB / 4; ++q4) {
                    const float4 v = src[q4];
                    yb_[(4 * q4 + 0) * cap + i] = v.x; yb_[(4 * q4 + 1) * cap + i] = v.y;
                    yb_[(4 * q4 + 2) * cap + i] = v.z; yb_[(4 * q4 + 3) * cap + i] = v.w;
                }
            }
            float pend = 0.f;   // x_new of the previous step of this block, still to be folded into vhat
            const int nd = D - db < EALS_DB ? D - db : EALS_DB;
            for (int dd = 0; dd < nd; ++dd) {
                const int d = db + dd;
                const float xd = xs[d];
                float num = 0.f, den = 0.f;
                const float* yd_ = yb_ + static_cast<size_t>(dd) * cap;
                const float* yp_ = yb_ + static_cast<size_t>(dd > 0 ? dd - 1 : 0) * cap;
                for (int64_t i = tid; i < n; i += BS) {
                    const float yd = yd_[i];
                    float vh = p.own[beg + i];
                    if (dd > 0) vh += pend * yp_[i];
                    const float pq = xd * yd;
                    const float vf = vh - pq;
                    const float v = p.vals[beg + i];
                    const float w = 1.f + p.alpha * v;
                    const float wm = wmc[i];
                    num += (w * v - wm * vf) * yd;
                    den += wm * yd * yd;
                    p.own[beg + i] = vf;
                }
                float dot = eals_dot_S(xs, p.S, d, vdim, D, tid, BS);
                num = wave_sum(num);
                den = wave_sum(den);
                dot = wave_sum(dot);
                if constexpr (BS != 64) {
                    if (lane == 0) { red[wv] = num; red[16 + wv] = den; red[32 + wv] = dot; }
                    __syncthreads();
                    num = den = dot = 0.f;
#pragma unroll
                    for (int w2 = 0; w2 < BS / 64; ++w2) { num += red[w2]; den += red[16 + w2]; dot += red[32 + w2]; }
                }
                const float xn = eals_new_coordinate(num, den, dot, xd, p.S[static_cast<size_t>(d) * vdim + d], cx, p.axis, p.reg);
                eals_group_sync<BS>();
                if (tid == 0) xs[d] = xn;
                eals_group_sync<BS>();
                pend = xn;
            }
            const float* yl_ = yb_ + static_cast<size_t>(nd - 1) * cap;   // close the block: the last step's update of vhat
            for (int64_t i = tid; i < n; i += BS) p.own[beg + i] += pend * yl_[i];
            eals_group_sync<BS>();
        }
        for (int e = tid; e < D; e += BS) xrow[e] = xs[e];
        for (int64_t i = tid; i < n; i += BS) p.other[p.map[beg + i]] = p.own[beg + i];
    }
}

// entry `ind` of a compressed side -> sort key (other id << 32 | own id); the payload is the entry's position
__global__ __launch_bounds__(256) void eals_coord_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ keys, int rows, int64_t nnz,
                                                         uint64_t* __restrict__ key_out, int64_t* __restrict__ pos_out) {
    const int64_t ind = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (ind >= nnz) return;
    const uint64_t x = static_cast<uint64_t>(lower_bound_dev<int64_t>(indptr, rows, ind + 1));   // first row whose END offset is > ind
    key_out[ind] = (static_cast<uint64_t>(static_cast<uint32_t>(keys[ind])) << 32) | x;
    pos_out[ind] = ind;
}
__global__ __launch_bounds__(256) void eals_rank_kernel(const int64_t* __restrict__ sorted_pos, int64_t nnz, int64_t* __restrict__ map) {
    const int64_t r = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (r < nnz) map[sorted_pos[r]] = r;
}

// vhat[ind] = X[row(ind)] . Y[key(ind)]   (eals.cc:72-78); one wave per row
__global__ __launch_bounds__(256) void eals_cache_kernel(const float* __restrict__ X, const float* __restrict__ Y, int vdim, int rows,
                                                         const int64_t* __restrict__ indptr, const int32_t* __restrict__ keys, float* __restrict__ vhat) {
    const int lane = threadIdx.x & 63;
    const int x = static_cast<int>((static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6);
    if (x >= rows) return;
    const int64_t beg = row_begin(indptr, x), end = indptr[x];
    const float* xr = X + static_cast<size_t>(x) * vdim;
    for (int64_t ind = beg; ind < end; ++ind) {
        const float part = wave_dot(xr, Y + static_cast<size_t>(keys[ind]) * vdim, vdim, lane);
        if (lane == 0) vhat[ind] = part;
    }
}

// out[r][e] = sqrt(w[r]) * F[r][e]
__global__ __launch_bounds__(256) void eals_scale_rows_kernel(const float* __restrict__ F, const float* __restrict__ w, int rows, int vdim, float* __restrict__ out) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i < static_cast<int64_t>(rows) * vdim) out[i] = sqrtf(w[i / vdim]) * F[i];
}

// eals.cc:134-150: per-entry loss terms; out[0] += feedbacks, out[1] += squared error
__global__ __launch_bounds__(256) void eals_loss_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ keys, const float* __restrict__ vals,
                                                        const float* __restrict__ vhat, const float* __restrict__ Cw, int rows, int axis, float alpha,
                                                        double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int x = static_cast<int>((static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6);
    if (x >= rows) return;
    const int64_t beg = row_begin(indptr, x), end = indptr[x];
    double fb = 0.0, se = 0.0;
    for (int64_t ind = beg + lane; ind < end; ind += 64) {
        const float v = vals[ind], vh = vhat[ind], err = v - vh;
        fb += static_cast<double>((1.f + alpha * v) * err * err) - static_cast<double>(Cw[axis == 0 ? keys[ind] : x] * vh * vh);
        se += static_cast<double>(err * err);
    }
    fb = wave_sum_f64(fb);
    se = wave_sum_f64(se);
    if (lane == 0 && end > beg) {
        atomicAdd(out, fb);
        atomicAdd(out + 1, se);
    }
}

// out += sum F^2 over [rows, vdim] (pad columns are zero)
__global__ __launch_bounds__(256) void eals_sqsum_kernel(const float* __restrict__ F, int64_t n, double* __restrict__ out) {
    double part = 0.0;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * 256)
        part += static_cast<double>(F[i]) * static_cast<double>(F[i]);
    part = wave_sum_f64(part);
    if ((threadIdx.x & 63) == 0) atomicAdd(out, part);
}

}  // namespace bfh
