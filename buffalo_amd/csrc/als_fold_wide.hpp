// als_fold_wide_kernel (gfx950) -- fold-in's fused row kernel for every vdim <= 256: Gramian, Cholesky and both triangular solves of ONE
// history in ONE 256-thread block, nothing of the system ever in HBM.  Reached through bfh_als_set_mode(h, "als_fold_solve", 2); the host
// side is AlsHandle::fold_in (als_handle.hpp).
//
//     out[b] = (FF + alpha sum v q q^T + reg ada I)^-1 sum (1 + alpha v) q          (tests/fold_in_cases.py states the rule)
//
// Why a kernel of its own: als_gram_kernel holds the whole triangle of tiles in ONE wave (576 accumulator registers at T = 8) and
// als_fold_solve_kernel keeps M as [vdim][vdim + 1] in LDS (263 KB at 256).  Here the T (T + 1) / 2 lower-triangle 32 x 32 tiles are dealt
// round-robin to the block's four waves (9 tiles = 144 accumulator registers at T = 8) and M lives in LDS as a lower triangle of tile rows.
//
// Phase A, the row Gramian on v_mfma_f32_32x32x2_f32.  The history is walked by its one block in CSR order, in groups of G = 16 entries (the
//   same G at every vdim).  A group's q rows are gathered ONCE per block: every thread issues its T 8-byte loads of group g + 1 (and the key
//   loads of group g + 2) before the block feeds group g to the matrix pipe, and parks them in the other half of a two-slot LDS ring after it;
//   one barrier per group.  Every wave reads the column blocks its tiles need from the ring: A = alpha v q[32 i + col], B = q[32 j + col],
//   one instruction per two entries (lane half = entry parity).  Thread c < vdim accumulates y[c] beside the tiles with one fused
//   multiply-add per entry, in entry order.  A short last group is filled with zero rows of weight zero.  No chunks, no heavy slots, no
//   atomics: a history of ANY length is one sequence of instructions fixed by (d, vdim) and its own entries -- its bits do not depend on the
//   batch, the position in it, the row order, the cuts or the run.
// Phase B, M in LDS and a right-looking blocked Cholesky, panels of 32.
//   layout  tile row i (matrix rows 32 i .. 32 i + 31) stores columns [0, 32 i + 32) with leading dimension 32 i + 33: the lower triangle of
//           tiles, the diagonal tiles whole (their upper halves are never read for a result).  512 T^2 + 544 T floats: 145 KB at T = 8 against
//           263 KB for the square.  The leading dimensions are odd, so the three access shapes that matter are spread over the banks: a
//           thread per row (triangular solve), a lane per row (operands of the trailing update) and a lane per column (accumulator tiles, back
//           substitution).  The ring of phase A aliases this region (dead by then, a barrier between); its entry stride is vdim (+ 32 at even
//           T, so that the two entries of an instruction do not start on the same bank).
//   build   accumulators + the matching FF tiles (L2-resident) + reg ada on the diagonal; rows [d, vdim) become identity rows with y = 0
//           (panels of 32: the padded system is exactly vdim wide).
//   panel   every wave factors the 32 x 32 diagonal block redundantly in registers (lane = row, columns unrolled, the pivot row's entries
//           passed around with v_readlane -- no LDS traffic, no hand-off between waves), and in the same sweep each thread solves the row
//           it owns below the block against it: the row's 32 panel entries sit in registers, the block's entries arrive as the very scalars
//           the factorisation reads.  Thread 255 owns y as one more row: that is the forward solve.  Three barriers per panel.
//   update  A22 -= L21 L21^T on the fp32 matrix instruction: 16 instructions per lower-triangle tile, tiles dealt round-robin to the four
//           waves (84 tile updates at T = 8: the d^3 of the method); y's trailing entries by the thread that owns the row.
//   back    L^T x = z backwards by the same panels, one barrier each: every wave solves the panel's 32 unknowns with a lane per unknown
//           (32 dependent steps, the block's columns preloaded), every thread left of the panel takes them out of its own z_r (a register).
//   x[0 .. d) goes to out; columns [d, vdim) are never written (the host zeroes out).
// Only plain vector loads and stores; FoldState is all the launch writes.  An exact solve, whatever optimizer the model was trained with.
#pragma once
#include "als_kernels.hpp"

namespace bfh {

constexpr int ALS_FW_G = 16;   // entries per ring group

__host__ __device__ constexpr int als_fw_entry_stride(int vdim) { return vdim + ((vdim / 32) % 2 == 0 ? 32 : 0); }
// floats of the lower triangle of tile rows / of the two-slot ring; the region both live in
__host__ __device__ constexpr int als_fw_tri_floats(int vdim) { return 512 * (vdim / 32) * (vdim / 32) + 544 * (vdim / 32); }
__host__ __device__ constexpr int als_fw_ring_floats(int vdim) { return 2 * ALS_FW_G * als_fw_entry_stride(vdim); }
__host__ __device__ constexpr int als_fw_region_floats(int vdim) {
    return als_fw_tri_floats(vdim) > als_fw_ring_floats(vdim) ? als_fw_tri_floats(vdim) : als_fw_ring_floats(vdim);
}
// dynamic LDS: M (aliased by the ring) | y -> z [vdim] | 1 / l_kk [vdim] | z of the panel being solved [vdim] | alpha v [2][G] | 1 + alpha v [2][G]
__host__ __device__ constexpr size_t als_fold_wide_lds_bytes(int vdim) {
    return (static_cast<size_t>(als_fw_region_floats(vdim)) + 3 * static_cast<size_t>(vdim) + 4 * ALS_FW_G) * sizeof(float);
}
static_assert(als_fold_wide_lds_bytes(256) <= 160 * 1024, "the carve of vdim 256 must fit one CU's LDS");
// two blocks per CU where the carve allows it (T <= 5), one above
__host__ __device__ constexpr int als_fold_wide_blocks_per_cu(int T) { return 2 * als_fold_wide_lds_bytes(32 * T) <= 160 * 1024 ? 2 : 1; }

// element (r, c), c < 32 (r / 32) + 32, of the triangle of tile rows
__device__ __forceinline__ int als_fw_at(int r, int c) {
    const int i = r >> 5;
    return 512 * i * i + 544 * i + (r & 31) * (32 * i + 33) + c;
}
// tile t of a lower triangle numbered row by row: (0,0) (1,0) (1,1) (2,0) ..
__device__ __forceinline__ void als_fw_tile(int t, int& i, int& j) {
    i = 0;
    while (t > i) { t -= i + 1; ++i; }
    j = t;
}
__device__ __forceinline__ float als_fw_readlane(float v, int lane) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

// list[h] = {row, kbeg, kend, -}: a non-empty history and its entries in p.keys / p.vals, longest first; taken by stride
template <int T>
__global__ __launch_bounds__(256, als_fold_wide_blocks_per_cu(T)) void als_fold_wide_kernel(AlsParams p, const AlsWork* __restrict__ list, int n_list) {
    constexpr int VD = 32 * T, G = ALS_FW_G, ES = als_fw_entry_stride(VD), NT = T * (T + 1) / 2, NTW = (NT + 3) / 4;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* M = lds;
    float* ring = lds;
    float* yv = lds + als_fw_region_floats(VD);
    float* dinv = yv + VD;
    float* zb = dinv + VD;
    float* wl = zb + VD;
    float* cl = wl + 2 * G;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, col = lane & 31;
    const int D = p.d;
    // this wave's tiles of the Gramian: wv, wv + 4, ..
    const int ntw = (NT - wv + 3) / 4;
    int ti[NTW], tj[NTW];
#pragma unroll
    for (int u = 0; u < NTW; ++u) {
        ti[u] = 0; tj[u] = 0;
        if (u < ntw) als_fw_tile(wv + 4 * u, ti[u], tj[u]);
    }
    // this thread's share of a group's gather: T pieces of 8 bytes, piece x = k * 256 + tid -> entry x / (16 T), floats 2 (x % (16 T)) ..
    int ent[T], pos[T];
#pragma unroll
    for (int k = 0; k < T; ++k) {
        const int x = k * 256 + tid;
        ent[k] = x / (16 * T);
        pos[k] = 2 * (x % (16 * T));
    }
    for (int h = blockIdx.x; h < n_list; h += gridDim.x) {
        const AlsWork wk = list[h];
        const int n = wk.kend - wk.kbeg;
        const int ng = (n + G - 1) / G;
        __syncthreads();   // the row before is out of LDS
        // ---- phase A ----
        auto keys_of = [&](int g, int (&kk)[T]) {
#pragma unroll
            for (int k = 0; k < T; ++k) {
                const int e = g * G + ent[k];
                kk[k] = e < n ? p.keys[wk.kbeg + e] : -1;   // -1: past the history's end, a zero row
            }
        };
        auto rows_of = [&](const int (&kk)[T], float2 (&q)[T]) {
#pragma unroll
            for (int k = 0; k < T; ++k) {
                q[k] = make_float2(0.f, 0.f);
                if (kk[k] >= 0) q[k] = *reinterpret_cast<const float2*>(p.Q + static_cast<size_t>(kk[k]) * VD + pos[k]);
            }
        };
        auto weight_of = [&](int g) {   // thread e < G: alpha v of entry e of the group (0 past the end)
            const int e = g * G + tid;
            return (tid < G && e < n) ? p.alpha * p.vals[wk.kbeg + e] : 0.f;
        };
        auto park = [&](int buf, int g, const float2 (&q)[T], float w) {
#pragma unroll
            for (int k = 0; k < T; ++k) *reinterpret_cast<float2*>(ring + (buf * G + ent[k]) * ES + pos[k]) = q[k];
            if (tid < G) {
                wl[buf * G + tid] = w;
                cl[buf * G + tid] = g * G + tid < n ? 1.0f + w : 0.f;
            }
        };
        f32x16 acc[NTW];
#pragma unroll
        for (int u = 0; u < NTW; ++u)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[u][e] = 0.f;
        float yacc = 0.f;
        int kc[T], kn[T];
        float2 qr[T];
        keys_of(0, kc);
        keys_of(1, kn);
        rows_of(kc, qr);
        float wr = weight_of(0);
        park(0, 0, qr, wr);
        __syncthreads();
        for (int g = 0; g < ng; ++g) {
            const int buf = g & 1;
            const bool more = g + 1 < ng;
            if (more) {   // in flight while this group feeds the matrix pipe
                rows_of(kn, qr);
                wr = weight_of(g + 1);
                keys_of(g + 2, kn);
            }
            const float* rb = ring + buf * G * ES;
            float wreg[G / 2];
#pragma unroll
            for (int s = 0; s < G / 2; ++s) wreg[s] = wl[buf * G + 2 * s + half];
#pragma unroll
            for (int u = 0; u < NTW; ++u) {
                if (u < ntw) {
                    const float* qa = rb + half * ES + 32 * ti[u] + col;
                    const float* qb = rb + half * ES + 32 * tj[u] + col;
#pragma unroll
                    for (int s = 0; s < G / 2; ++s) acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(wreg[s] * qa[2 * s * ES], qb[2 * s * ES], acc[u], 0, 0, 0);
                }
            }
            if (tid < VD) {
#pragma unroll
                for (int e = 0; e < G; ++e) yacc = __builtin_fmaf(cl[buf * G + e], rb[e * ES + tid], yacc);
            }
            if (more) park(buf ^ 1, g + 1, qr, wr);
            __syncthreads();
        }
        // ---- phase B: M = G + FF + reg ada I over the dead ring (the loop's last barrier lies between) ----
        const float regada = p.reg * (p.adaptive_reg ? static_cast<float>(n) : 1.0f);
#pragma unroll
        for (int u = 0; u < NTW; ++u) {
            if (u < ntw) {
                const int i = ti[u], j = tj[u];
                // the lane's first row and its column, opaque: the addresses and the 2 x 16 masks per tile are formed here, per row, instead of being
                // hoisted out of the persistent loop for all tiles at once and spilled (first compile: 1,246 scalar spills at T = 8)
                int r0 = 32 * i + 4 * half, c = 32 * j + col;
                asm volatile("" : "+v"(r0), "+v"(c));
                const float* Fl = p.FF + static_cast<size_t>(r0) * VD + c;
                float* Ml = M + als_fw_at(r0, c);
                const int ldi = 32 * i + 33;
                float fv[16];
#pragma unroll
                for (int e = 0; e < 16; ++e) fv[e] = Fl[als_acc_row(e) * VD];
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int r = r0 + als_acc_row(e);
                    float m = acc[u][e] + fv[e];
                    if (r == c) m += regada;
                    if (r >= D) m = r == c ? 1.0f : 0.f;   // padding: an identity row
                    Ml[als_acc_row(e) * ldi] = m;
                }
            }
        }
        if (tid < VD) yv[tid] = tid < D ? yacc : 0.f;
        for (int k = 0; k < T; ++k) {
            __syncthreads();   // M as built / the trailing update of the panel before is in LDS
            const int j0 = 32 * k, below = VD - j0 - 32;
            const bool rowt = tid < below, yt = tid == 255;   // below <= 224: thread 255 never owns a matrix row
            const int row = j0 + 32 + tid;
            float dg[32], a[32];
            const float* dsrc = M + als_fw_at(j0 + col, j0);
            const float* asrc = rowt ? M + als_fw_at(row, j0) : yv + j0;   // (threads that own nothing carry y along and store nothing)
#pragma unroll
            for (int m = 0; m < 32; ++m) { dg[m] = dsrc[m]; a[m] = asrc[m]; }
#pragma unroll
            for (int c = 0; c < 32; ++c) {   // lane `col` holds row col of the block; of its columns above the diagonal nothing is ever passed on
                // column c, left-looking: the columns before it out of this column, in column order
#pragma unroll
                for (int m = 0; m < c; ++m) {
                    const float l = als_fw_readlane(dg[m], c);   // L[c][m]
                    dg[c] = __builtin_fmaf(-dg[m], l, dg[c]);
                    a[c] = __builtin_fmaf(-a[m], l, a[c]);
                }
                const float inv = 1.0f / sqrtf(als_fw_readlane(dg[c], c));
                if (tid == 0) dinv[j0 + c] = inv;
                dg[c] *= inv;
                a[c] *= inv;
                // a[c] is finished HERE: left to itself the compiler postpones the row's chain and keeps every scalar of the block alive for it
                // (first compile: 677 scalar spills at T = 1)
                asm volatile("" : "+v"(a[c]));
            }
            __syncthreads();   // every read of the panel comes before any write into it
            if (rowt) {
                float* dst = M + als_fw_at(row, j0);
#pragma unroll
                for (int m = 0; m < 32; ++m) dst[m] = a[m];
            } else if (yt) {
#pragma unroll
                for (int m = 0; m < 32; ++m) yv[j0 + m] = a[m];
            }
            if (tid < 32) {
                float* dst = M + als_fw_at(j0 + tid, j0);
#pragma unroll
                for (int m = 0; m < 32; ++m) dst[m] = dg[m];   // (right of the diagonal: whatever the sweep left there, never read for a result)
            }
            __syncthreads();
            if (rowt) {   // y's trailing entry of this row
                float s = 0.f;
#pragma unroll
                for (int m = 0; m < 32; ++m) s = __builtin_fmaf(a[m], yv[j0 + m], s);
                yv[row] -= s;
            }
            const int rem = T - 1 - k, ntt = rem * (rem + 1) / 2;
            for (int t = wv; t < ntt; t += 4) {
                int i, j;
                als_fw_tile(t, i, j);
                i += k + 1; j += k + 1;
                float* Ct = M + als_fw_at(32 * i + 4 * half, 32 * j + col);
                const int ldi = 32 * i + 33;
                const float* La = M + als_fw_at(32 * i + col, j0 + half);
                const float* Lb = M + als_fw_at(32 * j + col, j0 + half);
                f32x16 c;
                float la[16], lb[16];
#pragma unroll
                for (int e = 0; e < 16; ++e) { c[e] = Ct[als_acc_row(e) * ldi]; la[e] = -La[2 * e]; lb[e] = Lb[2 * e]; }
#pragma unroll
                for (int s = 0; s < 16; ++s) c = __builtin_amdgcn_mfma_f32_32x32x2f32(la[s], lb[s], c, 0, 0, 0);
#pragma unroll
                for (int e = 0; e < 16; ++e) Ct[als_acc_row(e) * ldi] = c[e];
            }
        }
        __syncthreads();
        // ---- L^T x = z ----
        float zr = tid < VD ? yv[tid] : 0.f;
        for (int k = T - 1; k >= 0; --k) {
            const int j0 = 32 * k;
            if (tid >= j0 && tid < j0 + 32) zb[tid] = zr;
            __syncthreads();
            float zc = zb[j0 + col];
            const float di = dinv[j0 + col];
            float lc[32], xs[32];
            const float* Lc = M + als_fw_at(j0, j0) + col;
#pragma unroll
            for (int c = 0; c < 32; ++c) lc[c] = Lc[c * (j0 + 33)];   // L[c][col] (c >= col; the rest is masked below)
#pragma unroll
            for (int c = 31; c >= 0; --c) {
                xs[c] = als_fw_readlane(zc * di, c);
                zc = col < c ? __builtin_fmaf(-lc[c], xs[c], zc) : zc;
            }
            if (tid < j0) {
                const float* Lr = M + als_fw_at(j0, tid);
#pragma unroll
                for (int c = 31; c >= 0; --c) zr = __builtin_fmaf(-Lr[c * (j0 + 33)], xs[c], zr);
            } else if (tid < j0 + 32 && tid < D) {
                p.P[static_cast<size_t>(wk.row) * VD + tid] = zc * di;
            }
        }
    }
}

}  // namespace bfh
