// cfr_fold_kernel (gfx950) -- CoFactor fold-in: the row AND the bias of a user, item or context that is not in the model, every step of
// it in ONE launch, one 256-thread block per row, nothing of a row's system or of its intermediate x / b ever in HBM.  The host side is
// CfrHandle::fold_in (cfr_impl.hpp); the rule is cfr.cc:92-313 applied to a row outside the model (include/buffalo_hip.h states it).
//
// A row has a part a, entries (k_j, v_j), j < n_a, gathering y_j = Y[k_j], and a part c, entries (k_m, v_m), m < n_c, gathering
// g_m = G[k_m] and beta_m = B[k_m] (user: a only; context: c only; item: both).  With the sums over m taken ONCE,
//     A   = l (FF + alpha sum_j v_j y_j y_j^T) + sum_m g_m g_m^T + reg I               (the l (..) term only where there is a part a)
//     y_a = l sum_j (1 + alpha v_j) y_j      t = sum_m (v_m - beta_m) g_m      s = sum_m g_m      c = sum_m (v_m - beta_m)
//     b   = init_bias[row]
//     repeat iters times:   x = A^-1 (y_a + t - b s);   b = (c - x . s) / (n_c + 1e-10)          (b: item / context only)
// which is x = A^-1 (y_a + sum_m (v_m - b - beta_m) g_m), b = sum_m (v_m - x . g_m - beta_m) / (n_c + 1e-10) of the reference.  A does
// not depend on b: it is factored once, L stays in LDS, an iteration is one right-hand side, two triangular solves and one dot product.
//
// Phase A, the Gramian of both parts on v_mfma_f32_32x32x2_f32, fed from a two-slot LDS ring of fixed-size entry groups (G = 16 entries).
//   Part a is walked first, then part c, through the same ring into the same accumulator tiles.  The slot being filled holds the gathered
//   rows and, per entry, two scalars: part a  w = l alpha v (scales the A operand) and 1 + alpha v (for y_a), part c  v - beta (for t and c;
//   the operand is unscaled).  Every thread issues its 8-byte loads of slot s + 1 (and the key loads of slot s + 2) before the block feeds
//   slot s to the matrix pipe, and parks them afterwards; one barrier per slot.  Entries past a part's end are zero rows with zero scalars.
//   T = 3, 4 (6 and 10 lower-triangle tiles): a slot is one group, the tiles are dealt round-robin to the four waves, every wave eats every
//     entry.  Thread c < vdim sums column c of y_a, t and s in entry order.
//   T = 1, 2 (1 and 3 tiles): dealing tiles would idle waves, so a slot is FOUR groups, wave w eats group w of every slot into its own copy of
//     all tiles, and lane c of wave w sums column c over the same entries.  At the end the four copies meet in LDS and are added in wave order
//     ((0 + 1) + 2) + 3, tiles, vectors and c alike.
//   Either way a row is one sequence of instructions fixed by (d, vdim) and its own entries: no atomics, no chunks, no slots in HBM -- its bits
//   do not depend on the batch, the position in it, the order of the rows or the run, at any length.
// Phase B, M in LDS as the lower triangle of tile rows of als_fold_wide.hpp (als_fw_at; odd leading dimensions), built from the tiles + l FF
//   + reg on the diagonal, rows [d, vdim) identity rows.  Right-looking blocked Cholesky by panels of 32 as in als_fold_wide_kernel: every
//   wave factors the diagonal block in registers (lane = row, pivot rows passed by v_readlane), each thread solves the row it owns below
//   the block in the same sweep, the trailing update runs on the matrix instruction.  No right-hand side rides along: it changes per iteration.
// Phase C, per iteration: thread r < vdim forms z_r = y_a + t - b s from the three LDS vectors; forward by panels (the block's 32 unknowns by
//   every wave with a lane per unknown, every thread right of the panel takes them out of its own register), backward the same way from the
//   last panel; x_r ends in thread r.  x . s is a fixed tree (products in LDS, one or two per lane, a butterfly), formed by every wave alike.
// Precision: A, L and the solves are fp32.  The right-hand side is not: b absorbs the mean of v - beta, so t and b s cancel (12-fold in a
//   d = 1 context row of 64 entries, where fp32 sums in any order land 2.6e-6 from float64 in the median, 1.1e-5 at worst), and the error
//   feeds back through b.  So y_a, t, s, c, b, x . s and the subtraction y_a + t - b s are carried in fp64 (LDS vectors included) and z is
//   rounded to fp32 once, after the cancellation; x is fp32, b is rounded when it is stored.
// Only plain vector loads and stores.  The ring does NOT alias M here: the carve of vdim 128 is 66 KB, two blocks per CU.
#pragma once
#include <type_traits>

#include "als_fold_wide.hpp"

namespace bfh {

constexpr int CFR_FOLD_G = 16;   // entries per ring group
__host__ __device__ constexpr int cfr_fold_slot_groups(int T) { return T <= 2 ? 4 : 1; }   // groups per ring slot: one per wave where the waves split the entries
__host__ __device__ constexpr int cfr_fold_slot_entries(int T) { return CFR_FOLD_G * cfr_fold_slot_groups(T); }
// floats of the two-slot ring; at T <= 2 the four waves' tile copies (4 x NT x 1024) are staged in it after the walk
__host__ __device__ constexpr int cfr_fold_ring_floats(int T) {
    const int ring = 2 * cfr_fold_slot_entries(T) * als_fw_entry_stride(32 * T);
    const int stage = T <= 2 ? 4 * (T * (T + 1) / 2) * 1024 : 0;
    return ring > stage ? ring : stage;
}
// dynamic LDS: M | ring | fp64: y_a, t, s, x s [vdim each], the waves' vector copies [4][3][vdim] (T <= 2), c and the waves' copies of it [8] |
//              fp32: 1 / l_kk, z forwards, z backwards [vdim each], w [2][slot], second scalar [2][slot]
__host__ __device__ constexpr size_t cfr_fold_lds_bytes(int T) {
    return (static_cast<size_t>(als_fw_tri_floats(32 * T)) + cfr_fold_ring_floats(T) + (8 + (T <= 2 ? 24 : 0) + 3) * 32 * T + 16 +
            4 * cfr_fold_slot_entries(T)) * sizeof(float);
}
static_assert(2 * cfr_fold_lds_bytes(4) <= 160 * 1024, "two blocks of vdim 128 must fit one CU's LDS");
// blocks of the persistent grid per CU: what the carve (26 KB at T = 1, 41 .. 70 KB above) and the registers (147 at T = 1) let be resident
__host__ __device__ constexpr int cfr_fold_blocks_per_cu(int T) { return T == 1 ? 3 : 2; }
static_assert(cfr_fold_blocks_per_cu(1) * cfr_fold_lds_bytes(1) <= 160 * 1024 && cfr_fold_blocks_per_cu(2) * cfr_fold_lds_bytes(2) <= 160 * 1024 &&
              cfr_fold_blocks_per_cu(3) * cfr_fold_lds_bytes(3) <= 160 * 1024, "the persistent grid must be resident");

struct CfrFoldParams {
    const float* Ya;        // part a: the factor gathered [rows, vdim] and its Gramian [vdim, vdim]; both NULL where the kind has no part a
    const float* FF;
    const float* Gc;        // part c: the factor gathered and the bias beside it; both NULL where the kind has no part c
    const float* Bc;
    const int32_t* keys_a;
    const float* vals_a;
    const int32_t* keys_c;
    const float* vals_c;
    float* out;             // [n_rows, vdim], zeroed by the host: columns [d, vdim) and the empty rows are never written
    float* bias;            // [n_rows]: holds init_bias on entry, b on exit; NULL: the kind has no bias ("user")
    int d, iters;
    float alpha, l, reg;
};
// a non-empty row and its entries in the two parts; the list is sorted longest first and taken by stride
struct CfrFoldItem {
    int row, abeg, aend, cbeg, cend;
};

template <int T>
__global__ __launch_bounds__(256, 2) void cfr_fold_kernel(CfrFoldParams p, const CfrFoldItem* __restrict__ list, int n_list) {
    constexpr int VD = 32 * T, G = CFR_FOLD_G, EPS = cfr_fold_slot_entries(T), ES = als_fw_entry_stride(VD), NT = T * (T + 1) / 2;
    constexpr bool SPLIT = T <= 2;                  // the waves split the entries and every wave holds every tile
    constexpr int TPW = SPLIT ? NT : (NT + 3) / 4;  // tiles per wave, at most
    constexpr int NP = EPS * T / 16;                // 8-byte pieces of a slot's gather per thread
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* M = lds;
    float* ring = M + als_fw_tri_floats(VD);
    double* yav = reinterpret_cast<double*>(ring + cfr_fold_ring_floats(T));   // (every region before it is an even number of floats)
    double* tvv = yav + VD;
    double* svv = tvv + VD;
    double* prod = svv + VD;
    double* vpart = prod + VD;                  // [4][3][VD], T <= 2 only
    double* sc = vpart + (SPLIT ? 12 * VD : 0); // [0] c, [4 .. 8) the waves' copies
    float* dinv = reinterpret_cast<float*>(sc + 8);
    float* zf = dinv + VD;
    float* zb = zf + VD;
    float* wl = zb + VD;             // [2][EPS]
    float* cl = wl + 2 * EPS;        // [2][EPS]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, col = lane & 31;
    const int D = p.d;
    const int ntw = SPLIT ? NT : (NT - wv + 3) / 4;
    int ti[TPW], tj[TPW];
#pragma unroll
    for (int u = 0; u < TPW; ++u) {
        ti[u] = 0; tj[u] = 0;
        if (u < ntw) als_fw_tile(SPLIT ? u : wv + 4 * u, ti[u], tj[u]);
    }
    const int eb = SPLIT ? wv * G : 0;     // this wave's entries of a slot: [eb, eb + G)
    const int vc = SPLIT ? lane : tid;     // the column whose vector sums this thread carries (over this wave's entries)
    const bool vt = vc < VD;
    // this thread's share of a slot's gather: piece x = k * 256 + tid -> entry x / (16 T), floats 2 (x % (16 T)) ..
    int ent[NP], pos[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int x = k * 256 + tid;
        ent[k] = x / (16 * T);
        pos[k] = 2 * (x % (16 * T));
    }
    for (int h = blockIdx.x; h < n_list; h += gridDim.x) {
        const CfrFoldItem wk = list[h];
        const int n_c = wk.cend - wk.cbeg;
        __syncthreads();   // the row before is out of LDS
        f32x16 acc[TPW];
#pragma unroll
        for (int u = 0; u < TPW; ++u)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[u][e] = 0.f;
        double ya = 0.0, tv = 0.0, sv = 0.0, cs = 0.0;   // fp64: see "Precision" at the head
        // ---- phase A: one part through the ring (part: std::false_type = a, std::true_type = c) ----
        auto walk = [&](auto part, const float* __restrict__ F, const int32_t* __restrict__ keys, const float* __restrict__ vals, int beg, int n) {
            constexpr bool C = decltype(part)::value;
            if (n == 0) return;
            const int ns = (n + EPS - 1) / EPS;
            auto keys_of = [&](int s, int (&kk)[NP]) {
#pragma unroll
                for (int k = 0; k < NP; ++k) {
                    const int e = s * EPS + ent[k];
                    kk[k] = e < n ? keys[beg + e] : -1;   // -1: past the part's end, a zero row
                }
            };
            auto rows_of = [&](const int (&kk)[NP], float2 (&q)[NP]) {
#pragma unroll
                for (int k = 0; k < NP; ++k) {
                    q[k] = make_float2(0.f, 0.f);
                    if (kk[k] >= 0) q[k] = *reinterpret_cast<const float2*>(F + static_cast<size_t>(kk[k]) * VD + pos[k]);
                }
            };
            auto scalars_of = [&](int s, float& w, float& c) {   // thread e < EPS: the two scalars of entry e of the slot (0 past the end)
                const int e = s * EPS + tid;
                w = 0.f; c = 0.f;
                if (tid < EPS && e < n) {
                    const float v = vals[beg + e];
                    if constexpr (C) {
                        c = v - p.Bc[keys[beg + e]];
                    } else {
                        const float av = p.alpha * v;
                        w = p.l * av;
                        c = 1.0f + av;
                    }
                }
            };
            auto park = [&](int buf, const float2 (&q)[NP], float w, float c) {
#pragma unroll
                for (int k = 0; k < NP; ++k) *reinterpret_cast<float2*>(ring + (buf * EPS + ent[k]) * ES + pos[k]) = q[k];
                if (tid < EPS) {
                    wl[buf * EPS + tid] = w;
                    cl[buf * EPS + tid] = c;
                }
            };
            int kc[NP], kn[NP];
            float2 qr[NP];
            float wr, cr;
            keys_of(0, kc);
            keys_of(1, kn);
            rows_of(kc, qr);
            scalars_of(0, wr, cr);
            park(0, qr, wr, cr);
            __syncthreads();
            for (int s = 0; s < ns; ++s) {
                const int buf = s & 1;
                const bool more = s + 1 < ns;
                if (more) {   // in flight while this slot feeds the matrix pipe
                    rows_of(kn, qr);
                    scalars_of(s + 1, wr, cr);
                    keys_of(s + 2, kn);
                }
                if (s * EPS + eb < n) {   // (wave-uniform: a group past the end is zero rows, skipping it leaves every bit as it is)
                    const float* rb = ring + (buf * EPS + eb) * ES;
                    float wreg[G / 2];
                    if constexpr (!C) {
#pragma unroll
                        for (int m = 0; m < G / 2; ++m) wreg[m] = wl[buf * EPS + eb + 2 * m + half];
                    }
#pragma unroll
                    for (int u = 0; u < TPW; ++u) {
                        if (u < ntw) {
                            const float* qa = rb + half * ES + 32 * ti[u] + col;
                            const float* qb = rb + half * ES + 32 * tj[u] + col;
#pragma unroll
                            for (int m = 0; m < G / 2; ++m) {
                                float a = qa[2 * m * ES];
                                if constexpr (!C) a *= wreg[m];
                                acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, qb[2 * m * ES], acc[u], 0, 0, 0);
                            }
                        }
                    }
                    if (vt) {
#pragma unroll
                        for (int e = 0; e < G; ++e) {
                            const double r = rb[e * ES + vc], c = cl[buf * EPS + eb + e];
                            if constexpr (C) {
                                tv = __builtin_fma(c, r, tv);
                                sv += r;
                                cs += c;
                            } else {
                                ya = __builtin_fma(c, r, ya);
                            }
                        }
                    }
                }
                if (more) park(buf ^ 1, qr, wr, cr);
                __syncthreads();
            }
        };
        if (p.Ya) walk(std::false_type{}, p.Ya, p.keys_a, p.vals_a, wk.abeg, wk.aend - wk.abeg);
        if (p.Gc) walk(std::true_type{}, p.Gc, p.keys_c, p.vals_c, wk.cbeg, n_c);
        // ---- phase B: M = tiles + l FF + reg I ----
        auto build = [&](int i, int j, const f32x16& a) {
            // the lane's first row and its column, opaque: the addresses and masks of a tile are formed here, per tile, instead of being hoisted out
            // of the persistent loop for all tiles at once (als_fold_wide.hpp)
            int r0 = 32 * i + 4 * half, c = 32 * j + col;
            asm volatile("" : "+v"(r0), "+v"(c));
            float* Ml = M + als_fw_at(r0, c);
            const int ldi = 32 * i + 33;
            float fv[16];
#pragma unroll
            for (int e = 0; e < 16; ++e) fv[e] = 0.f;
            if (p.FF) {
                const float* Fl = p.FF + static_cast<size_t>(r0) * VD + c;
#pragma unroll
                for (int e = 0; e < 16; ++e) fv[e] = Fl[als_acc_row(e) * VD];
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int r = r0 + als_acc_row(e);
                float m = __builtin_fmaf(p.l, fv[e], a[e]);
                if (r == c) m += p.reg;
                if (r >= D) m = r == c ? 1.0f : 0.f;   // padding: an identity row
                Ml[als_acc_row(e) * ldi] = m;
            }
        };
        if constexpr (SPLIT) {
            // the four waves' copies meet in LDS (the ring is dead: the walk's last barrier lies between) and are added in wave order
#pragma unroll
            for (int u = 0; u < NT; ++u)
#pragma unroll
                for (int e = 0; e < 16; ++e) ring[((wv * NT + u) * 16 + e) * 64 + lane] = acc[u][e];
            if (vt) {
                vpart[(wv * 3 + 0) * VD + vc] = ya;
                vpart[(wv * 3 + 1) * VD + vc] = tv;
                vpart[(wv * 3 + 2) * VD + vc] = sv;
            }
            if (lane == 0) sc[4 + wv] = cs;
            __syncthreads();
            if (wv < NT) {   // tile wv by wave wv
                f32x16 a;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const float* q = ring + (wv * 16 + e) * 64 + lane;
                    a[e] = ((q[0] + q[NT * 1024]) + q[2 * NT * 1024]) + q[3 * NT * 1024];
                }
                int i, j;
                als_fw_tile(wv, i, j);
                build(i, j, a);
            }
            if (tid < VD) {
                ya = ((vpart[tid] + vpart[3 * VD + tid]) + vpart[6 * VD + tid]) + vpart[9 * VD + tid];
                tv = ((vpart[VD + tid] + vpart[4 * VD + tid]) + vpart[7 * VD + tid]) + vpart[10 * VD + tid];
                sv = ((vpart[2 * VD + tid] + vpart[5 * VD + tid]) + vpart[8 * VD + tid]) + vpart[11 * VD + tid];
            }
            cs = ((sc[4] + sc[5]) + sc[6]) + sc[7];
        } else {
#pragma unroll
            for (int u = 0; u < TPW; ++u)
                if (u < ntw) build(ti[u], tj[u], acc[u]);
        }
        if (tid < VD) {
            const bool in = tid < D;
            yav[tid] = in ? static_cast<double>(p.l) * ya : 0.0;
            tvv[tid] = in ? tv : 0.0;
            svv[tid] = in ? sv : 0.0;
        }
        if (tid == 0) sc[0] = cs;
        for (int k = 0; k < T; ++k) {
            __syncthreads();   // M and the vectors as built / the trailing update of the panel before is in LDS
            const int j0 = 32 * k, below = VD - j0 - 32;
            const bool rowt = tid < below;
            const int row = j0 + 32 + tid;
            float dg[32], a[32];
            const float* dsrc = M + als_fw_at(j0 + col, j0);
            const float* asrc = rowt ? M + als_fw_at(row, j0) : dsrc;   // (threads that own no row carry the block's own row along and store nothing)
#pragma unroll
            for (int m = 0; m < 32; ++m) { dg[m] = dsrc[m]; a[m] = asrc[m]; }
#pragma unroll
            for (int c = 0; c < 32; ++c) {   // lane `col` holds row col of the block; of its columns above the diagonal nothing is ever passed on
#pragma unroll
                for (int m = 0; m < c; ++m) {
                    const float lcm = als_fw_readlane(dg[m], c);   // L[c][m]
                    dg[c] = __builtin_fmaf(-dg[m], lcm, dg[c]);
                    a[c] = __builtin_fmaf(-a[m], lcm, a[c]);
                }
                const float inv = 1.0f / sqrtf(als_fw_readlane(dg[c], c));
                if (tid == 0) dinv[j0 + c] = inv;
                dg[c] *= inv;
                a[c] *= inv;
                asm volatile("" : "+v"(a[c]));   // finished here: the row's chain is not postponed with every scalar of the block alive for it (als_fold_wide.hpp)
            }
            __syncthreads();   // every read of the panel comes before any write into it
            if (rowt) {
                float* dst = M + als_fw_at(row, j0);
#pragma unroll
                for (int m = 0; m < 32; ++m) dst[m] = a[m];
            }
            if (tid < 32) {
                float* dst = M + als_fw_at(j0 + tid, j0);
#pragma unroll
                for (int m = 0; m < 32; ++m) dst[m] = dg[m];   // (right of the diagonal: whatever the sweep left there, never read for a result)
            }
            __syncthreads();
            const int rem = T - 1 - k, ntt = rem * (rem + 1) / 2;
            for (int t = wv; t < ntt; t += 4) {   // A22 -= L21 L21^T
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
                for (int m = 0; m < 16; ++m) c = __builtin_amdgcn_mfma_f32_32x32x2f32(la[m], lb[m], c, 0, 0, 0);
#pragma unroll
                for (int e = 0; e < 16; ++e) Ct[als_acc_row(e) * ldi] = c[e];
            }
        }
        __syncthreads();
        // ---- phase C: the iterations on L ----
        const double csum = sc[0];
        const double nc = static_cast<double>(n_c) + 1e-10;
        double b = p.bias ? static_cast<double>(p.bias[wk.row]) : 0.0;
        float zr = 0.f;
        for (int it = 0; it < p.iters; ++it) {
            zr = tid < VD ? static_cast<float>(__builtin_fma(-b, svv[tid], yav[tid] + tvv[tid])) : 0.f;
            for (int k = 0; k < T; ++k) {   // L z = r
                const int j0 = 32 * k;
                if (tid >= j0 && tid < j0 + 32) zf[tid] = zr;
                __syncthreads();
                float zc = zf[j0 + col];
                const float di = dinv[j0 + col];
                float lr[32], xs[32];
                const float* Lr = M + als_fw_at(j0 + col, j0);
#pragma unroll
                for (int c = 0; c < 32; ++c) lr[c] = Lr[c];   // L[col][c] (c <= col; the rest is masked below)
#pragma unroll
                for (int c = 0; c < 32; ++c) {
                    xs[c] = als_fw_readlane(zc * di, c);
                    zc = col > c ? __builtin_fmaf(-lr[c], xs[c], zc) : zc;
                }
                if (tid >= j0 + 32 && tid < VD) {
                    const float* Lt = M + als_fw_at(tid, j0);
#pragma unroll
                    for (int c = 0; c < 32; ++c) zr = __builtin_fmaf(-Lt[c], xs[c], zr);
                } else if (tid >= j0 && tid < j0 + 32) {
                    zr = zc * di;
                }
            }
            for (int k = T - 1; k >= 0; --k) {   // L^T x = z
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
                    const float* Lt = M + als_fw_at(j0, tid);
#pragma unroll
                    for (int c = 31; c >= 0; --c) zr = __builtin_fmaf(-Lt[c * (j0 + 33)], xs[c], zr);
                } else if (tid < j0 + 32) {
                    zr = zc * di;
                }
            }
            if (p.bias) {   // b = (c - x . s) / (n_c + 1e-10), the same tree in every wave
                if (tid < VD) prod[tid] = static_cast<double>(zr) * svv[tid];
                __syncthreads();
                double v = lane < VD ? prod[lane] : 0.0;
                if (VD > 64 && lane + 64 < VD) v += prod[lane + 64];
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);   // a butterfly: the same tree, so the same bits, in every lane
                b = (csum - v) / nc;
            }
        }
        if (tid < D) p.out[static_cast<size_t>(wk.row) * VD + tid] = zr;
        if (p.bias && tid == 0) p.bias[wk.row] = static_cast<float>(b);
    }
}

}  // namespace bfh
