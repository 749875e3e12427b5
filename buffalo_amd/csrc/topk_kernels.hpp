// Top-k selection over factor products on gfx950 -- the device code (host side: csrc/topk.hip).
//
// Reference semantics: parallel::dot_topn and parallel::quickselect (the reference's parallel/_core.hpp:37-142).
//
// Two kernels per batch of queries:
//   topk_scores_kernel  S[b][j] = P[q_b] . Q[j] on the matrix cores (v_mfma_f32_32x32x2_f32, exact fp32
//                       products, fp32 accumulation).  A wave owns 32 queries; its A operands (the query
//                       rows, <= 128 columns per K-chunk) stay in registers while it sweeps item tiles of
//                       32 rows whose B operands stream in as float4s; the four waves of a block sweep
//                       the same tiles for different queries, so each Q row leaves L2 once per 128
//                       queries.  Lane (i, h) supplies columns [h*W/2, (h+1)*W/2) of row i to both
//                       operands -- the MFMA sums over k in any order, so the two half-waves simply take
//                       the two halves of the chunk (contiguous float4 loads, no transposition).
//   topk_select_kernel  one block per query row: 4-pass radix select (8 bits per pass, LDS histogram)
//                       of the k-th largest admissible score, ordered collection of the boundary ties,
//                       bitonic sort of the <= k survivors in LDS by (score desc, index desc).
// Selection is exact (bit-level on the scores the first kernel produced); the scores differ from the
// reference's Eigen dot products only by fp32 summation order.
// The selection kernels have seen-aware instances (template flag SEEN; recommend_unseen and the validation
// ranking): a user's training row is excluded inside the selection.  The score kernels know no users.
// topk_normalize_kernel (most_similar) makes the row-normalised copy of a factor matrix that the same two kernels then rank: the bits of
// the reference's numpy line, summation order included (at the end of this file).
// topk_half_sqnorm_kernel / topk_sqdist_kernel ("score_func" = 1): the per-column bias that turns the same ranking into a ranking by
// squared distance, and the distances of the listed keys (at the end of this file as well).
#pragma once
#include <cfloat>

#include "common.hpp"
#include "pairwise_sum.hpp"

namespace bfh {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kWaveHistBins = 4096;   // uint32 per wave
constexpr int kSampleCap = 512;      // entries of a row's sample segment (normally kk plus the ties at the threshold)

// ------------------------------------------------------------------------------------------------
// Keys, composites, the admission rule, the sort and the row write-out: shared by every selection kernel
// ------------------------------------------------------------------------------------------------
// order-preserving map: smaller key <=> larger score (-0 and +0 coincide)
__device__ __forceinline__ uint32_t desc_key(float s) {
    s += 0.0f;
    uint32_t u = __builtin_bit_cast(uint32_t, s);
    u = (u >> 31) ? ~u : (u | 0x80000000u);
    return ~u;
}
__device__ __forceinline__ float key_score(uint32_t k) {
    const uint32_t u = ~k;
    return __builtin_bit_cast(float, (u >> 31) ? (u ^ 0x80000000u) : ~u);
}
// sort composite: ascending = (score desc, column desc)
__device__ __forceinline__ unsigned long long pack(uint32_t key, uint32_t j) { return (static_cast<unsigned long long>(key) << 32) | (0xFFFFFFFFu - j); }
__device__ __forceinline__ int32_t packed_column(unsigned long long c) { return static_cast<int32_t>(0xFFFFFFFFu - static_cast<uint32_t>(c & 0xFFFFFFFFull)); }
__device__ __forceinline__ float packed_score(unsigned long long c) { return key_score(static_cast<uint32_t>(c >> 32)); }

__device__ __forceinline__ bool pool_bit(uint32_t word, int j) { return ((word >> (j & 31)) & 1u) != 0u; }   // word = pool[j >> 5]

struct AdmitArgs {
    const float* Qb;          // nullable: added to every score
    const uint32_t* pool;     // nullable bitmap over columns: columns outside it are never candidates
    const int32_t* self_idx;  // nullable: column excluded for the row (dot_topn with P == Q)
    int rule_flt_min;         // dot_topn: only scores > FLT_MIN are admissible
};

// The admission rule for column j with raw score s: self exclusion, pool bitmap, bias, FLT_MIN rule; key = desc_key of the (biased)
// score.  It is written out twice.  topk_admit is the branch-free form of the two wave kernels: `ok` is the caller's own precondition
// (the slot holds an entry), `bias` = Qb[j] and `word` = pool[j >> 5] are the caller's already-loaded values (read only where a.Qb /
// a.pool are set), not pointers -- the wave kernels fetch them in straight-line groups (see topk_thr_wave_kernel); `biased`: s carries
// the bias already (sample-segment entries); key = 0 where not admitted.  topk_select_kernel's key_of is the early-out form: self,
// [seen,] pool, then the bias and the FLT_MIN rule, each load issued only for a column that is still in.  Calling topk_admit from key_of
// made the validation ranking 2 % slower, so the block kernel keeps its own copy; a change to the rule goes into both.
__device__ __forceinline__ bool topk_admit(const AdmitArgs& a, bool ok, int j, int self, float s, float bias, bool biased, uint32_t word, uint32_t& key) {
    if (a.Qb && !biased) s += bias;
    ok = ok && j != self;
    if (a.pool) ok = ok && pool_bit(word, j);
    if (a.rule_flt_min) ok = ok && s > FLT_MIN;
    key = ok ? desc_key(s) : 0u;
    return ok;
}

// Bitonic sort of the n (a power of two) LDS entries v[] by NT threads, ascending by `after(x, y)` = "x belongs behind y".
// `sync` orders one compare-exchange step against the next (__syncthreads for a block, wave_lds_sync for one wave); the caller
// syncs before the call, the last step is synced on return.
template <int NT, typename T, typename Sync, typename After>
__device__ __forceinline__ void lds_bitonic_sort(T* v, int n, int tid, Sync sync, After after) {
    for (int size = 2; size <= n; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (n >> 1); t += NT) {
                const int lo = ((t & ~(stride - 1)) << 1) | (t & (stride - 1));
                const int hi = lo | stride;
                const bool up = (lo & size) == 0;
                const T x = v[lo], y = v[hi];
                if (after(x, y) == up) { v[lo] = y; v[hi] = x; }
            }
            sync();
        }
}
__device__ __forceinline__ bool packed_after(unsigned long long x, unsigned long long y) { return x > y; }

struct OutArgs {
    int32_t* keys;            // [.., k]
    float* scores;            // nullable (quickselect, rank_unseen)
    int k, kk;                // output width, min(k, cols[, pool_size])
    int q0;                   // output row (and self_idx / seen_row entry) of row 0
    const int32_t* out_row;   // nullable: output row of row b (else q0 + b); self_idx is then indexed by b
};

// output row `orow` from the sorted composites: kk_eff entries, then the -1 / FLT_MIN / 0 padding (_core.hpp:26 / :134-137)
template <int NT>
__device__ __forceinline__ void write_row(const OutArgs& o, int orow, const unsigned long long* sel, int kk_eff, int tid) {
    int32_t* ok = o.keys + static_cast<size_t>(orow) * o.k;
    float* os = o.scores ? o.scores + static_cast<size_t>(orow) * o.k : nullptr;
    for (int r = tid; r < o.k; r += NT) {
        if (r < kk_eff) {
            const unsigned long long c = sel[r];
            ok[r] = packed_column(c);
            if (os) os[r] = packed_score(c);
        } else {
            ok[r] = -1;
            if (os) os[r] = r < o.kk ? FLT_MIN : 0.0f;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Candidate matrix -> MFMA operand order, once per call (14 MB at ML-20M): Qp[((t*16 + v)*64 + lane)] (float4) =
// Q[32 t + (lane&31)][kc + (lane>>5)*W/2 + 4v .. +3].  A wave's B-operand load in the score kernel is then ONE
// contiguous KiB instead of 64 row-strided 16-byte pieces in 64 different cache lines -- with the strided form the
// texture-address unit of the CU was as busy as the matrix cores.  Rows beyond q_rows and float4s beyond the chunk
// are zero.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void topk_pack_kernel(const float* __restrict__ Q, int q_rows, int ld, int kc, int W, float4* __restrict__ Qp,
                                                        int n_tiles) {
    const int64_t idx = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;   // (t, v, lane)
    if (idx >= static_cast<int64_t>(n_tiles) * 16 * 64) return;
    const int lane = static_cast<int>(idx & 63), v = static_cast<int>((idx >> 6) & 15), t = static_cast<int>(idx >> 10);
    const int j = t * 32 + (lane & 31);
    float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j < q_rows && v < W / 8) out = *reinterpret_cast<const float4*>(Q + static_cast<int64_t>(j) * ld + kc + (lane >> 5) * (W / 2) + 4 * v);
    Qp[idx] = out;
}

// ------------------------------------------------------------------------------------------------
// S[b][j] (+)= sum_{c in [kc, kc+W)} A[row(b)][c] * Q[j][c]
//   A row of query b: P + (qidx ? qidx[q0+b] : q0+b) * ld.  W = min(128, d_pad - kc), W % 8 == 0.
// grid.x = item-tile groups, grid.y = query blocks of 128; block = 256 threads.
// ------------------------------------------------------------------------------------------------
// The fused form (FILTER): the tile's scores never reach HBM.  Every query row carries a threshold -- the kk-th best
// admissible score of a SAMPLE of the columns (the first C0), i.e. a lower bound of the final kk-th best -- and the
// epilogue appends the (column, score) pairs at or above it to the row's candidate segment of this tile group: a few
// hundred of 27 K columns.  Slots come from a per-wave LDS counter (one wave owns a row within a tile group, so no
// global atomics); a segment that overflows is noticed by the select kernel, which sends the row to the dense path.
struct FilterArgs {
    const float* thr;       // [nq] batch-local thresholds on score (+ bias)
    const float* Qb;        // nullable: added to every score before the comparison (as topk_admit does)
    const uint32_t* pool;   // nullable bitmap over columns: columns outside it are never candidates
    uint2* cand;            // [(b * gridDim.x + blockIdx.x) * cap_seg + slot] = (column, bits of the raw score)
    int* cand_cnt;          // [b * gridDim.x + blockIdx.x] candidates seen (> cap_seg: overflow)
    int cap_seg;
    int t_first;            // first tile of the sweep: the sampled columns in front of it reach the selection from their dense scores
};

// FULL: the K-chunk is a whole 128 columns (nv == 16): no per-float4 guards, straight-line MFMA stream
template <bool FULL, bool FILTER>
__global__ __launch_bounds__(256, 3) void topk_scores_kernel(const float* __restrict__ P, const int32_t* __restrict__ qidx, int q0, int nq,
                                                             const float4* __restrict__ Qp, int q_rows, int ld, int kc, int W, float* __restrict__ S,
                                                             size_t ld_s, int tiles_per_block, int accumulate, FilterArgs f) {
    __shared__ int s_cnt[FILTER ? 4 : 1][32];
    __shared__ float s_thr[FILTER ? 4 : 1][32];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int half = lane >> 5, col = lane & 31;
    const int b0q = (blockIdx.y * 4 + wv) * 32;   // first query (batch-local) of this wave
    if (b0q >= nq) return;
    if constexpr (FILTER) {
        if (lane < 32) {
            s_cnt[wv][lane] = 0;
            // rows beyond nq (their A operand is row nq - 1 again) must keep nothing -- their segments do not exist.  NaN, not +inf:
            // no score compares >= NaN, while a +inf SCORE is >= a +inf threshold and was written behind the end of `cand`
            s_thr[wv][lane] = b0q + lane < nq ? f.thr[b0q + lane] : __builtin_nanf("");
        }
        wave_lds_sync();
    }
    const int nv = W / 8;                        // float4s per lane and row
    const int koff = kc + half * (W / 2);
    // A operands: query row b0 + col, this half's columns
    int bq = b0q + col;
    if (bq >= nq) bq = nq - 1;                   // clamped rows compute garbage that is never stored
    const int64_t prow = qidx ? qidx[q0 + bq] : (q0 + bq);
    const float4* ap = reinterpret_cast<const float4*>(P + prow * ld + koff);
    float4 a[16];
#pragma unroll
    for (int v = 0; v < 16; ++v) a[v] = (FULL || v < nv) ? ap[v] : make_float4(0.f, 0.f, 0.f, 0.f);

    const int n_tiles = (q_rows + 31) / 32;
    const int t_begin = (FILTER ? f.t_first : 0) + blockIdx.x * tiles_per_block;
    int t_end = t_begin + tiles_per_block;
    if (t_end > n_tiles) t_end = n_tiles;
    // B operands of a tile in two halves of 8 float4s: the second half of tile t and the first half of tile t+1 are in
    // flight while the first / second half's 32 MFMAs run (no wave waits for a whole tile's loads with an idle pipe)
    auto tile_row = [&](int t) { return Qp + (static_cast<int64_t>(t) * 16 * 64 + lane); };   // float4 v of the tile at [v * 64]
    float4 b0[8], b1[8];
    auto mfma4 = [](f32x16 acc, const float4& x, const float4& y) {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.x, y.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.y, y.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.z, y.z, acc, 0, 0, 0);
        return __builtin_amdgcn_mfma_f32_32x32x2f32(x.w, y.w, acc, 0, 0, 0);
    };
    if (t_begin < t_end) {
        const float4* bp = tile_row(t_begin);
#pragma unroll
        for (int v = 0; v < 8; ++v)
            if (FULL || v < nv) b0[v] = bp[v * 64];
    }
    for (int t = t_begin; t < t_end; ++t) {
        const bool jok = t * 32 + col < q_rows;
        const float4* bp = tile_row(t);
#pragma unroll
        for (int v = 0; v < 8; ++v)
            if (FULL || 8 + v < nv) b1[v] = bp[(8 + v) * 64];
        f32x16 acc;
        float* Sl = FILTER ? nullptr : S + static_cast<size_t>(b0q + 4 * half) * ld_s + t * 32 + col;   // C layout: row (e&3)+8(e>>2)+4half, col lane&31
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int r = (e & 3) + 8 * (e >> 2);
            if constexpr (FILTER) acc[e] = 0.f;
            else acc[e] = (accumulate && jok && b0q + 4 * half + r < nq) ? Sl[static_cast<size_t>(r) * ld_s] : 0.f;
        }
#pragma unroll
        for (int v = 0; v < 8; ++v)
            if (FULL || v < nv) acc = mfma4(acc, a[v], b0[v]);
        if (t + 1 < t_end) {
            const float4* bn = tile_row(t + 1);
#pragma unroll
            for (int v = 0; v < 8; ++v)
                if (FULL || v < nv) b0[v] = bn[v * 64];
        }
#pragma unroll
        for (int v = 0; v < 8; ++v)
            if (FULL || 8 + v < nv) acc = mfma4(acc, a[8 + v], b1[v]);
        if constexpr (FILTER) {
            const int j = t * 32 + col;
            bool colok = jok;
            if (f.pool && jok) colok = ((f.pool[j >> 5] >> (j & 31)) & 1u) != 0u;
            const float qb = (f.Qb && jok) ? f.Qb[j] : 0.f;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int rr = 4 * half + (e & 3) + 8 * (e >> 2);
                const float sc = f.Qb ? acc[e] + qb : acc[e];   // the very sum topk_admit forms
                if (colok && sc >= s_thr[wv][rr]) {           // rows beyond nq carry NaN: never true
                    const int slot = atomicAdd(&s_cnt[wv][rr], 1);
                    const float raw = acc[e];   // (a bit_cast applied to the vector element itself reads element 0)
                    if (slot < f.cap_seg)
                        f.cand[(static_cast<size_t>(b0q + rr) * gridDim.x + blockIdx.x) * f.cap_seg + slot] =
                            make_uint2(static_cast<uint32_t>(j), __float_as_uint(raw));
                }
            }
        } else if (jok) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int r = (e & 3) + 8 * (e >> 2);
                if (b0q + 4 * half + r < nq) Sl[static_cast<size_t>(r) * ld_s] = acc[e];
            }
        }
    }
    if constexpr (FILTER) {
        wave_lds_sync();
        if (lane < 32 && b0q + lane < nq) f.cand_cnt[static_cast<size_t>(b0q + lane) * gridDim.x + blockIdx.x] = s_cnt[wv][lane];
    }
}

// thr[b] = the kk-th best admissible score of the sampled columns (row q0 + b of the select output), or "everything":
// with the admission rule only scores > FLT_MIN can be listed, so FLT_MIN itself is a valid bound then
__global__ void topk_thr_kernel(const int32_t* __restrict__ keys, const float* __restrict__ scores, int q0, int nb, int k, int kk, int rule_flt_min,
                                float* __restrict__ thr) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nb) return;
    const size_t at = static_cast<size_t>(q0 + b) * k + (kk - 1);
    thr[b] = (kk > 0 && keys[at] >= 0) ? scores[at] : (rule_flt_min ? FLT_MIN : -__builtin_inff());
}

// Arguments of the selection kernels, in groups; each kernel's comment names the groups it reads
struct DenseArgs {            // the row is a dense score row
    const float* S;           // [rows, ld_s]
    size_t ld_s;
    int cols;
};
// the row is the candidate segments topk_scores_kernel<.., FILTER> wrote -- every admissible column at or above a lower bound of
// the kk-th best score, in no particular order -- plus the sampled columns' own candidates (written by topk_thr_wave_kernel from
// the dense sample scores; the filtered sweep then starts behind the sample)
struct ListArgs {
    const uint2* cand;        // nullable (dense row): [(b * n_seg + g) * cap_seg + slot] = (column, bits of the raw score)
    const int* cand_cnt;      // [b * n_seg + g]
    int n_seg, cap_seg;
    int list_cap;             // entries of the LDS list behind the candidate buffer
    uint2* s0_cand;           // nullable (the sweep covered every column): [b * s0_cap + slot]; bit 31 of the column: biased score
    int* s0_cnt;              // [b] (> s0_cap: overflow)
    int s0_cap;
};
// the seen-aware selections (recommend_unseen, the validation ranking of csrc/eval.hip): row b belongs to user row[q0 + b], whose
// training row -- the ascending keys [indptr[u - 1], indptr[u]) of an END-offset CSR -- holds columns that are never candidates
struct SeenArgs {
    const int64_t* indptr;
    const int32_t* keys;
    const int32_t* row;
    int lds_cap;              // runs up to this many keys are searched in LDS, longer ones in HBM.  topk_select_kernel stages them in a
                              // region of their own behind the candidate buffer and the list, topk_list_wave_kernel in its wave's histogram
};
// the training row of user u
__device__ __forceinline__ const int32_t* seen_run(const SeenArgs& s, int u, int& n_seen) {
    const int64_t beg = u > 0 ? s.indptr[u - 1] : 0;
    n_seen = static_cast<int>(s.indptr[u] - beg);
    return s.keys + beg;
}
struct WorkArgs {
    int* redo;                // [0]: rows sent to the dense path (a segment or the list overflowed), [1 + i]: their b
    int* general;             // [0]: rows topk_list_wave_kernel passed on to topk_select_kernel (ties at the k-th place), [1 + i]: their b
    const int* row_list;      // nullable: block x works on row row_list[x] (the `general` rows)
    float* thr;               // topk_thr_wave_kernel: [b] the kk-th best admissible score of the row, or "everything"
};
struct SelectArgs {
    AdmitArgs adm;
    OutArgs out;
    DenseArgs dense;
    ListArgs list;
    SeenArgs seen;
    WorkArgs work;
    int p2;                   // power of two >= kk: sort buffer entries
    int cand_cap;             // entries of the candidate buffer behind the sort buffer (0: multi-pass path only)
};

// One block per row.  Reads adm, out, p2 / cand_cap, work.row_list; the row from `dense`, or -- list mode, list.cand set -- from
// `list` (overflowing rows go to work.redo).  SEEN: the per-row exclusion `seen`, for dense rows and for lists alike (the filtered
// sweep does not know the users: a list carries the row's seen columns at or above the threshold, and key_of drops them here).
template <bool SEEN>
__global__ __launch_bounds__(256) void topk_select_kernel(SelectArgs a) {
    // p2 sort entries, then cand_cap candidates [, then list.list_cap list entries (list mode)] [, then seen.lds_cap keys (SEEN)]
    extern __shared__ __attribute__((aligned(16))) unsigned long long sel[];
    __shared__ int hist[4096];
    __shared__ int part[256];
    __shared__ int s_misc[8];   // 0: chosen bin, 1: remaining, 2: n_gt slots, 3: run_eq, 4..7: wave eq counts / fast-path counters
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int b = a.work.row_list ? a.work.row_list[blockIdx.x] : blockIdx.x;
    const bool list = a.list.cand != nullptr;
    const float* row = list ? nullptr : a.dense.S + static_cast<size_t>(b) * a.dense.ld_s;
    const int orow = a.out.out_row ? a.out.out_row[b] : a.out.q0 + b;
    const int self = a.adm.self_idx ? a.adm.self_idx[a.out.out_row ? b : a.out.q0 + b] : -1;
    uint2* lst = reinterpret_cast<uint2*>(sel + a.p2 + a.cand_cap);
    int cols = a.dense.cols;   // positions the passes run over: columns of the dense row, or entries of the list
    const int32_t* seen = nullptr;   // the row's excluded columns, ascending
    int n_seen = 0;
    if constexpr (SEEN) {
        const int u = a.seen.row[a.out.q0 + b];
        const int64_t beg = u > 0 ? a.seen.indptr[u - 1] : 0;
        n_seen = static_cast<int>(a.seen.indptr[u] - beg);
        seen = a.seen.keys + beg;
        if (n_seen <= a.seen.lds_cap) {   // block-uniform
            int32_t* staged = reinterpret_cast<int32_t*>(sel + a.p2 + a.cand_cap + (list ? a.list.list_cap : 0));   // behind the list
            for (int i = tid; i < n_seen; i += 256) staged[i] = seen[i];
            seen = staged;
            __syncthreads();
        }
    }
    if (list) {
        // gather the segments into one LDS list; a row whose segments or list overflowed is redone densely by the host
        const ListArgs& l = a.list;
        const int n_seg = l.n_seg + (l.s0_cand ? 1 : 0);   // the sample segment comes last
        auto seg_count = [&](int g) { return g < l.n_seg ? l.cand_cnt[static_cast<size_t>(b) * l.n_seg + g] : l.s0_cnt[b]; };
        if (tid == 0) {
            int tot = 0, over = 0;
            for (int g = 0; g < n_seg; ++g) {
                const int c = seg_count(g);
                over |= c > (g < l.n_seg ? l.cap_seg : l.s0_cap);
                tot += c;
            }
            s_misc[6] = tot;
            s_misc[7] = (over || tot > l.list_cap) ? 1 : 0;
        }
        __syncthreads();
        cols = s_misc[6];
        if (s_misc[7]) {   // block-uniform
            if (tid == 0) a.work.redo[1 + atomicAdd(a.work.redo, 1)] = b;
            return;
        }
        int off = 0;
        for (int g = 0; g < n_seg; ++g) {
            const int c = seg_count(g);
            const uint2* seg = g < l.n_seg ? l.cand + (static_cast<size_t>(b) * l.n_seg + g) * l.cap_seg : l.s0_cand + static_cast<size_t>(b) * l.s0_cap;
            for (int i = tid; i < c; i += 256) lst[off + i] = seg[i];
            off += c;
        }
        __syncthreads();
    }
    // position i -> (admissible?, key, column j)
    auto key_of = [&](int i, uint32_t& key, int& j) -> bool {
        float s;
        bool biased = false;   // sample-segment entries carry the bias already (bit 31 of the column)
        if (list) {
            const uint2 c = lst[i];
            j = static_cast<int>(c.x & 0x7FFFFFFFu);
            biased = (c.x >> 31) != 0u;
            s = __builtin_bit_cast(float, c.y);
        } else {
            j = i;
            s = row[i];
        }
        if (j == self) return false;   // the admission rule, early-out form (see topk_admit)
        if constexpr (SEEN) {
            if (sorted_contains(seen, 0, n_seen, j)) return false;
        }
        if (a.adm.pool && !pool_bit(a.adm.pool[j >> 5], j)) return false;
        if (a.adm.Qb && !biased) s += a.adm.Qb[j];
        if (a.adm.rule_flt_min && !(s > FLT_MIN)) return false;
        key = desc_key(s);
        return true;
    };

    // ---------------- fast path: two reads of the row ----------------
    // 12-bit histogram of the key's top bits (sign, exponent, 3 mantissa bits), then ONE more pass that sends
    // everything above the threshold bin to the output list and the bin's members (~1 % of the row) to an LDS
    // candidate buffer, where the remaining 20 bits are resolved.  Falls through to the multi-pass path when the
    // bin overflows the buffer or when ties straddle the k-th place (the reference's tie rule needs column order).
    bool done = false;
    int fast_kk_eff = 0;
    if (a.cand_cap > 0) {
        unsigned long long* cand = sel + a.p2;
        // histogram `hist[0..nbins)` is filled; finds the bin where the running count reaches `want`
        auto find_bin = [&](int nbins, int want) {   // -> s_misc[0] bin (-1: fewer than want in total), [1] remaining inside it, [2] total, [3] bin count
            const int per = nbins / 256;
            int ps = 0;
            for (int q = 0; q < per; ++q) ps += hist[tid * per + q];
            part[tid] = ps;
            __syncthreads();
            if (tid == 0) {
                int tot = 0;
                for (int t = 0; t < 256; ++t) tot += part[t];
                int bin = -1, rem = want, cnt = 0;
                if (tot >= want) {
                    int cum = 0, t = 0;
                    while (cum + part[t] < want) cum += part[t++];
                    int q = t * per;
                    while (cum + hist[q] < want) cum += hist[q++];
                    bin = q;
                    rem = want - cum;
                    cnt = hist[q];
                }
                s_misc[0] = bin; s_misc[1] = rem; s_misc[2] = tot; s_misc[3] = cnt;
            }
            __syncthreads();
        };
        for (int i = tid; i < 4096; i += 256) hist[i] = 0;
        for (int i = tid; i < a.p2; i += 256) sel[i] = ~0ull;
        __syncthreads();
        for (int i = tid; i < cols; i += 256) {
            uint32_t key;
            int j;
            if (key_of(i, key, j)) atomicAdd(&hist[key >> 20], 1);
        }
        __syncthreads();
        find_bin(4096, a.out.kk);
        const int bin1 = s_misc[0], rem1 = s_misc[1], total1 = s_misc[2];
        __syncthreads();
        if (tid == 0) { s_misc[4] = 0; s_misc[5] = 0; }
        __syncthreads();
        const bool all1 = bin1 < 0;
        for (int i = tid; i < cols; i += 256) {
            uint32_t key;
            int j;
            if (!key_of(i, key, j)) continue;
            const int top = static_cast<int>(key >> 20);
            if (all1 || top < bin1) sel[atomicAdd(&s_misc[4], 1)] = pack(key, j);
            else if (top == bin1) {
                const int c = atomicAdd(&s_misc[5], 1);
                if (c < a.cand_cap) cand[c] = pack(key, j);
            }
        }
        __syncthreads();
        const int n_cand = s_misc[5];
        if (all1) {
            done = true;
            fast_kk_eff = total1;
        } else if (n_cand <= a.cand_cap) {
            for (int i = tid; i < 1024; i += 256) hist[i] = 0;
            __syncthreads();
            for (int i = tid; i < n_cand; i += 256) atomicAdd(&hist[(static_cast<uint32_t>(cand[i] >> 32) >> 10) & 1023u], 1);
            __syncthreads();
            find_bin(1024, rem1);
            const int bin2 = s_misc[0], rem2 = s_misc[1];
            __syncthreads();
            for (int i = tid; i < 1024; i += 256) hist[i] = 0;
            __syncthreads();
            for (int i = tid; i < n_cand; i += 256) {
                const uint32_t k = static_cast<uint32_t>(cand[i] >> 32);
                if (static_cast<int>((k >> 10) & 1023u) == bin2) atomicAdd(&hist[k & 1023u], 1);
            }
            __syncthreads();
            find_bin(1024, rem2);
            const int bin3 = s_misc[0], need_eq = s_misc[1], eq_cnt = s_misc[3];
            __syncthreads();
            if (need_eq == eq_cnt) {   // no tie straddles the k-th place: everything up to the threshold key is in
                const uint32_t thr = (static_cast<uint32_t>(bin1) << 20) | (static_cast<uint32_t>(bin2) << 10) | static_cast<uint32_t>(bin3);
                for (int i = tid; i < n_cand; i += 256)
                    if (static_cast<uint32_t>(cand[i] >> 32) <= thr) sel[atomicAdd(&s_misc[4], 1)] = cand[i];
                done = true;
                fast_kk_eff = a.out.kk;
            }
        }
        __syncthreads();
    }

    int kk_eff = fast_kk_eff;
    if (!done) {   // ---------------- multi-pass path (8 bits per pass over the row) ----------------
        uint32_t prefix = 0, mask = 0;
        int remaining = a.out.kk, total = 0, eq_total = 0;
        bool take_all = false;
        for (int pass = 0; pass < 4 && !take_all; ++pass) {
            const int shift = 24 - 8 * pass;
            hist[tid] = 0;
            __syncthreads();
            for (int i = tid; i < cols; i += 256) {
                uint32_t key;
                int j;
                if (key_of(i, key, j) && (key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1);
            }
            __syncthreads();
            if (tid == 0) {
                int cum = 0, bin = 255, rem = remaining;
                int tot = 0;
                for (int i = 0; i < 256; ++i) tot += hist[i];
                if (pass == 0 && tot < remaining) {
                    bin = -1;   // fewer admissible candidates than slots: take them all
                } else {
                    for (int i = 0; i < 256; ++i) {
                        if (cum + hist[i] >= rem) { bin = i; break; }
                        cum += hist[i];
                    }
                    rem -= cum;
                }
                s_misc[0] = bin;
                s_misc[1] = rem;
                s_misc[2] = tot;
                s_misc[3] = bin >= 0 ? hist[bin] : 0;
            }
            __syncthreads();
            const int bin = s_misc[0];
            if (pass == 0) total = s_misc[2];
            if (bin < 0) { take_all = true; break; }
            remaining = s_misc[1];
            eq_total = s_misc[3];
            prefix |= static_cast<uint32_t>(bin) << shift;
            mask |= 255u << shift;
            __syncthreads();
        }
        kk_eff = take_all ? total : a.out.kk;
        // now: keys < prefix are in, `remaining` of the eq_total keys == prefix are in (the first ones by column)
        for (int i = tid; i < a.p2; i += 256) sel[i] = ~0ull;
        if (tid == 0) { s_misc[2] = 0; s_misc[3] = 0; }
        __syncthreads();
        const int n_gt = kk_eff - (take_all ? 0 : remaining);
        // Boundary ties (more candidates equal to the k-th score than slots left): the reference's running list
        // (_core.hpp:115-128) admits an equal-score candidate only while fewer than kk candidates >= that score
        // have been seen, and every later better candidate then evicts the OLDEST of them.  Closed form: let F be
        // the first kk candidates (by index) with score >= t and A the candidates == t inside F; the survivors are
        // the `remaining` members of A with the HIGHEST indices.
        const bool ordered = !take_all && remaining < eq_total;
        if (kk_eff > 0) {
            for (int i = tid; i < cols; i += 256) {
                uint32_t key = 0;
                int j;
                if (!key_of(i, key, j)) continue;
                if (take_all || key < prefix) sel[atomicAdd(&s_misc[2], 1)] = pack(key, j);
                else if (!ordered && key == prefix) sel[n_gt + atomicAdd(&s_misc[3], 1)] = pack(key, j);   // all eq_total == remaining of them
            }
        }
        if (ordered) {
            __shared__ int s_run[4];    // 0: candidates >= t so far, 1: candidates == t so far, 2: |A|, 3: done
            __shared__ int s_wave[8];   // per-wave counts of the current 256-column step: [0..3] >= t, [4..7] == t
            if (list) {
                // the tie rule walks the candidates in COLUMN order; the list is in arrival order: sort it by column
                // (every column at or above the k-th score is in the list, so the walk sees what the dense walk sees)
                int n2 = 2;
                while (n2 < cols) n2 <<= 1;
                __syncthreads();
                for (int i = cols + tid; i < n2; i += 256) lst[i] = make_uint2(0xFFFFFFFFu, 0u);
                __syncthreads();
                lds_bitonic_sort<256>(lst, n2, tid, [] { __syncthreads(); },
                                      [](uint2 x, uint2 y) { return (x.x & 0x7FFFFFFFu) > (y.x & 0x7FFFFFFFu); });   // (bit 31: bias flag)
            }
            if (tid < 4) s_run[tid] = 0;
            __syncthreads();
            for (int phase = 0; phase < 2; ++phase) {
                // phase 0 finds |A| (the == t count when the kk-th candidate >= t arrives); phase 1 places the survivors
                const int cnt_a = s_run[2];
                __syncthreads();
                if (tid < 2) s_run[tid] = 0;
                __syncthreads();
                for (int base = 0; base < cols; base += 256) {
                    const int i = base + tid;
                    uint32_t key = 0;
                    int j = 0;
                    const bool ok = i < cols && key_of(i, key, j);
                    const bool ge = ok && key <= prefix, eq = ok && key == prefix;
                    const unsigned long long bge = __ballot(ge), beq = __ballot(eq);
                    const unsigned long long below = (1ull << lane) - 1ull;
                    if (lane == 0) { s_wave[wv] = __popcll(bge); s_wave[4 + wv] = __popcll(beq); }
                    __syncthreads();
                    int ge_rank = s_run[0] + __popcll(bge & below), eq_rank = s_run[1] + __popcll(beq & below);
                    for (int w = 0; w < wv; ++w) { ge_rank += s_wave[w]; eq_rank += s_wave[4 + w]; }
                    if (phase == 0) {
                        if (ge && ge_rank == a.out.kk - 1) s_run[2] = eq_rank + (eq ? 1 : 0);
                    } else if (eq && eq_rank < cnt_a && eq_rank >= cnt_a - remaining) {
                        sel[n_gt + (eq_rank - (cnt_a - remaining))] = pack(key, j);
                    }
                    __syncthreads();
                    if (tid == 0) {
                        s_run[0] += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
                        s_run[1] += s_wave[4] + s_wave[5] + s_wave[6] + s_wave[7];
                    }
                    __syncthreads();
                    if (s_run[phase == 0 ? 0 : 1] >= (phase == 0 ? a.out.kk : cnt_a)) break;   // block-uniform
                }
                __syncthreads();
            }
        }
    }
    __syncthreads();
    lds_bitonic_sort<256>(sel, a.p2, tid, [] { __syncthreads(); }, packed_after);
    write_row<256>(a.out, orow, sel, kk_eff, tid);
}

// ------------------------------------------------------------------------------------------------
// One WAVE per row, for rows that fit in registers: no block barriers, no LDS histograms.  The k-th smallest key of the
// row is found bit by bit (32 rounds of "how many live keys have a 0 here", one DPP wave sum each) over the keys the
// lanes hold; a 256-thread block per row spends most of its time in the fixed cost of its barriers when the row has a
// few hundred entries, as the candidate lists of the fused path do.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int wave_incl_scan_i32(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __builtin_amdgcn_ds_bpermute(((lane - d) & 63) << 2, v);
        if (lane >= d) v += o;
    }
    return v;
}

// key[s], s < SLOTS, live where bit s of `valid` is set.  Returns the number of live keys m; when m >= kk: kth = the kk-th
// smallest, need_eq = how many of the keys == kth belong to the kk smallest, eq_total = how many there are.
// Three histogram levels over the key's bits 31..20, 19..8, 7..0 in the wave's own LDS histogram `hist` (kWaveHistBins
// words): the live keys that match the prefix found so far are counted by their next digit (LDS atomics), the digit
// holding the kk-th key is located with two wave scans (row totals of the [rows][64] bin matrix, then inside the row).
template <int SLOTS>
__device__ __forceinline__ int wave_kth_key(const uint32_t (&key)[SLOTS], uint64_t valid, int kk, uint32_t* hist, int lane, uint32_t& kth, int& need_eq,
                                            int& eq_total) {
    const int m = wave_sum_i32(__popcll(valid));
    kth = 0u; need_eq = 0; eq_total = 0;
    if (m < kk) return m;
    uint32_t prefix = 0u, mask = 0u;
    int remaining = kk, bin_count = 0;
#pragma unroll
    for (int level = 0; level < 3; ++level) {
        const int shift = level == 0 ? 20 : (level == 1 ? 8 : 0);
        const int nb = level == 2 ? 256 : 4096;
        const int rows = nb / 64;
        uint4* h4 = reinterpret_cast<uint4*>(hist);
        for (int i = lane; i < nb / 4; i += 64) h4[i] = make_uint4(0u, 0u, 0u, 0u);
        wave_lds_sync();
#pragma unroll
        for (int sl = 0; sl < SLOTS; ++sl) {
            const uint32_t k = key[sl];
            if (((valid >> sl) & 1ull) && (k & mask) == prefix) atomicAdd(&hist[(k >> shift) & static_cast<uint32_t>(nb - 1)], 1u);
        }
        wave_lds_sync();
        // row totals: lane r < rows sums bins [64 r, 64 r + 64), read skewed so that the lanes spread over the banks
        int rt = 0;
        if (lane < rows)
            for (int j = 0; j < 64; ++j) rt += static_cast<int>(hist[lane * 64 + ((j + lane) & 63)]);
        const int rincl = wave_incl_scan_i32(rt, lane);
        const unsigned long long rb = __ballot(lane < rows && rincl >= remaining);
        const int r = __builtin_ctzll(rb);   // rb != 0: the matching keys number at least `remaining`
        remaining -= __builtin_amdgcn_readlane(rincl - rt, r);
        const int bv = static_cast<int>(hist[r * 64 + lane]);
        const int bincl = wave_incl_scan_i32(bv, lane);
        const unsigned long long bb = __ballot(bincl >= remaining);
        const int c = __builtin_ctzll(bb);
        remaining -= __builtin_amdgcn_readlane(bincl - bv, c);
        bin_count = __builtin_amdgcn_readlane(bv, c);
        prefix |= static_cast<uint32_t>(r * 64 + c) << shift;
        mask |= static_cast<uint32_t>(nb - 1) << shift;
        wave_lds_sync();
    }
    kth = prefix; need_eq = remaining; eq_total = bin_count;
    return m;
}

// Both wave kernels fetch a row's entries in straight-line groups of 16 loads per lane: a load that sits behind the
// admission branches of the previous entry is not issued before that entry is done, and 64 serialised round trips per row
// made the first version of these kernels 10x slower than their arithmetic.

// thresholds of the fused path from the dense scores of the sampled columns (dense.cols <= 4096: 64 keys per lane):
// thr[b] = the kk-th best admissible score, or -- with fewer than kk of them -- "everything" (with the admission rule only
// scores > FLT_MIN can be listed, so FLT_MIN is a valid bound then).  The sampled columns that reach the threshold are
// written out as the row's sample segment (list.s0_*), so that the filtered sweep can start behind the sample.
// Reads adm, dense, out.kk / out.q0, list.s0_*, work.thr.  grid: ceil(rows / 4) blocks of 4 waves; dynamic LDS: 4 histograms.
// SEEN (reads seen): the user's seen columns are no candidates of the sample either, so the threshold is the kk-th best UNSEEN
// admissible score of the sample -- a lower bound of the row's final kk-th best -- and a sample with fewer than kk of them bounds
// nothing.  The sampled columns are the first `cols`, so the seen ones are a prefix of the user's ascending run: the wave marks them
// in an LDS bitmap (4,096 bits in front of its histogram, which wave_kth_key clears before use) and every lane drops its own.
template <bool SEEN>
__global__ __launch_bounds__(256, 2) void topk_thr_wave_kernel(SelectArgs a, int rows) {
    extern __shared__ __attribute__((aligned(16))) uint32_t whist_dyn[];   // 4 * kWaveHistBins words
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= rows) return;
    const int cols = a.dense.cols, kk = a.out.kk;
    const float* row = a.dense.S + static_cast<size_t>(b) * a.dense.ld_s;
    const int self = a.adm.self_idx ? a.adm.self_idx[a.out.q0 + b] : -1;
    uint32_t key[64];
    uint64_t valid = 0ull;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float rawv[16], qb[16];
        uint32_t pw[16];
        auto col_of = [&](int t) { return min((c * 16 + t) * 64 + lane, cols - 1); };   // (clamped: loads beyond the row are not used)
#pragma unroll
        for (int t = 0; t < 16; ++t) rawv[t] = row[col_of(t)];
        if (a.adm.Qb) {
#pragma unroll
            for (int t = 0; t < 16; ++t) qb[t] = a.adm.Qb[col_of(t)];
        }
        if (a.adm.pool) {
#pragma unroll
            for (int t = 0; t < 16; ++t) pw[t] = a.adm.pool[col_of(t) >> 5];
        }
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int sl = c * 16 + t;
            const int j = sl * 64 + lane;
            const bool ok = topk_admit(a.adm, j < cols, j, self, rawv[t], a.adm.Qb ? qb[t] : 0.f, false, a.adm.pool ? pw[t] : 0u, key[sl]);
            valid |= static_cast<uint64_t>(ok ? 1 : 0) << sl;
        }
        __builtin_amdgcn_sched_barrier(0);   // one group's loads in flight at a time: 64 keys + 48 group registers, not 256
    }
    if constexpr (SEEN) {
        uint32_t* bm = whist_dyn + (threadIdx.x >> 6) * kWaveHistBins;   // bit j: column j < cols <= 4096 is in the user's training row
        int n_seen;
        const int32_t* seen = seen_run(a.seen, a.seen.row[a.out.q0 + b], n_seen);
        for (int i = lane; i < 128; i += 64) bm[i] = 0u;
        wave_lds_sync();
        for (int base = 0; base < n_seen; base += 64) {
            const int32_t s = base + lane < n_seen ? seen[base + lane] : cols;
            if (s < cols) atomicOr(&bm[s >> 5], 1u << (s & 31));
            if (__ballot(s < cols) != ~0ull) break;   // ascending keys: the rest of the run lies behind the sample
        }
        wave_lds_sync();
        uint64_t seen_mask = 0ull;
#pragma unroll
        for (int sl = 0; sl < 64; ++sl) seen_mask |= static_cast<uint64_t>((bm[sl * 2 + (lane >> 5)] >> (lane & 31)) & 1u) << sl;   // column sl * 64 + lane
        valid &= ~seen_mask;
        wave_lds_sync();   // the bitmap is read before wave_kth_key clears the histogram
    }
    uint32_t kth; int need_eq, eq_total;
    const int m = wave_kth_key<64>(key, valid, kk, whist_dyn + (threadIdx.x >> 6) * kWaveHistBins, lane, kth, need_eq, eq_total);
    if (lane == 0) a.work.thr[b] = m >= kk ? key_score(kth) : (a.adm.rule_flt_min ? FLT_MIN : -__builtin_inff());
    if (a.list.s0_cand) {   // the admissible sampled columns at or above the threshold: the kk best plus the ties at the k-th place
        uint2* out = a.list.s0_cand + static_cast<size_t>(b) * a.list.s0_cap;
        int n0 = 0;
#pragma unroll
        for (int sl = 0; sl < 64; ++sl) {
            const bool win = ((valid >> sl) & 1ull) && (m < kk || key[sl] <= kth);
            const unsigned long long mask = __ballot(win);
            const int at = n0 + __popcll(mask & ((1ull << lane) - 1ull));
            // bit 31 of the column: the score already carries the bias (key -> score is exact, so the selection sees the same key)
            if (win && at < a.list.s0_cap) out[at] = make_uint2(static_cast<uint32_t>(sl * 64 + lane) | 0x80000000u, __float_as_uint(key_score(key[sl])));
            n0 += __popcll(mask);
            if ((sl & 7) == 7) __builtin_amdgcn_sched_barrier(0);   // keep the 64 ballots from being formed all at once (SGPR spills)
        }
        if (lane == 0) a.list.s0_cnt[b] = n0;
    }
}

// selection over the candidate lists of the fused path, one wave per row (lists of <= 2048 entries: 32 per lane).
// A row whose segments or list overflowed goes to work.redo (dense path); a row with ties straddling the k-th place goes to
// work.general (topk_select_kernel's list mode, which walks the ties in column order).
// Reads adm, out, list, p2, work.redo / work.general.  Dynamic LDS: 4 histograms + 4 * p2 * 8 bytes.
// SEEN (reads seen): the list's seen columns are dropped before the selection.  The rule is key_of's conjunction -- self, seen, pool,
// bias, FLT_MIN -- with the seen test issued last, for the entries that are still in.  A training row of up to min(seen.lds_cap, kWaveHistBins) keys is searched in the wave's histogram
// words, which are free until wave_kth_key clears them; a longer one in HBM.
template <bool SEEN>
__global__ __launch_bounds__(256) void topk_list_wave_kernel(SelectArgs a, int rows) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long wsel[];   // 4 histograms (kWaveHistBins words), then 4 * p2 sort entries
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.x * 4 + wv;
    if (b >= rows) return;
    const ListArgs& l = a.list;
    uint32_t* whist = reinterpret_cast<uint32_t*>(wsel) + static_cast<size_t>(wv) * kWaveHistBins;
    unsigned long long* sel = wsel + (4 * kWaveHistBins) / 2 + static_cast<size_t>(wv) * a.p2;
    const int self = a.adm.self_idx ? a.adm.self_idx[a.out.q0 + b] : -1;
    // segment ends (n_seg <= 8 sweep segments, then the sample segment): seg_end[g] = entries of the segments 0..g
    int seg_end[9];
    int over = 0, tot = 0;
#pragma unroll
    for (int g = 0; g < 9; ++g) {
        int c = 0;
        if (g < 8 ? g < l.n_seg : l.s0_cand != nullptr) {
            c = g < 8 ? l.cand_cnt[static_cast<size_t>(b) * l.n_seg + g] : l.s0_cnt[b];
            over |= c > (g < 8 ? l.cap_seg : l.s0_cap);
        }
        tot += c;
        seg_end[g] = tot;
    }
    if (over || tot > l.list_cap) {
        if (lane == 0) a.work.redo[1 + atomicAdd(a.work.redo, 1)] = b;
        return;
    }
    uint32_t key[32], col[32];
    uint64_t valid = 0ull;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        uint2 cv[16];
        float qb[16];
        uint32_t pw[16];
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            int i = (c * 16 + t) * 64 + lane;
            if (i >= tot) i = tot > 0 ? tot - 1 : 0;
            int g = 0, beg = 0;
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (i >= seg_end[q]) { g = q + 1; beg = seg_end[q]; }
            const uint2* src = g < 8 ? l.cand + (static_cast<size_t>(b) * l.n_seg + g) * l.cap_seg : l.s0_cand + static_cast<size_t>(b) * l.s0_cap;
            cv[t] = tot > 0 ? src[i - beg] : make_uint2(0u, 0u);
        }
        if (a.adm.Qb) {
#pragma unroll
            for (int t = 0; t < 16; ++t) qb[t] = a.adm.Qb[cv[t].x & 0x7FFFFFFFu];
        }
        if (a.adm.pool) {
#pragma unroll
            for (int t = 0; t < 16; ++t) pw[t] = a.adm.pool[(cv[t].x & 0x7FFFFFFFu) >> 5];
        }
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int sl = c * 16 + t;
            const int i = sl * 64 + lane;
            const int j = static_cast<int>(cv[t].x & 0x7FFFFFFFu);
            const bool biased = (cv[t].x >> 31) != 0u;   // sample-segment entries carry the bias already
            const bool ok = topk_admit(a.adm, i < tot, j, self, __uint_as_float(cv[t].y), a.adm.Qb ? qb[t] : 0.f, biased, a.adm.pool ? pw[t] : 0u, key[sl]);
            col[sl] = static_cast<uint32_t>(j);
            valid |= static_cast<uint64_t>(ok ? 1 : 0) << sl;
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (SEEN) {
        int n_seen;
        const int32_t* seen = seen_run(a.seen, a.seen.row[a.out.q0 + b], n_seen);
        if (n_seen <= min(a.seen.lds_cap, kWaveHistBins)) {   // wave-uniform
            int32_t* staged = reinterpret_cast<int32_t*>(whist);
            for (int i = lane; i < n_seen; i += 64) staged[i] = seen[i];
            seen = staged;
            wave_lds_sync();
        }
#pragma unroll
        for (int sl = 0; sl < 32; ++sl)
            if (((valid >> sl) & 1ull) && sorted_contains(seen, 0, n_seen, static_cast<int32_t>(col[sl]))) valid &= ~(1ull << sl);
        wave_lds_sync();   // the staged keys are read before wave_kth_key clears the histogram
    }
    uint32_t kth; int need_eq, eq_total;
    const int m = wave_kth_key<32>(key, valid, a.out.kk, whist, lane, kth, need_eq, eq_total);
    const bool take_all = m < a.out.kk;
    if (!take_all && need_eq < eq_total) {   // ties straddle the k-th place: the reference's rule needs column order
        if (lane == 0) a.work.general[1 + atomicAdd(a.work.general, 1)] = b;
        return;
    }
    const int kk_eff = take_all ? m : a.out.kk;
    for (int i = lane; i < a.p2; i += 64) sel[i] = ~0ull;
    wave_lds_sync();
    int base = 0;
#pragma unroll
    for (int sl = 0; sl < 32; ++sl) {
        const bool win = ((valid >> sl) & 1ull) && (take_all || key[sl] <= kth);
        const unsigned long long mask = __ballot(win);
        if (win) sel[base + __popcll(mask & ((1ull << lane) - 1ull))] = pack(key[sl], col[sl]);
        base += __popcll(mask);
    }
    wave_lds_sync();
    lds_bitonic_sort<64>(sel, a.p2, lane, [] { wave_lds_sync(); }, packed_after);
    write_row<64>(a.out, a.out.q0 + b, sel, kk_eff, lane);
}

// ------------------------------------------------------------------------------------------------
// Small steps around the selections
// ------------------------------------------------------------------------------------------------
// The rows the fused path handed back, for the dense step.  On entry side[2n + i] = the i-th row (batch-local, ascending); on return
// side[i] = its row of dP, side[n + i] = its query id (self exclusion; the user of a seen-aware call), side[2n + i] = its output row.
// The ids are read where they are: the validation ranking's exist on the device alone.
__global__ void topk_redo_side_kernel(int32_t* __restrict__ side, int n, int q0, const int32_t* __restrict__ qidx, const int32_t* __restrict__ ids) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int q = q0 + side[2 * static_cast<size_t>(n) + i];
    side[i] = qidx ? qidx[q] : q;
    side[static_cast<size_t>(n) + i] = ids[q];
    side[2 * static_cast<size_t>(n) + i] = q;
}

// recommend_unseen: the pool of row b is the call's pool (every column without one, `pool_cols` columns) minus the user's training row,
// so row b's slots from kk_b = min(kk, columns of that pool) on read (-1, 0.0).  The selections know the call's kk alone and wrote
// (-1, FLT_MIN) there.  One wave per row counts the user's distinct seen columns inside the pool.  grid: ceil(nq / 4) blocks of 4 waves.
__global__ __launch_bounds__(256) void topk_unseen_padding_kernel(SeenArgs s, const uint32_t* __restrict__ pool, int pool_cols, int nq, int k, int kk,
                                                                  const int32_t* __restrict__ keys, float* __restrict__ scores) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= nq) return;
    int n_seen;
    const int32_t* seen = seen_run(s, s.row[b], n_seen);
    int cnt = 0;
    for (int i = lane; i < n_seen; i += 64) {
        const int32_t j = seen[i];
        if ((i == 0 || seen[i - 1] != j) && (!pool || pool_bit(pool[j >> 5], j))) ++cnt;
    }
    cnt = wave_sum_i32(cnt);
    const int kk_b = min(kk, pool_cols - cnt);
    for (int r = kk_b + lane; r < kk; r += 64) {
        const size_t at = static_cast<size_t>(b) * k + r;
        if (keys[at] < 0) scores[at] = 0.0f;
    }
}

// ------------------------------------------------------------------------------------------------
// Row normalisation (most_similar): Fn[j][c] = F[j][c] / sqrt(s_j + 1e-8f), the bits of the reference's numpy line
// feat / sqrt((feat ** 2).sum(-1) + 1e-8) on float32 factors (algo/base.py:26-28).  s_j is the float32 sum of the float32-ROUNDED
// squares of the row's d columns (never of its ld) in numpy's pairwise order: pairwise_row_sum over SquareOf (csrc/pairwise_sum.hpp,
// eight lanes per row).  `#pragma clang fp contract(off)` here as there; this toolchain's __fsqrt_rn is the native square root: the
// operators below, with contraction off, are the correctly rounded ones (HIP's default for float sqrtf and /).
// ------------------------------------------------------------------------------------------------
// F, out: [rows, ld], ld % 8 == 0; out's columns [d, ld) are written as zero.  out == F is allowed: a row's sum is complete (it feeds
// every quotient) before its first element is written, and only the row's own eight lanes touch it -- hence no __restrict__.
// grid: ceil(rows / 32) blocks of 256 threads.
__global__ __launch_bounds__(256) void topk_normalize_kernel(const float* F, int rows, int d, int ld, float* out) {
#pragma clang fp contract(off)
    const int j = blockIdx.x * 32 + (threadIdx.x >> 3), i = threadIdx.x & 7;
    if (j >= rows) return;
    const float* a = F + static_cast<size_t>(j) * ld;
    const float s = pairwise_row_sum(SquareOf{a}, d, i);
    const float norm = sqrtf(s + 1e-8f);
    float* o = out + static_cast<size_t>(j) * ld;
    for (int c = i; c < ld; c += 8) o[c] = c < d ? a[c] / norm : 0.f;
}

// ------------------------------------------------------------------------------------------------
// Ranking by squared distance ("score_func" = 1): -|p - q_j|^2 = 2 (p . q_j - s_j / 2) - |p|^2, so per query the order of the keys
// p . q_j + hb_j, hb_j = -0.5f * s_j, is the order of the distances: hb rides where the item bias Qb rides and no ranking kernel changes.
// ------------------------------------------------------------------------------------------------
// hb[j] = -0.5f * s_j, s_j the normaliser's sum above (the same bits; halving is exact).  grid: ceil(rows / 32) blocks of 256 threads.
__global__ __launch_bounds__(256) void topk_half_sqnorm_kernel(const float* __restrict__ Q, int rows, int d, int ld, float* __restrict__ hb) {
    const int j = blockIdx.x * 32 + (threadIdx.x >> 3), i = threadIdx.x & 7;
    if (j >= rows) return;
    const float s = pairwise_row_sum(SquareOf{Q + static_cast<size_t>(j) * ld}, d, i);
    if (i == 0) hb[j] = -0.5f * s;
}

// The reported score of a listed key: scores[b][r] = sum_c fl(fl(Q[key][c] - P[row(b)][c])^2) in numpy's pairwise order -- the bits of
// ((Q[key] - p) ** 2).sum(-1) on float32 arrays -- recomputed from the two rows, not backed out of the ranking key; +inf where the slot
// holds no key (-1).  row(b) = qidx ? qidx[b] : b, the indirection of topk_scores_kernel (the validation ranking's rows exist on the
// device alone).  Eight lanes per (b, r) slot of the [nq, k] result; grid: ceil(nq * k / 32) blocks of 256 threads.
__global__ __launch_bounds__(256) void topk_sqdist_kernel(const float* __restrict__ P, const int32_t* __restrict__ qidx, const float* __restrict__ Q,
                                                          int d, int ld, const int32_t* __restrict__ keys, int64_t slots, int k,
                                                          float* __restrict__ scores) {
    const int64_t at = static_cast<int64_t>(blockIdx.x) * 32 + (threadIdx.x >> 3);
    const int i = threadIdx.x & 7;
    if (at >= slots) return;   // whole eight-lane groups leave together
    const int64_t b = at / k;
    const int32_t key = keys[at];
    const float* p = P + (qidx ? static_cast<int64_t>(qidx[b]) : b) * ld;
    const float* q = Q + static_cast<int64_t>(key < 0 ? 0 : key) * ld;   // an empty slot sums row 0 and drops the sum: the eight lanes stay together
    const float dist = pairwise_row_sum(SqDiffOf{q, p}, d, i);
    if (i == 0) scores[at] = key < 0 ? __builtin_inff() : dist;
}

}  // namespace bfh
