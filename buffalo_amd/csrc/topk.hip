// Top-k selection over factor products on gfx950 -- the handle, the engine functions of csrc/topk_engine.hpp and the C ABI.
// The kernels and what they compute: csrc/topk_kernels.hpp.
#include <numeric>

#include "abi.hpp"
#include "topk_engine.hpp"
#include "topk_kernels.hpp"

namespace bfh {

constexpr int TOPK_MAX_K = 16384;
constexpr int kListCap = 2048;   // entries of the select kernels' candidate list of a row (fused path)

struct TopkModes {
    bool fast_select = true;    // 0: multi-pass radix select only (debug / comparison)
    int fused = -1;             // -1: by size (default), 0: dense path only, 1: whenever d <= 128 (tests)
    int fused_c0 = 0;           // with fused = 1: columns sampled for the thresholds (0: by rule)
    bool wave_select = true;    // 0: block-per-row selection everywhere (comparison)
    bool flt_min_rule = true;   // _core.hpp:26,115: the running list starts at FLT_MIN, so scores <= FLT_MIN are never admitted
    bool l2 = false;            // "score_func" = 1: rank by squared distance (include/buffalo_hip.h) -- hb for Qb, every score admissible, distances out
};

// The fused path's shape for a call, or `on = false`: the dense path.  C0 = sampled columns (the thresholds' source):
// the filter is expected to pass kk * q_rows / C0 columns per query, which must sit well inside the LDS list.
struct FusedPlan {
    bool on = false;
    int c0 = 0, c0_tiles = 0, n_seg = 1, tpb = 1, cap_seg = 0;
    bool sample_seg = false;
};
static FusedPlan fused_plan(const TopkModes& m, int num_cus, int nq, int q_rows, int d_pad, int kk) {
    FusedPlan fp;
    if (m.fused == 0 || d_pad > 128) return fp;   // two K-chunks accumulate through the score buffer
    const bool force = m.fused > 0;
    if (!force && (nq < 8192 || q_rows < 8192)) return fp;   // small sweeps: the dense path's item-tile parallelism matters more
    const int n_tiles = (q_rows + 31) / 32;
    int64_t need = (static_cast<int64_t>(kk) * q_rows + kListCap / 3 - 1) / (kListCap / 3);
    int c0 = force ? 32 : 2048;
    while (c0 < need) c0 <<= 1;
    if (force && m.fused_c0 > 0) c0 = m.fused_c0;   // tests: exactly this sample (too small a sample overflows the lists: the dense redo path)
    c0 = (c0 + 31) / 32 * 32;
    if (force) c0 = std::min(c0, n_tiles * 32);   // tests: any shape goes through (overflowing rows take the dense path)
    else if (c0 > q_rows / 4) return fp;
    if (c0 >= q_rows + 32) return fp;
    fp.c0 = std::min(c0, q_rows);
    fp.c0_tiles = (fp.c0 + 31) / 32;              // c0 is a multiple of 32 or the whole matrix
    fp.sample_seg = m.wave_select && fp.c0 <= 4096;   // topk_thr_wave_kernel writes the sample's own candidates ...
    const int sweep_tiles = n_tiles - (fp.sample_seg ? fp.c0_tiles : 0);   // ... and the filtered sweep starts behind the sample
    const int qblocks = (nq + 127) / 128;
    int tpb = static_cast<int>((static_cast<int64_t>(sweep_tiles) * qblocks + num_cus * 8 - 1) / (num_cus * 8));
    tpb = std::max(tpb, (sweep_tiles + 7) / 8);   // at most 8 segments per query
    fp.tpb = std::max(1, tpb);
    fp.n_seg = std::max(1, (sweep_tiles + fp.tpb - 1) / fp.tpb);
    fp.cap_seg = static_cast<int>(std::min<int64_t>(static_cast<int64_t>(fp.tpb) * 32, std::max(64, 2 * kListCap / fp.n_seg)));
    fp.on = true;
    return fp;
}

// Every size of a call, worked out once: nq queries against q_rows candidates of d columns, k slots per row.
struct TopkPlan {
    int k = 0, kk = 0;        // output width, min(k, q_rows[, pool_size])
    int p2 = 2;               // power of two >= kk: sort buffer entries
    int cand_cap = 0;         // candidate buffer of the select kernel's fast path (entries behind the sort buffer)
    int seen_cap = 0;         // seen-aware calls: training rows up to this many keys are staged in LDS (topk_kernels.hpp: SeenArgs)
    size_t ld_s = 0;          // row pitch of the dense score buffer
    int d_pad = 0, n_tiles = 0;
    FusedPlan fp;
    int batch = 0;            // queries per sweep, a multiple of 128 (or all of them)
    int redo_rows = 0;        // fused: dense rows per sweep of the rows handed back
    bool wave_list = false;   // fused: topk_list_wave_kernel selects (else list-mode topk_select_kernel for all rows)
    size_t lds_dense = 0, lds_list = 0;                 // topk_select_kernel: dense rows, list mode (seen-aware calls: + the staged seen keys)
    size_t lds_wave = 0, lds_wave_list = 0;             // topk_thr_wave_kernel (four histograms), topk_list_wave_kernel (+ 4 sort buffers)
};
// `num_cus`: of the device (sizes the tile groups of the fused sweep), 0: dense only (quickselect); `max_batch` > 0 caps the queries per
// sweep; `seen`: a seen-aware call (recommend_unseen, rank_unseen)
static TopkPlan make_plan(const TopkModes& m, int num_cus, int nq, int q_rows, int d, int k, int pool_size, int max_batch, bool seen) {
    TopkPlan pl;
    pl.k = k;
    pl.kk = std::min(q_rows, k);
    if (pool_size) pl.kk = std::min(pool_size, pl.kk);
    while (pl.p2 < pl.kk) pl.p2 <<= 1;
    pl.cand_cap = (140 * 1024 - pl.p2 * 8) / 8 >= 1024 ? 1024 : 0;   // small on purpose: LDS per block decides how many rows a CU works on at once
    pl.ld_s = (static_cast<size_t>(q_rows) + 31) / 32 * 32;
    pl.d_pad = (d + 7) / 8 * 8;
    pl.n_tiles = (q_rows + 31) / 32;
    if (num_cus) pl.fp = fused_plan(m, num_cus, nq, q_rows, pl.d_pad, pl.kk);
    const FusedPlan& fp = pl.fp;
    if (seen) pl.seen_cap = (140 * 1024 - (pl.p2 + pl.cand_cap + (fp.on ? kListCap : 0)) * 8) / 4 >= 2048 ? 2048 : 0;
    // query batch, multiple of 128 rows: dense -- score buffer <= 2 GiB; fused -- sample scores + candidate segments <= 2 GiB,
    // and room in the score buffer for 128 dense rows (the rows the fused path hands back)
    const size_t per_query = fp.on ? static_cast<size_t>(fp.c0) * 4 + static_cast<size_t>(fp.n_seg) * fp.cap_seg * 8 : pl.ld_s * 4;
    pl.batch = static_cast<int>(std::min<size_t>(nq, std::max<size_t>(128, ((size_t(1) << 31) / per_query) / 128 * 128)));
    if (max_batch > 0) pl.batch = std::min(pl.batch, max_batch);
    pl.redo_rows = fp.on ? static_cast<int>(std::max<size_t>(128, std::min<size_t>(pl.batch, (size_t(1) << 28) / pl.ld_s) / 128 * 128)) : 0;
    pl.wave_list = m.wave_select && pl.p2 <= 1024;
    pl.lds_dense = static_cast<size_t>(pl.p2 + pl.cand_cap) * 8 + static_cast<size_t>(pl.seen_cap) * 4;
    pl.lds_list = pl.lds_dense + static_cast<size_t>(kListCap) * 8;
    pl.lds_wave = static_cast<size_t>(4) * kWaveHistBins * 4;
    pl.lds_wave_list = pl.lds_wave + static_cast<size_t>(4) * std::min(pl.p2, 1024) * 8;
    return pl;
}

template <typename K>
static void allow_dynamic_lds(K kernel, size_t bytes) {
    BFH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(bytes)));
}

class TopkHandle : public HandleBase {
 public:
    ~TopkHandle() override {
        if (stream) (void)hipStreamDestroy(stream);
    }
    void ensure() {
        BFH_HIP(hipSetDevice(device));
        if (!stream) {
            BFH_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
            hipDeviceProp_t prop;
            BFH_HIP(hipGetDeviceProperties(&prop, device));
            num_cus_ = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        }
    }

    // what the steps of one dot_topn / recommend_unseen / rank_unseen call share: factor matrices in HBM, [rows, ld]
    struct Call {
        TopkPlan pl;
        const float* dP;
        const int32_t* qidx;      // nullable: query b is row qidx[q0 + b] of dP (else row q0 + b)
        int q_rows, ld;
        SelectArgs base;          // adm (the pool), out (but q0; scores nullable), seen (seen.row set: a seen-aware call), p2 / cand_cap
        const int32_t* d_ids;     // device: the id of query b -- the caller's index (self exclusion) or user (seen.row); uploaded from the
                                  // caller's host array, or the validation ranking's device rows
        bool same;                // P == Q: a query's own column is excluded
    };
    SelectArgs select_base(const TopkPlan& pl, const float* dQb, const uint32_t* d_pool, bool rule_flt_min, int32_t* keys, float* scores) const {
        SelectArgs a{};
        a.adm.Qb = dQb; a.adm.pool = d_pool; a.adm.rule_flt_min = rule_flt_min ? 1 : 0;
        a.out.keys = keys; a.out.scores = scores; a.out.k = pl.k; a.out.kk = pl.kk;
        a.p2 = pl.p2; a.cand_cap = m_.fast_select ? pl.cand_cap : 0;
        return a;
    }

    // dense scores of `nb` queries (rows qidx ? qidx[q0 + b] : q0 + b of dP) against the first `cols` candidates -> S_ [nb, ld_s]
    void launch_scores(const float* dP, const int32_t* qidx, int q0, int nb, int cols, int ld, int d_pad, size_t ld_s, size_t tiles_all) {
        const int n_tiles = (cols + 31) / 32;
        const int qblocks = (nb + 127) / 128;
        int tpb = static_cast<int>((static_cast<int64_t>(n_tiles) * qblocks + num_cus_ * 8 - 1) / (num_cus_ * 8));
        if (tpb < 1) tpb = 1;
        const dim3 grid((n_tiles + tpb - 1) / tpb, qblocks);
        for (int kc = 0; kc < d_pad; kc += 128) {
            const int W = std::min(128, d_pad - kc);
            const float4* qp = Qp_.get() + static_cast<size_t>(kc / 128) * tiles_all * 16 * 64;
            hipLaunchKernelGGL((W == 128 ? topk_scores_kernel<true, false> : topk_scores_kernel<false, false>), grid, dim3(256), 0, stream, dP, qidx, q0,
                               nb, qp, cols, ld, kc, W, S_.get(), ld_s, tpb, kc > 0 ? 1 : 0, FilterArgs{});
            BFH_HIP(hipGetLastError());
        }
    }
    void launch_select(const SelectArgs& a, int rows, size_t lds) {   // a.seen.row set: the seen-aware instance
        hipLaunchKernelGGL((a.seen.row ? topk_select_kernel<true> : topk_select_kernel<false>), dim3(rows), dim3(256), lds, stream, a);
        BFH_HIP(hipGetLastError());
    }

    // ---- the dense step: scores of a batch against every candidate into S_ (kernel_ms), then one block per row selects (aux_ms) ----
    void select_rows(const SelectArgs& a, int rows, size_t lds) {   // the select half (quickselect: the scores are the caller's)
        t_aux_.timed(stream, [&] { launch_select(a, rows, lds); });
    }
    void dense_step(const Call& c, const int32_t* qidx, int q0, int nb, SelectArgs a, size_t lds) {
        t_main_.timed(stream, [&] { launch_scores(c.dP, qidx, q0, nb, c.q_rows, c.ld, c.pl.d_pad, c.pl.ld_s, c.pl.n_tiles); });
        a.dense = DenseArgs{S_.get(), c.pl.ld_s, c.q_rows};
        a.out.q0 = q0;
        select_rows(a, nb, lds);   // the scores kernel of the next batch reuses S_: the stream orders it after this select
    }

    const int32_t* upload_queries(const int32_t* indexes, int nq) {
        grow(d_idx_, nq);
        BFH_HIP(hipMemcpyAsync(d_idx_.get(), indexes, sizeof(int32_t) * nq, hipMemcpyHostToDevice, stream));
        stats.h2d_bytes += 4.0 * nq;
        return d_idx_.get();
    }
    // the pool as a bitmap over the columns (null: no pool); pool_cols_ = the columns it admits
    const uint32_t* upload_pool(const int32_t* pool, int pool_size, int q_rows) {
        pool_cols_ = q_rows;
        if (!pool_size) return nullptr;
        const size_t words = (static_cast<size_t>(q_rows) + 31) / 32;
        std::vector<uint32_t> bm(words, 0u);
        for (int i = 0; i < pool_size; ++i) {
            const int32_t j = pool[i];
            if (j >= 0 && j < q_rows) bm[j >> 5] |= 1u << (j & 31);   // ids outside the matrix can never match a candidate
        }
        pool_cols_ = 0;
        for (uint32_t w : bm) pool_cols_ += __builtin_popcount(w);
        grow(d_pool_, words);
        BFH_HIP(hipMemcpyAsync(d_pool_.get(), bm.data(), words * 4, hipMemcpyHostToDevice, stream));
        BFH_HIP(hipStreamSynchronize(stream));   // bm is a local
        stats.h2d_bytes += 4.0 * words;
        return d_pool_.get();
    }
    // `own_out`: the rows go to d_keys_ / d_scores_ (else to the caller's device list; the fused path's block route still reads its
    // thresholds from d_scores_); `seen`: the seen-aware kernel instances run
    void ensure_buffers(const TopkPlan& pl, int nq, bool own_out, bool seen) {
        const FusedPlan& fp = pl.fp;
        if (own_out) grow(d_keys_, static_cast<size_t>(nq) * pl.k);
        if (own_out || fp.on) grow(d_scores_, static_cast<size_t>(nq) * pl.k);
        grow(S_, fp.on ? std::max(static_cast<size_t>(pl.batch) * fp.c0, static_cast<size_t>(pl.redo_rows) * pl.ld_s) : static_cast<size_t>(pl.batch) * pl.ld_s);
        const size_t lds_select = fp.on ? pl.lds_list : pl.lds_dense;
        if (seen) allow_dynamic_lds(topk_select_kernel<true>, lds_select);
        else allow_dynamic_lds(topk_select_kernel<false>, lds_select);
        if (!fp.on) return;
        if (m_.wave_select && seen) {
            allow_dynamic_lds(topk_thr_wave_kernel<true>, pl.lds_wave);
            allow_dynamic_lds(topk_list_wave_kernel<true>, pl.lds_wave_list);
        } else if (m_.wave_select) {
            allow_dynamic_lds(topk_thr_wave_kernel<false>, pl.lds_wave);
            allow_dynamic_lds(topk_list_wave_kernel<false>, pl.lds_wave_list);
        }
        const size_t batch = static_cast<size_t>(pl.batch);
        grow(thr_, batch);
        grow(cand_, batch * fp.n_seg * fp.cap_seg);
        grow(cnt_, batch * fp.n_seg);
        grow(redo_, batch + 1);
        grow(general_, batch + 1);
        grow(s0_cand_, batch * kSampleCap);
        grow(s0_cnt_, batch);
    }
    // candidate matrix in operand order, one slab per K-chunk
    void pack_candidates(const float* dQ, int q_rows, int ld, int d_pad) {
        const int n_tiles = (q_rows + 31) / 32;
        const int n_chunks = (d_pad + 127) / 128;
        const size_t per = static_cast<size_t>(n_tiles) * 16 * 64;
        grow(Qp_, per * n_chunks);
        t_aux_.timed(stream, [&] {
            for (int c = 0; c < n_chunks; ++c) {
                const int W = std::min(128, d_pad - c * 128);
                hipLaunchKernelGGL(topk_pack_kernel, dim3(static_cast<unsigned>((per + 255) / 256)), dim3(256), 0, stream, dQ, q_rows, ld, c * 128, W,
                                   Qp_.get() + per * c, n_tiles);
                BFH_HIP(hipGetLastError());
            }
        });
    }

    // fused (1): thresholds from the dense scores of the first c0 columns -> thr_; redo_ / general_ counters cleared.  The wave kernel
    // also writes the sample's own candidates (s0_*), and the sweep then starts behind the sample; the block-level route (samples
    // beyond 4096 columns, wave_select = 0) only yields thresholds, and the sweep covers every column
    void sample_thresholds(const Call& c, int q0, int nb) {
        const TopkPlan& pl = c.pl;
        const FusedPlan& fp = pl.fp;
        t_main_.timed(stream, [&] { launch_scores(c.dP, c.qidx, q0, nb, fp.c0, c.ld, pl.d_pad, static_cast<size_t>(fp.c0), pl.n_tiles); });
        SelectArgs a = c.base;
        a.dense = DenseArgs{S_.get(), static_cast<size_t>(fp.c0), fp.c0};
        a.out.q0 = q0;
        t_aux_.timed(stream, [&] {
            if (fp.sample_seg) {
                a.work.thr = thr_.get();
                a.list.s0_cand = s0_cand_.get(); a.list.s0_cnt = s0_cnt_.get(); a.list.s0_cap = kSampleCap;
                hipLaunchKernelGGL((a.seen.row ? topk_thr_wave_kernel<true> : topk_thr_wave_kernel<false>), dim3((nb + 3) / 4), dim3(256), pl.lds_wave,
                                   stream, a, nb);
            } else {
                launch_select(a, nb, pl.lds_dense);
                hipLaunchKernelGGL(topk_thr_kernel, dim3((nb + 255) / 256), dim3(256), 0, stream, a.out.keys, a.out.scores, q0, nb, pl.k, pl.kk,
                                   a.adm.rule_flt_min, thr_.get());
            }
            BFH_HIP(hipGetLastError());
            BFH_HIP(hipMemsetAsync(redo_.get(), 0, sizeof(int), stream));
            BFH_HIP(hipMemsetAsync(general_.get(), 0, sizeof(int), stream));
        });
    }
    // fused (2): the sweep whose epilogue keeps the columns at or above the row's threshold -> cand_ / cnt_
    void filtered_sweep(const Call& c, int q0, int nb) {
        const TopkPlan& pl = c.pl;
        const FusedPlan& fp = pl.fp;
        const FilterArgs f{thr_.get(), c.base.adm.Qb, c.base.adm.pool, cand_.get(), cnt_.get(), fp.cap_seg, fp.sample_seg ? fp.c0_tiles : 0};
        const dim3 grid(fp.n_seg, (nb + 127) / 128);
        t_main_.timed(stream, [&] {
            hipLaunchKernelGGL((pl.d_pad == 128 ? topk_scores_kernel<true, true> : topk_scores_kernel<false, true>), grid, dim3(256), 0, stream, c.dP,
                               c.qidx, q0, nb, Qp_.get(), c.q_rows, c.ld, 0, pl.d_pad, static_cast<float*>(nullptr), size_t(0), fp.tpb, 0, f);
            BFH_HIP(hipGetLastError());
        });
    }
    // fused (3): selection over the candidate lists, one wave or one block per row, then the rows with ties at the k-th place
    // (block-level list selection).  Returns the number of rows handed back to the dense path (redo_[1..]).
    int select_lists(const Call& c, int q0, int nb) {
        const TopkPlan& pl = c.pl;
        const FusedPlan& fp = pl.fp;
        SelectArgs a = c.base;
        a.out.q0 = q0;
        a.list = ListArgs{cand_.get(), cnt_.get(), fp.n_seg, fp.cap_seg, kListCap, nullptr, nullptr, 0};
        if (fp.sample_seg) { a.list.s0_cand = s0_cand_.get(); a.list.s0_cnt = s0_cnt_.get(); a.list.s0_cap = kSampleCap; }
        a.work.redo = redo_.get(); a.work.general = general_.get();
        if (pl.wave_list)
            t_aux_.timed(stream, [&] {
                hipLaunchKernelGGL((a.seen.row ? topk_list_wave_kernel<true> : topk_list_wave_kernel<false>), dim3((nb + 3) / 4), dim3(256),
                                   pl.lds_wave_list, stream, a, nb);
                BFH_HIP(hipGetLastError());
            });
        else select_rows(a, nb, pl.lds_list);
        int n_redo = 0, n_general = 0;
        BFH_HIP(hipMemcpyAsync(&n_redo, redo_.get(), sizeof(int), hipMemcpyDeviceToHost, stream));
        BFH_HIP(hipMemcpyAsync(&n_general, general_.get(), sizeof(int), hipMemcpyDeviceToHost, stream));
        BFH_HIP(hipStreamSynchronize(stream));
        stats.merges += n_redo;         // top-k: rows the fused path handed back to the dense path
        stats.exchanges += n_general;   // top-k: rows with ties at the k-th place (block-level list selection)
        if (n_general > 0) {
            a.work.row_list = general_.get() + 1;
            select_rows(a, n_general, pl.lds_list);
        }
        return n_redo;
    }
    // fused (4): the rows whose candidates did not fit (ties at the threshold, all-inadmissible rows, tiny pools, lists full of seen
    // columns) take the dense step, each with its own query's id: the self exclusion's index, the seen-aware step's user
    void redo_dense(const Call& c, int q0, int n_redo) {
        std::vector<int32_t> rows(static_cast<size_t>(n_redo));
        BFH_HIP(hipMemcpy(rows.data(), redo_.get() + 1, sizeof(int32_t) * n_redo, hipMemcpyDeviceToHost));
        std::sort(rows.begin(), rows.end());
        grow(redo_side_, rows.size() * 3);   // row of dP | query id | output row (topk_redo_side_kernel)
        BFH_HIP(hipMemcpy(redo_side_.get() + 2 * static_cast<size_t>(n_redo), rows.data(), rows.size() * 4, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(topk_redo_side_kernel, dim3((n_redo + 255) / 256), dim3(256), 0, stream, redo_side_.get(), n_redo, q0, c.qidx, c.d_ids);
        BFH_HIP(hipGetLastError());
        for (int r0 = 0; r0 < n_redo; r0 += c.pl.redo_rows) {
            SelectArgs r = c.base;
            r.adm.self_idx = c.same ? redo_side_.get() + n_redo + r0 : nullptr;
            if (c.base.seen.row) r.seen.row = redo_side_.get() + n_redo + r0;
            r.out.out_row = redo_side_.get() + 2 * static_cast<size_t>(n_redo) + r0;
            dense_step(c, redo_side_.get() + r0, 0, std::min(c.pl.redo_rows, n_redo - r0), r, c.pl.lds_dense);
        }
    }

    // core: factor matrices in HBM, [rows, ld], ld % 8 == 0, columns [d, ld) zero
    void run_device(const int32_t* indexes, int nq, const float* dP, bool gather, const float* dQ, int q_rows, int d, int ld, const float* dQb,
                    bool same, int32_t* out_keys, float* out_scores, const int32_t* pool, int pool_size, int k) {
        BFH_REQUIRE(k > 0 && k <= TOPK_MAX_K, "k must be in [1, 16384]");
        BFH_REQUIRE(ld % 8 == 0 && d <= ld && d > 0, "factor matrices need a leading dimension that is a multiple of 8 and >= d");
        BFH_REQUIRE(nq >= 0 && q_rows > 0, "empty candidate matrix");
        if (nq == 0) return;
        ensure();
        const int32_t* d_idx = upload_queries(indexes, nq);
        const uint32_t* d_pool = upload_pool(pool, pool_size, q_rows);
        const TopkPlan pl = make_plan(m_, num_cus_, nq, q_rows, d, k, pool_size, 0, false);
        ensure_buffers(pl, nq, true, false);
        pack_candidates(dQ, q_rows, ld, pl.d_pad);
        dQb = half_norms(dQ, q_rows, d, ld, dQb);
        Call c{pl, dP, gather ? d_idx : nullptr, q_rows, ld, select_base(pl, dQb, d_pool, admit_rule(), d_keys_.get(), d_scores_.get()), d_idx, same};
        c.base.adm.self_idx = same ? d_idx : nullptr;
        run_batches(c, nq);
        rescore_distances(c, dQ, d, nq);
        download_rows(out_keys, out_scores, nq, k);
        finish_call(nq, q_rows);
    }
    // every batch of a call: the dense step, or the four steps of the fused path
    void run_batches(const Call& c, int nq) {
        const TopkPlan& pl = c.pl;
        for (int q0 = 0; q0 < nq; q0 += pl.batch) {
            const int nb = std::min(pl.batch, nq - q0);
            if (!pl.fp.on) {
                dense_step(c, c.qidx, q0, nb, c.base, pl.lds_dense);
                continue;
            }
            sample_thresholds(c, q0, nb);
            filtered_sweep(c, q0, nb);
            const int n_redo = select_lists(c, q0, nb);
            if (n_redo > 0) redo_dense(c, q0, n_redo);
        }
    }
    // ---- "score_func" = 1: the two steps around the unchanged ranking (topk_kernels.hpp: ranking by squared distance) ----
    void refuse_bias(bool has_bias) const {
        if (m_.l2 && has_bias) throw Error(BFH_ERR_INVALID, "score_func = l2: the L2 score has no item bias (qb_rows must be 0)");
    }
    bool admit_rule() const { return m_.flt_min_rule && !m_.l2; }   // a distance has no FLT_MIN start: every score is admissible under L2
    // the bias of a call: the caller's Qb, or under L2 hb_ [q_rows] = -|q_j|^2 / 2, made once per call from dQ over its d columns (aux_ms)
    const float* half_norms(const float* dQ, int q_rows, int d, int ld, const float* dQb) {
        if (!m_.l2) return dQb;
        refuse_bias(dQb != nullptr);
        grow(hb_, static_cast<size_t>(q_rows));
        t_aux_.timed(stream, [&] {
            hipLaunchKernelGGL(topk_half_sqnorm_kernel, dim3((q_rows + 31) / 32), dim3(256), 0, stream, dQ, q_rows, d, ld, hb_.get());
            BFH_HIP(hipGetLastError());
        });
        return hb_.get();
    }
    // under L2 the listed scores are the squared distances of the listed keys, recomputed from the rows (key -1: +inf); aux_ms
    void rescore_distances(const Call& c, const float* dQ, int d, int nq) {
        if (!m_.l2 || !c.base.out.scores) return;
        const int64_t slots = static_cast<int64_t>(nq) * c.pl.k;
        t_aux_.timed(stream, [&] {
            hipLaunchKernelGGL(topk_sqdist_kernel, dim3(static_cast<unsigned>((slots + 31) / 32)), dim3(256), 0, stream, c.dP, c.qidx, dQ, d, c.ld,
                               c.base.out.keys, slots, c.pl.k, c.base.out.scores);
            BFH_HIP(hipGetLastError());
        });
    }
    void download_rows(int32_t* out_keys, float* out_scores, int nq, int k) {
        BFH_HIP(hipMemcpyAsync(out_keys, d_keys_.get(), sizeof(int32_t) * nq * k, hipMemcpyDeviceToHost, stream));
        BFH_HIP(hipMemcpyAsync(out_scores, d_scores_.get(), sizeof(float) * nq * k, hipMemcpyDeviceToHost, stream));
        stats.d2h_bytes += 8.0 * nq * k;
    }
    void finish_call(int nq, int q_rows) {
        BFH_HIP(hipStreamSynchronize(stream));
        stats.samples += static_cast<int64_t>(nq) * q_rows;
        stats.kernel_ms += t_main_.drain();
        stats.aux_ms += t_aux_.drain();
    }

    // ---- recommend_unseen: dot_topn whose row b leaves out the training row of user users[b] ----
    void set_seen(int num_users, int num_items, const int64_t* seen_indptr, const int32_t* seen_keys, int64_t nnz) {
        validate_seen_csr("set_seen", num_users, num_items, seen_indptr, seen_keys, nnz);
        ensure();
        seen_users_ = 0;   // unbound while the arrays are replaced
        seen_indptr_.resize(num_users);
        seen_keys_.resize(std::max<int64_t>(nnz, 1));
        BFH_HIP(hipMemcpyAsync(seen_indptr_.get(), seen_indptr, sizeof(int64_t) * num_users, hipMemcpyHostToDevice, stream));
        if (nnz) BFH_HIP(hipMemcpyAsync(seen_keys_.get(), seen_keys, sizeof(int32_t) * nnz, hipMemcpyHostToDevice, stream));
        BFH_HIP(hipStreamSynchronize(stream));
        stats.h2d_bytes += 8.0 * num_users + 4.0 * nnz;
        seen_users_ = num_users; seen_items_ = num_items;
    }
    void check_unseen(const int32_t* users, int nq, int p_rows, int q_rows, int k) const {
        BFH_REQUIRE(seen_users_ > 0, "recommend_unseen: set_seen has not been called");
        BFH_REQUIRE(p_rows == seen_users_, "recommend_unseen: P must have one row per user of set_seen");
        BFH_REQUIRE(q_rows == seen_items_, "recommend_unseen: Q must have one row per item of set_seen");
        BFH_REQUIRE(k > 0 && k <= TOPK_MAX_K, "k must be in [1, 16384]");
        BFH_REQUIRE(nq >= 0 && (nq == 0 || users), "recommend_unseen: null or negative number of users");
        for (int i = 0; i < nq; ++i)
            if (users[i] < 0 || users[i] >= seen_users_) throw Error(BFH_ERR_INVALID, "recommend_unseen: user outside [0, num_users) at position " + std::to_string(i));
    }
    // core, as run_device: query b is row users[b] of dP (`gather`) or row b
    void recommend_unseen_device(const int32_t* users, int nq, const float* dP, bool gather, const float* dQ, int q_rows, int d, int ld,
                                 const float* dQb, int32_t* out_keys, float* out_scores, const int32_t* pool, int pool_size, int k) {
        BFH_REQUIRE(ld % 8 == 0 && d <= ld && d > 0, "factor matrices need a leading dimension that is a multiple of 8 and >= d");
        if (nq == 0) return;
        ensure();
        const int32_t* d_users = upload_queries(users, nq);
        const uint32_t* d_pool = upload_pool(pool, pool_size, q_rows);
        const TopkPlan pl = make_plan(m_, num_cus_, nq, q_rows, d, k, pool_size, 0, true);
        ensure_buffers(pl, nq, true, true);
        pack_candidates(dQ, q_rows, ld, pl.d_pad);
        dQb = half_norms(dQ, q_rows, d, ld, dQb);
        Call c{pl, dP, gather ? d_users : nullptr, q_rows, ld, select_base(pl, dQb, d_pool, admit_rule(), d_keys_.get(), d_scores_.get()), d_users, false};
        c.base.seen = SeenArgs{seen_indptr_.get(), seen_keys_.get(), d_users, pl.seen_cap};
        run_batches(c, nq);
        if (!m_.l2) t_aux_.timed(stream, [&] {   // the per-user pool sizes decide where the (-1, FLT_MIN) padding ends (L2: every empty slot reads +inf)
            hipLaunchKernelGGL(topk_unseen_padding_kernel, dim3((nq + 3) / 4), dim3(256), 0, stream, c.base.seen, d_pool, pool_cols_, nq, pl.k, pl.kk,
                               d_keys_.get(), d_scores_.get());
            BFH_HIP(hipGetLastError());
        });
        rescore_distances(c, dQ, d, nq);
        download_rows(out_keys, out_scores, nq, k);
        finish_call(nq, q_rows);
    }

    // The validation ranking (csrc/eval.hip; evaluate/base.py:80-89 with filter_seen_items folded into the selection): for query b the
    // min(k, q_rows) best columns that are NOT in the training row of user d_rows[b], listed by (score desc, index desc), the rest of the
    // k slots -1.  Every score is admissible (no FLT_MIN rule).  Everything stays on the device: d_rows [nq] and d_out_keys [nq, k] are
    // device arrays.  The same steps as dot_topn, planned by the same rule ("fused": the seen-aware instances of the fused path's kernels,
    // d <= 128); `max_batch` > 0 caps the queries per sweep (rows are independent: the lists do not depend on it).
    void rank_unseen(const int32_t* d_rows, int nq, const float* dP, const float* dQ, int q_rows, int d, int ld, const float* dQb,
                     const int64_t* d_seen_indptr, const int32_t* d_seen_keys, int k, int32_t* d_out_keys, int max_batch) {
        BFH_REQUIRE(k > 0 && k <= TOPK_MAX_K, "topk must be in [1, 16384]");
        BFH_REQUIRE(ld % 8 == 0 && d <= ld && d > 0, "factor matrices need a leading dimension that is a multiple of 8 and >= d");
        BFH_REQUIRE(nq >= 0 && q_rows > 0, "empty candidate matrix");
        if (nq == 0) return;
        ensure();
        const TopkPlan pl = make_plan(m_, num_cus_, nq, q_rows, d, k, 0, max_batch, true);
        ensure_buffers(pl, nq, false, true);
        pack_candidates(dQ, q_rows, ld, pl.d_pad);
        dQb = half_norms(dQ, q_rows, d, ld, dQb);
        // no scores leave (so there is nothing to rescore under L2); the fused path's block route reads its thresholds from the sample's
        Call c{pl, dP, d_rows, q_rows, ld, select_base(pl, dQb, nullptr, false, d_out_keys, pl.fp.on ? d_scores_.get() : nullptr), d_rows, false};
        c.base.seen = SeenArgs{d_seen_indptr, d_seen_keys, d_rows, pl.seen_cap};
        run_batches(c, nq);
        finish_call(nq, q_rows);
    }

    // host matrices: upload the query rows (gathered) and the candidate matrix, zero-padded to ld = d_pad
    struct HostFactors {
        const float *dP, *dQ, *dQb;
        bool whole;   // dP is all of P: the kernel gathers by index (else row b of dP is query b)
        int d, ld;
    };
    HostFactors upload_host(const int32_t* indexes, int nq, const float* P, int p_rows, int p_cols, const float* Q, int q_rows, int q_cols,
                            const float* Qb, int qb_rows) {
        BFH_REQUIRE(p_cols == q_cols, "P and Q must have the same number of columns");
        BFH_REQUIRE(qb_rows == 0 || qb_rows == q_rows, "Qb must have one row per row of Q");
        ensure();
        const int d = p_cols, ld = (d + 7) / 8 * 8;
        for (int i = 0; i < nq; ++i) BFH_REQUIRE(indexes[i] >= 0 && indexes[i] < p_rows, "query index outside P");
        // query rows: when most of P is asked for and needs no padding, P goes up as it is and the kernel gathers by
        // index; otherwise the rows are gathered (and zero-padded to ld) on the host first
        const bool whole = ld == d && static_cast<int64_t>(nq) * 2 >= p_rows;
        std::vector<float> stage;
        if (whole) {
            grow(hP_, static_cast<size_t>(p_rows) * ld);
            BFH_HIP(hipMemcpyAsync(hP_.get(), P, static_cast<size_t>(p_rows) * d * 4, hipMemcpyHostToDevice, stream));
        } else {
            stage.assign(static_cast<size_t>(nq) * ld, 0.f);
            for (int i = 0; i < nq; ++i)
                std::memcpy(&stage[static_cast<size_t>(i) * ld], P + static_cast<size_t>(indexes[i]) * p_cols, sizeof(float) * d);
            grow(hP_, stage.size());
            BFH_HIP(hipMemcpyAsync(hP_.get(), stage.data(), stage.size() * 4, hipMemcpyHostToDevice, stream));
        }
        upload_padded(hQ_, Q, q_rows, d, ld, stream);
        const float* dQb = nullptr;
        if (qb_rows) {
            grow(hQb_, static_cast<size_t>(q_rows));
            BFH_HIP(hipMemcpyAsync(hQb_.get(), Qb, static_cast<size_t>(q_rows) * 4, hipMemcpyHostToDevice, stream));
            dQb = hQb_.get();
        }
        BFH_HIP(hipStreamSynchronize(stream));   // `stage` is a local
        stats.h2d_bytes += 4.0 * ((whole ? static_cast<double>(p_rows) * d : static_cast<double>(stage.size())) + static_cast<double>(q_rows) * d + (qb_rows ? q_rows : 0));
        return HostFactors{hP_.get(), hQ_.get(), dQb, whole, d, ld};
    }
    void run_host(const int32_t* indexes, int nq, const float* P, int p_rows, int p_cols, const float* Q, int q_rows, int q_cols, const float* Qb,
                  int qb_rows, int32_t* out_keys, float* out_scores, const int32_t* pool, int pool_size, int k) {
        refuse_bias(qb_rows != 0);
        if (nq == 0) {
            BFH_REQUIRE(p_cols == q_cols, "P and Q must have the same number of columns");
            BFH_REQUIRE(qb_rows == 0 || qb_rows == q_rows, "Qb must have one row per row of Q");
            return;
        }
        const HostFactors f = upload_host(indexes, nq, P, p_rows, p_cols, Q, q_rows, q_cols, Qb, qb_rows);
        // host-gathered: row b of hP_ is query b (the self-exclusion still needs the original ids, which run_device uploads)
        run_device(indexes, nq, f.dP, f.whole, f.dQ, q_rows, f.d, f.ld, f.dQb, P == Q, out_keys, out_scores, pool, pool_size, k);
    }
    void recommend_unseen_host(const int32_t* users, int nq, const float* P, int p_rows, int p_cols, const float* Q, int q_rows, int q_cols,
                               const float* Qb, int qb_rows, int32_t* out_keys, float* out_scores, const int32_t* pool, int pool_size, int k) {
        check_unseen(users, nq, p_rows, q_rows, k);
        refuse_bias(qb_rows != 0);
        BFH_REQUIRE(P && Q && p_cols > 0, "null or empty factor matrix");
        if (nq == 0) return;
        const HostFactors f = upload_host(users, nq, P, p_rows, p_cols, Q, q_rows, q_cols, Qb, qb_rows);
        recommend_unseen_device(users, nq, f.dP, f.whole, f.dQ, q_rows, f.d, f.ld, f.dQb, out_keys, out_scores, pool, pool_size, k);
    }

    // ---- most_similar: dot_topn over Fn_, the row-normalised copy of ONE factor matrix (topk_normalize_kernel); the caller's is not written.
    // Under L2 the candidates are the rows as given: the host forms stage F in Fn_ without normalising it, the device form ranks dF where it is ----
    void launch_normalize(const float* dF, int rows, int d, int ld, float* dOut) {   // aux_ms
        t_aux_.timed(stream, [&] {
            hipLaunchKernelGGL(topk_normalize_kernel, dim3((rows + 31) / 32), dim3(256), 0, stream, dF, rows, d, ld, dOut);
            BFH_HIP(hipGetLastError());
        });
    }
    static void check_matrix(const char* what, const void* F, int rows, int d, int ld) {
        if (rows < 1 || d < 1) throw Error(BFH_ERR_INVALID, std::string(what) + ": the factor matrix needs at least one row and one column");
        if (!F) throw Error(BFH_ERR_INVALID, std::string(what) + ": null factor matrix");
        if (ld % 8 != 0 || d > ld) throw Error(BFH_ERR_INVALID, std::string(what) + ": factor matrices need a leading dimension that is a multiple of 8 and >= d");
        if (d > (1 << 24)) throw Error(BFH_ERR_INVALID, std::string(what) + ": more than 2^24 columns");   // topk_normalize_kernel: kPairwiseDepth halvings
    }
    // everything a most_similar call can refuse, before anything is uploaded or launched
    static void check_similar(const int32_t* indexes, int nq, const void* F, int rows, int d, int ld, const int32_t* out_keys, const float* out_scores,
                              const int32_t* pool, int pool_size, int k) {
        check_matrix("most_similar", F, rows, d, ld);
        BFH_REQUIRE(k > 0 && k <= TOPK_MAX_K, "k must be in [1, 16384]");
        BFH_REQUIRE(nq >= 0 && pool_size >= 0, "most_similar: negative number of queries or pool ids");
        BFH_REQUIRE(nq == 0 || (out_keys && out_scores), "most_similar: null output array");
        BFH_REQUIRE(pool_size == 0 || pool, "most_similar: null pool");
        if (indexes)   // null: the queries are vectors
            for (int i = 0; i < nq; ++i)
                if (indexes[i] < 0 || indexes[i] >= rows) throw Error(BFH_ERR_INVALID, "most_similar: index outside [0, rows) at position " + std::to_string(i));
        for (int i = 0; i < pool_size; ++i)
            if (pool[i] < 0 || pool[i] >= rows) throw Error(BFH_ERR_INVALID, "most_similar: pool id outside [0, rows) at position " + std::to_string(i));
    }
    void normalize_device(const float* dF, int rows, int d, int ld, float* dOut) {
        check_matrix("normalize", dF, rows, d, ld);
        BFH_REQUIRE(dOut, "normalize: null output matrix");
        ensure();
        launch_normalize(dF, rows, d, ld, dOut);
        BFH_HIP(hipStreamSynchronize(stream));
        stats.aux_ms += t_aux_.drain();
    }
    // the host matrix F [rows, d] -> Fn_ [rows, ld], normalised in place (`as_given`: left as it is)
    void normalize_upload(const float* F, int rows, int d, int ld, bool as_given = false) {
        ensure();
        upload_padded(Fn_, F, rows, d, ld, stream);
        stats.h2d_bytes += 4.0 * rows * d;
        if (!as_given) launch_normalize(Fn_.get(), rows, d, ld, Fn_.get());
    }
    void normalize_host(const float* F, int rows, int cols, float* out) {
        const int ld = (cols + 7) / 8 * 8;
        check_matrix("normalize", F, rows, cols, ld);
        BFH_REQUIRE(out, "normalize: null output matrix");
        normalize_upload(F, rows, cols, ld);
        stats.d2h_bytes += rows_to_host(out, cols, Fn_.get(), ld, 0, rows, stream);
        BFH_HIP(hipStreamSynchronize(stream));
        stats.aux_ms += t_aux_.drain();
    }
    // row b = the dot_topn row of indexes[b] with P = Q = dFn (self-excluded)
    void rank_similar(const int32_t* indexes, int nq, const float* dFn, int rows, int d, int ld, int32_t* out_keys, float* out_scores,
                      const int32_t* pool, int pool_size, int k) {
        run_device(indexes, nq, dFn, true, dFn, rows, d, ld, nullptr, true, out_keys, out_scores, pool, pool_size, k);
    }
    void most_similar_host(const int32_t* indexes, int nq, const float* F, int rows, int cols, int32_t* out_keys, float* out_scores,
                           const int32_t* pool, int pool_size, int k) {
        const int ld = (cols + 7) / 8 * 8;
        BFH_REQUIRE(nq == 0 || indexes, "most_similar: null indexes");
        check_similar(indexes, nq, F, rows, cols, ld, out_keys, out_scores, pool, pool_size, k);
        if (nq == 0) return;
        normalize_upload(F, rows, cols, ld, m_.l2);
        rank_similar(indexes, nq, Fn_.get(), rows, cols, ld, out_keys, out_scores, pool, pool_size, k);
    }
    void most_similar_device(const int32_t* indexes, int nq, const float* dF, int rows, int d, int ld, int32_t* out_keys, float* out_scores,
                             const int32_t* pool, int pool_size, int k) {
        BFH_REQUIRE(nq == 0 || indexes, "most_similar: null indexes");
        check_similar(indexes, nq, dF, rows, d, ld, out_keys, out_scores, pool, pool_size, k);
        if (nq == 0) return;
        ensure();
        if (m_.l2) return rank_similar(indexes, nq, dF, rows, d, ld, out_keys, out_scores, pool, pool_size, k);
        grow(Fn_, static_cast<size_t>(rows) * ld);
        launch_normalize(dF, rows, d, ld, Fn_.get());
        rank_similar(indexes, nq, Fn_.get(), rows, d, ld, out_keys, out_scores, pool, pool_size, k);
    }
    // queries given as vectors V [nq, cols], scored as they are against Fn_: the dot_topn row of query b with P = V, Q = Fn_ (no self-exclusion)
    void most_similar_vectors(const float* V, int nq, const float* F, int rows, int cols, int32_t* out_keys, float* out_scores, const int32_t* pool,
                              int pool_size, int k) {
        const int ld = (cols + 7) / 8 * 8;
        BFH_REQUIRE(nq == 0 || V, "most_similar: null query vectors");
        check_similar(nullptr, nq, F, rows, cols, ld, out_keys, out_scores, pool, pool_size, k);
        if (nq == 0) return;
        normalize_upload(F, rows, cols, ld, m_.l2);
        upload_padded(hP_, V, nq, cols, ld, stream);
        stats.h2d_bytes += 4.0 * nq * cols;
        std::vector<int32_t> ids(static_cast<size_t>(nq));
        std::iota(ids.begin(), ids.end(), 0);
        run_device(ids.data(), nq, hP_.get(), false, Fn_.get(), rows, cols, ld, nullptr, false, out_keys, out_scores, pool, pool_size, k);
    }

    void quickselect(const float* scores, int rows, int cols, int32_t* result, int k) {
        BFH_REQUIRE(rows >= 0 && cols > 0, "empty score matrix");
        BFH_REQUIRE(k > 0 && k <= cols && k <= TOPK_MAX_K, "k must be in [1, min(cols, 16384)]");
        if (rows == 0) return;
        ensure();
        const size_t n = static_cast<size_t>(rows) * cols;
        grow(S_, n);
        BFH_HIP(hipMemcpyAsync(S_.get(), scores, n * 4, hipMemcpyHostToDevice, stream));
        grow(d_keys_, static_cast<size_t>(rows) * k);
        const TopkPlan pl = make_plan(m_, 0, rows, cols, 0, k, 0, 0, false);
        allow_dynamic_lds(topk_select_kernel<false>, pl.lds_dense);
        SelectArgs a = select_base(pl, nullptr, nullptr, false, d_keys_.get(), nullptr);
        a.dense = DenseArgs{S_.get(), static_cast<size_t>(cols), cols};
        select_rows(a, rows, pl.lds_dense);
        BFH_HIP(hipMemcpyAsync(result, d_keys_.get(), sizeof(int32_t) * rows * k, hipMemcpyDeviceToHost, stream));
        BFH_HIP(hipStreamSynchronize(stream));
        stats.h2d_bytes += 4.0 * n;
        stats.d2h_bytes += 4.0 * rows * k;
        stats.aux_ms += t_aux_.drain();
    }

    void set_mode(const std::string& name, int64_t v) {
        if (name == "flt_min_rule") m_.flt_min_rule = v != 0;
        else if (name == "fast_select") m_.fast_select = v != 0;
        else if (name == "fused") m_.fused = static_cast<int>(v);
        else if (name == "wave_select") m_.wave_select = v != 0;
        else if (name == "fused_c0") m_.fused_c0 = static_cast<int>(v);
        else if (name == "timing") timing = v != 0;
        else if (name == "score_func") {
            BFH_REQUIRE(v == 0 || v == 1, "score_func must be 0 (dot) or 1 (l2)");
            m_.l2 = v == 1;
        } else throw Error(BFH_ERR_INVALID, "unknown mode '" + name + "'");
    }

 private:
    TopkModes m_;
    int num_cus_ = 256;   // of the device: sizes the tile groups of the sweeps
    DevBuf<int32_t> d_idx_, d_keys_;
    DevBuf<uint32_t> d_pool_;
    DevBuf<float> d_scores_, S_, hP_, hQ_, hQb_;
    DevBuf<float> hb_;    // "score_func" = 1: -|q_j|^2 / 2 of the current call's candidates [q_rows]; only grows
    DevBuf<float> Fn_;    // most_similar: the row-normalised factor matrix [rows, ld]; only grows, reused across calls
    DevBuf<float4> Qp_;   // candidate matrix in MFMA operand order (topk_pack_kernel)
    // fused path: per-query thresholds, candidate segments + counts, rows handed back to the dense path
    DevBuf<float> thr_;
    DevBuf<uint2> cand_, s0_cand_;
    DevBuf<int> cnt_, redo_, general_, s0_cnt_;
    DevBuf<int32_t> redo_side_;
    // recommend_unseen: the training matrix of set_seen (END-offset CSR) and the columns of the current call's pool
    DevBuf<int64_t> seen_indptr_;
    DevBuf<int32_t> seen_keys_;
    int seen_users_ = 0, seen_items_ = 0, pool_cols_ = 0;
    EventTimer t_main_, t_aux_;
};

// csrc/topk_engine.hpp: the ranking as the validation evaluator (csrc/eval.hip) uses it
HandleBase* topk_engine_new(int device) {
    TopkHandle* h = new TopkHandle();
    h->device = device;
    return h;
}
void topk_engine_set_mode(HandleBase* engine, const std::string& name, int64_t value) { static_cast<TopkHandle*>(engine)->set_mode(name, value); }
void topk_engine_rank_unseen(HandleBase* engine, const int32_t* d_rows, int nq, const float* dP, const float* dQ, int q_rows, int d, int ld,
                             const float* dQb, const int64_t* d_seen_indptr, const int32_t* d_seen_keys, int k, int32_t* d_out_keys, int max_batch) {
    TopkHandle* h = static_cast<TopkHandle*>(engine);
    BFH_HIP(hipSetDevice(h->device));
    h->rank_unseen(d_rows, nq, dP, dQ, q_rows, d, ld, dQb, d_seen_indptr, d_seen_keys, k, d_out_keys, max_batch);
}
}  // namespace bfh

using bfh::guarded;
using bfh::TopkHandle;

extern "C" {

BFH_ABI_LIFECYCLE(topk, TopkHandle)

int bfh_topk_dot_topn(void* h, const int32_t* indexes, int num_queries, const float* P, int p_rows, int p_cols, const float* Q, int q_rows,
                      int q_cols, const float* Qb, int qb_rows, int32_t* out_keys, float* out_scores, const int32_t* pool, int pool_size, int k) {
    return guarded<TopkHandle>(h, [&](TopkHandle& t) {
        t.run_host(indexes, num_queries, P, p_rows, p_cols, Q, q_rows, q_cols, Qb, qb_rows, out_keys, out_scores, pool, pool_size, k);
    });
}
int bfh_topk_dot_topn_device(void* h, const int32_t* indexes, int num_queries, const float* dP, int p_rows, const float* dQ, int q_rows, int d,
                             int ld, const float* dQb, int qb_rows, int same, int32_t* out_keys, float* out_scores, const int32_t* pool,
                             int pool_size, int k) {
    return guarded<TopkHandle>(h, [&](TopkHandle& t) {
        for (int i = 0; i < num_queries; ++i)
            if (indexes[i] < 0 || indexes[i] >= p_rows) throw bfh::Error(BFH_ERR_INVALID, "query index outside P");
        if (qb_rows != 0 && qb_rows != q_rows) throw bfh::Error(BFH_ERR_INVALID, "Qb must have one row per row of Q");
        t.refuse_bias(qb_rows != 0);
        t.run_device(indexes, num_queries, dP, true, dQ, q_rows, d, ld, qb_rows ? dQb : nullptr, same != 0, out_keys, out_scores, pool, pool_size, k);
    });
}
int bfh_topk_set_seen(void* h, int num_users, int num_items, const int64_t* seen_indptr, const int32_t* seen_keys, int64_t nnz) {
    return guarded<TopkHandle>(h, [&](TopkHandle& t) { t.set_seen(num_users, num_items, seen_indptr, seen_keys, nnz); });
}
int bfh_topk_recommend_unseen(void* h, const int32_t* users, int num_queries, const float* P, int p_rows, int p_cols, const float* Q, int q_rows,
                              int q_cols, const float* Qb, int qb_rows, int32_t* out_keys, float* out_scores, const int32_t* pool, int pool_size,
                              int k) {
    return guarded<TopkHandle>(h, [&](TopkHandle& t) {
        t.recommend_unseen_host(users, num_queries, P, p_rows, p_cols, Q, q_rows, q_cols, Qb, qb_rows, out_keys, out_scores, pool, pool_size, k);
    });
}
int bfh_topk_recommend_unseen_device(void* h, const int32_t* users, int num_queries, const float* dP, int p_rows, const float* dQ, int q_rows, int d,
                                     int ld, const float* dQb, int qb_rows, int32_t* out_keys, float* out_scores, const int32_t* pool,
                                     int pool_size, int k) {
    return guarded<TopkHandle>(h, [&](TopkHandle& t) {
        t.check_unseen(users, num_queries, p_rows, q_rows, k);
        if (!dP || !dQ) throw bfh::Error(BFH_ERR_INVALID, "null device factor matrix");
        if (qb_rows != 0 && (qb_rows != q_rows || !dQb)) throw bfh::Error(BFH_ERR_INVALID, "Qb must have one row per row of Q");
        t.refuse_bias(qb_rows != 0);
        t.recommend_unseen_device(users, num_queries, dP, true, dQ, q_rows, d, ld, qb_rows ? dQb : nullptr, out_keys, out_scores, pool, pool_size, k);
    });
}
int bfh_topk_normalize(void* h, const float* F, int rows, int cols, float* out) {
    return guarded<TopkHandle>(h, [&](TopkHandle& t) { t.normalize_host(F, rows, cols, out); });
}
int bfh_topk_normalize_device(void* h, const float* dF, int rows, int d, int ld, float* dOut) {
    return guarded<TopkHandle>(h, [&](TopkHandle& t) { t.normalize_device(dF, rows, d, ld, dOut); });
}
int bfh_topk_most_similar(void* h, const int32_t* indexes, int num_queries, const float* F, int rows, int cols, int32_t* out_keys, float* out_scores,
                          const int32_t* pool, int pool_size, int k) {
    return guarded<TopkHandle>(h, [&](TopkHandle& t) {
        t.most_similar_host(indexes, num_queries, F, rows, cols, out_keys, out_scores, pool, pool_size, k);
    });
}
int bfh_topk_most_similar_device(void* h, const int32_t* indexes, int num_queries, const float* dF, int rows, int d, int ld, int32_t* out_keys,
                                 float* out_scores, const int32_t* pool, int pool_size, int k) {
    return guarded<TopkHandle>(h, [&](TopkHandle& t) {
        t.most_similar_device(indexes, num_queries, dF, rows, d, ld, out_keys, out_scores, pool, pool_size, k);
    });
}
int bfh_topk_most_similar_vectors(void* h, const float* V, int num_queries, const float* F, int rows, int cols, int32_t* out_keys,
                                  float* out_scores, const int32_t* pool, int pool_size, int k) {
    return guarded<TopkHandle>(h, [&](TopkHandle& t) {
        t.most_similar_vectors(V, num_queries, F, rows, cols, out_keys, out_scores, pool, pool_size, k);
    });
}
int bfh_topk_quickselect(void* h, const float* scores, int rows, int cols, int32_t* result, int k, int sorted) {
    (void)sorted;   // always sorted
    return guarded<TopkHandle>(h, [&](TopkHandle& t) { t.quickselect(scores, rows, cols, result, k); });
}
int bfh_topk_set_mode(void* h, const char* name, int64_t value) {
    return guarded<TopkHandle>(h, [&](TopkHandle& t) { t.set_mode(name ? name : "", value); });
}

}  // extern "C"
