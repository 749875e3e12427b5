// WARP on gfx950: the handle (host path of a partial_update call, compute_loss) and the C ABI.  The device code and the kernel
// shape are in warp_kernels.hpp.
//
// Reference semantics: CWARP::worker / update_parameters / compute_loss
// (/root/reference/lib/algo_impl/warp/warp.cc:103-226).  The reference has no GPU WARP
// (/root/reference/buffalo/algo/warp.py:31-32); the object surface is the one warp.py:212-234
// expects from an accelerator (same as CuBPR).
#include "warp_kernels.hpp"
#include "warp_fold_kernels.hpp"

#include <algorithm>
#include <cmath>

#include "sgd_abi.hpp"

namespace bfh {

class WarpHandle : public SgdHandle {
 public:
    WarpHandle() : SgdHandle(1) {}
    bool project_unit_ball() const override { return true; }  // warp.cc:194-200
    void parse_specific() override {
        BFH_REQUIRE(optimizer_ != "sgd", "WARP accumulates gradients: optimizer must be adagrad or adam");
        max_trial_ = opt_.integer("max_trials");
        threshold_ = opt_.num("threshold");
        // warp.cc:76-83: only the exact string "l2" selects the L2 score (Q-23)
        l2_ = opt_.str("score_func") == "l2";
        cnt_.resize(kWarpCounters, true, stream);
    }
    // "warp_presample" is this handle's own knob; every other name is SgdHandle's
    void set_mode(const std::string& name, int64_t v) override {
        if (name == "warp_presample") {
            BFH_REQUIRE(v == -1 || v == 0 || v == 4 || v == 8, "warp_presample must be -1 (auto), 0, 4 or 8");
            presample_ = static_cast<int>(v);
        } else {
            SgdHandle::set_mode(name, v);
        }
    }
    void device_buffer(const std::string& name, void** p, size_t* bytes) override {
        if (name != "fold") return SgdHandle::device_buffer(name, p, bytes);
        *p = fold_.rows ? fold_.out.get() : nullptr;   // the rows of the last fold_in (which returned with the stream drained)
        *bytes = static_cast<size_t>(fold_.rows) * vdim_ * sizeof(float);
    }
    // the rows of an earlier fold_in belong to the model they were folded against
    void initialize_model(float* P, int P_rows, float* Q, float* Qb, int Q_rows, int64_t num_nnz, bool set_gpu) {
        fold_.rows = 0;
        SgdHandle::initialize_model(P, P_rows, Q, Qb, Q_rows, num_nnz, set_gpu);
    }
    int dim() const { return d_; }   // the unpadded width of a row of init / out (bfh_warp_get_dim)

    void partial_update(int start_x, int next_x, const int64_t* indptr, const int32_t* keys, double* loss_sum, double* n_samples) {
        SgdParams p;
        const int64_t n = stage_chunk(start_x, next_x, indptr, keys, &p);
        *loss_sum = 0.0;
        *n_samples = static_cast<double>(n);
        if (has_comm()) exchange_arm();   // Z = the gradient buffers BEFORE this model accumulates anything (they are exchanged as deltas)
        if (n == 0) return;          // no collective in WARP's partial_update: an empty shard chunk may return
        WarpConsts c = trial_consts(n);                          // the call's constants
        zero_outputs();                                          // the loss sum and the counters
        const int S = presample_depth();                         // candidates per positive from the pre-pass
        if (S > 0) presample(p, n, S, c);                        // draw them, one thread per positive
        if (accum_two_pass_) two_pass_outputs(n, c);             // the trial kernel records (user, Phi, negative) for the gather
        const TrialGrid g = trial_grid((n + chunk_ - 1) / chunk_);   // one wave per work item, up to what the chip keeps resident
        launch_trials(p, c, S, g);                               // trial loop + gradP (+ the item rows by atomics, one-pass)
        if (accum_two_pass_) gather_item_rows(p, start_x, next_x);   // the item rows' gradients, summed per item
        harvest(n, loss_sum);                                    // loss, counters, timers; the stream is idle afterwards
        advance_progress(start_x, next_x, indptr);
    }

    double compute_loss(int n, const int32_t* users, const int32_t* pos, const int32_t* neg) {
        BFH_REQUIRE(model_on_gpu_, "compute_loss before initialize_model(..., set_gpu=True)");
        if (n <= 0) return 0.0;
        const int32_t* inj = upload_triples(n, users, pos, neg);
        BFH_HIP(hipMemsetAsync(cnt_.get(), 0, sizeof(unsigned long long), stream));
        const int slot = t_aux_.begin(stream);
        hipLaunchKernelGGL(warp_loss_kernel, dim3((n + 3) / 4), dim3(256), 0, stream, P_.get(), Q_.get(), inj, inj + n,
                           inj + 2 * n, n, vdim_, static_cast<int>(l2_), threshold_, cnt_.get());
        BFH_HIP(hipGetLastError());
        t_aux_.end(slot, stream);
        unsigned long long v = 0;
        BFH_HIP(hipMemcpyAsync(&v, cnt_.get(), sizeof(v), hipMemcpyDeviceToHost, stream));
        sync_stream();
        harvest_timers();
        return static_cast<double>(v) / static_cast<double>(n);
    }

    // ---- fold-in: rows for histories that are not in the model (bfh_warp_fold_in) --------------------------------------------------------
    // out[b] = the row after `iters` passes of the trial loop over history b against the handle's current Q, which does not move (the rule
    // is in buffalo_hip.h, the kernel in warp_fold_kernels.hpp).  Everything it writes is its own (FoldState); of the training state it
    // reads Q_, the options and the sampler's seed, so it may be called anywhere between two training calls.
    void fold_in(int n_rows, const int64_t* indptr, const int32_t* keys, int64_t nnz, const int32_t* row_ids, int iters, float lr,
                 const float* init, float* out, int64_t* counts, double* kernel_ms) {
        BFH_REQUIRE(model_on_gpu_, "fold_in before initialize_model(..., set_gpu=True)");
        if (vdim_ > 256) throw Error(BFH_ERR_UNSUPPORTED, "fold_in: d = " + std::to_string(d_) + " is above 256, the columns one lane group holds");
        fold_check(n_rows, indptr, keys, nnz, iters);            // refuse bad input on the host
        finish_for_reader();   // an exchange in flight is finished first, as for every reader of Q
        FoldState& f = fold_;
        f.rows = n_rows;
        if (kernel_ms) *kernel_ms = 0.0;
        if (n_rows == 0) return;
        fold_work_items(f, n_rows, indptr, row_ids);             // the histories as work items, longest first
        fold_pass_consts(f, iters, lr);                          // the optimizer's constants of every pass
        WarpFoldArgs a = fold_upload(f, n_rows, keys, nnz, iters, init, out != nullptr, counts != nullptr);
        fold_zero(f, n_rows, counts != nullptr);                 // the ticket and the counts
        fold_launch(f, a);                                       // one launch
        fold_copy_out(f, n_rows, out, counts);                   // one dense copy; the stream is idle afterwards
        const double ms = f.t_fold.drain();
        if (kernel_ms) *kernel_ms = ms;
    }

 private:
    // Everything bfh_warp_fold_in refuses, before anything is uploaded or launched: host scans of the offsets and of all nnz keys.  Serving
    // input is not trusted; an out-of-range key must never reach a gather.  A row that holds every item is not refused: the attempt cap
    // ends its draws.
    void fold_check(int n_rows, const int64_t* indptr, const int32_t* keys, int64_t nnz, int iters) const {
        BFH_REQUIRE(n_rows >= 0, "fold_in: n_rows is negative");
        BFH_REQUIRE(nnz >= 0, "fold_in: nnz is negative");
        BFH_REQUIRE(iters >= 0 && iters <= 10000, "fold_in: iters must be in [0, 10000]");
        BFH_REQUIRE(n_rows == 0 || indptr, "fold_in: null indptr");
        BFH_REQUIRE(nnz == 0 || keys, "fold_in: null keys with nnz > 0");
        int64_t prev = 0;
        for (int b = 0; b < n_rows; ++b) {
            BFH_REQUIRE(indptr[b] >= prev, "fold_in: indptr decreases at row " + std::to_string(b));
            prev = indptr[b];
        }
        BFH_REQUIRE(prev == nnz, "fold_in: indptr[n_rows - 1] != nnz");
        prev = 0;
        for (int b = 0; b < n_rows; ++b) {
            const int64_t beg = prev, end = indptr[b];
            prev = end;
            for (int64_t i = beg; i < end; ++i) {
                const int64_t k = keys[i];
                if (k < 0 || k >= Q_rows_)
                    throw Error(BFH_ERR_INVALID, "fold_in: key " + std::to_string(k) + " at position " + std::to_string(i) + " is outside [0, " +
                                                     std::to_string(Q_rows_) + ")");
                BFH_REQUIRE(i == beg || keys[i - 1] < k, "fold_in: the keys of row " + std::to_string(b) + " are not strictly ascending at position " + std::to_string(i));
            }
        }
    }

    // fold_in's own state: nothing here is read or written by a training call, nothing of the training state is written by fold_in
    struct FoldState {
        int rows = 0;                      // rows of the last call: what device buffer "fold" holds
        DevBuf<float> out;                 // [rows, vdim]: device buffer "fold"
        DevBuf<float> dense;               // [rows, d]: the rows as the caller's `out` takes them
        DevBuf<float> init;                // [rows, vdim]: the caller's start rows
        DevBuf<OptConsts> steps;           // [iters]
        DevBuf<int32_t> keys;
        DevBuf<WarpFoldRow> items;
        DevBuf<int> ticket;
        DevBuf<unsigned long long> counts; // [2 * rows]
        std::vector<WarpFoldRow> host_items;
        std::vector<OptConsts> host_steps;
        std::map<const void*, int> occupancy;   // kernel -> resident 256-thread blocks per CU
        EventTimer t_fold;
    };

    // a stable sort: the order, like the results, is a function of the call alone
    void fold_work_items(FoldState& f, int n_rows, const int64_t* indptr, const int32_t* row_ids) {
        std::vector<WarpFoldRow>& items = f.host_items;
        items.resize(static_cast<size_t>(n_rows));
        for (int b = 0; b < n_rows; ++b) {
            const int64_t beg = b == 0 ? 0 : indptr[b - 1];
            items[b] = WarpFoldRow{beg, static_cast<int32_t>(indptr[b] - beg), b, static_cast<uint32_t>(row_ids ? row_ids[b] : b), 0u};
        }
        std::stable_sort(items.begin(), items.end(), [](const WarpFoldRow& x, const WarpFoldRow& y) { return x.n > y.n; });
    }
    // SgdHandle::optimizer_step's constants for a P row at iteration count t (Q-5: beta2 is read from "beta1")
    void fold_pass_consts(FoldState& f, int iters, float lr) {
        f.host_steps.resize(static_cast<size_t>(std::max(iters, 1)));
        const double b = beta1();
        for (int t = 0; t < iters; ++t) {
            OptConsts& k = f.host_steps[t];
            k.reg2 = static_cast<float>(2.0 * static_cast<double>(reg_u_));
            k.lr = lr;
            k.b1 = k.b2 = static_cast<float>(b);
            k.omb1 = k.omb2 = static_cast<float>(1.0 - b);
            k.c1 = k.c2 = static_cast<float>(1.0 - std::pow(b, t + 1));
        }
    }
    WarpFoldArgs fold_upload(FoldState& f, int n_rows, const int32_t* keys, int64_t nnz, int iters, const float* init, bool dense, bool counts) {
        const size_t nout = static_cast<size_t>(n_rows) * vdim_;
        grow(f.out, nout);
        grow(f.items, static_cast<size_t>(n_rows));
        grow(f.keys, static_cast<size_t>(std::max<int64_t>(nnz, 1)));
        grow(f.steps, f.host_steps.size());
        grow(f.ticket, 1);
        if (counts) grow(f.counts, 2 * static_cast<size_t>(n_rows));
        if (dense) grow(f.dense, static_cast<size_t>(n_rows) * d_);
        BFH_HIP(hipMemcpyAsync(f.items.get(), f.host_items.data(), n_rows * sizeof(WarpFoldRow), hipMemcpyHostToDevice, stream));
        BFH_HIP(hipMemcpyAsync(f.steps.get(), f.host_steps.data(), f.host_steps.size() * sizeof(OptConsts), hipMemcpyHostToDevice, stream));
        if (nnz) BFH_HIP(hipMemcpyAsync(f.keys.get(), keys, nnz * sizeof(int32_t), hipMemcpyHostToDevice, stream));
        if (init) {
            grow(f.init, nout);
            (void)rows_to_device(f.init.get(), vdim_, init, d_, 0, n_rows, stream);   // the pad columns are never read
        }
        WarpFoldArgs a{};
        a.Q = Q_.get();
        a.init = init ? f.init.get() : nullptr;
        a.out = f.out.get();
        a.dense = dense ? f.dense.get() : nullptr;
        a.keys = f.keys.get(); a.rows = f.items.get(); a.steps = f.steps.get();
        a.ticket = f.ticket.get();
        a.counts = counts ? f.counts.get() : nullptr;
        a.n_rows = n_rows; a.Q_rows = Q_rows_; a.d = d_; a.vdim = vdim_; a.iters = iters;
        a.max_trial = max_trial_; a.l2 = l2_; a.pcn = pcn_;
        a.reg_u = reg_u_;
        a.threshold = threshold_;
        a.seed = seed();
        return a;
    }
    void fold_zero(FoldState& f, int n_rows, bool counts) {
        BFH_HIP(hipMemsetAsync(f.ticket.get(), 0, sizeof(int), stream));
        if (counts) BFH_HIP(hipMemsetAsync(f.counts.get(), 0, 2 * static_cast<size_t>(n_rows) * sizeof(unsigned long long), stream));
    }
    // as many blocks as histories, up to what the chip keeps resident ("waves_per_cu" overrides): the blocks behind the first take their
    // histories from the counter
    void fold_launch(FoldState& f, const WarpFoldArgs& a) {
        using KernelFn = void (*)(WarpFoldArgs);
        static const KernelFn table[3][2] = {{warp_fold_kernel<16, false>, warp_fold_kernel<16, true>},
                                             {warp_fold_kernel<32, false>, warp_fold_kernel<32, true>},
                                             {warp_fold_kernel<64, false>, warp_fold_kernel<64, true>}};
        const int G = fold_group_of(vdim_);
        const KernelFn fn = table[G == 16 ? 0 : G == 32 ? 1 : 2][optimizer_ == "adam" ? 1 : 0];
        int64_t resident;
        if (waves_per_cu_ > 0) {
            resident = std::max<int64_t>(1, static_cast<int64_t>(num_cus_) * waves_per_cu_ / 4);
        } else {
            auto it = f.occupancy.find(reinterpret_cast<const void*>(fn));
            if (it == f.occupancy.end()) {
                int blocks = 0;
                BFH_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, fn, 256, 0));
                it = f.occupancy.emplace(reinterpret_cast<const void*>(fn), std::max(1, blocks)).first;
            }
            resident = static_cast<int64_t>(num_cus_) * it->second;
        }
        const int slot = f.t_fold.begin(stream);
        hipLaunchKernelGGL(fn, dim3(static_cast<unsigned>(std::min<int64_t>(a.n_rows, resident))), dim3(256), 0, stream, a);
        BFH_HIP(hipGetLastError());
        f.t_fold.end(slot, stream);
    }
    // a pitched copy into pageable memory goes row by row: the kernel wrote the unpadded rows beside the padded ones
    void fold_copy_out(FoldState& f, int n_rows, float* out, int64_t* counts) {
        if (out) BFH_HIP(hipMemcpyAsync(out, f.dense.get(), static_cast<size_t>(n_rows) * d_ * sizeof(float), hipMemcpyDeviceToHost, stream));
        if (counts) BFH_HIP(hipMemcpyAsync(counts, f.counts.get(), 2 * static_cast<size_t>(n_rows) * sizeof(int64_t), hipMemcpyDeviceToHost, stream));
        sync_stream();
    }
    FoldState fold_;

    struct TrialGrid {
        dim3 grid{1}, block{256};
    };

    WarpConsts trial_consts(int64_t n) {
        WarpConsts c{};
        c.reg_u = reg_u_; c.reg_i = reg_i_; c.reg_j = reg_j_;
        c.threshold = threshold_;
        c.max_trial = max_trial_; c.l2 = l2_; c.pcn = pcn_;
        c.chunk = chunk_;
        c.total = n;
        c.loss_out = scratch_.get();
        c.cnt = cnt_.get();
        return c;
    }
    void zero_outputs() {
        BFH_HIP(hipMemsetAsync(scratch_.get(), 0, sizeof(double), stream));
        BFH_HIP(hipMemsetAsync(cnt_.get(), 0, kWarpCounters * sizeof(unsigned long long), stream));
    }
    // 4 while most positives accept one of their first draws, 8 once they do not; "warp_presample" pins it
    int presample_depth() const { return presample_ < 0 ? (last_T_ > 2.0 ? 8 : 4) : presample_; }
    void presample(const SgdParams& p, int64_t n, int S, WarpConsts& c) {
        if (cand_.size() < static_cast<size_t>(n) * S) cand_.resize(static_cast<size_t>(n) * S);
        if (next_.size() < static_cast<size_t>(n)) next_.resize(static_cast<size_t>(n));
        const int slot = t_aux_.begin(stream);
        hipLaunchKernelGGL(S == 4 ? warp_presample_kernel<4> : warp_presample_kernel<8>, dim3(blocks_of(n)), dim3(256), 0, stream, p, n,
                           cand_.get(), next_.get());
        BFH_HIP(hipGetLastError());
        t_aux_.end(slot, stream);
        c.cand = cand_.get();
        c.next_attempt = next_.get();
    }
    void two_pass_outputs(int64_t n, WarpConsts& c) {
        acc_prepare(n);
        c.two_pass = 1;
        c.uc_out = gather_.uc();
        c.neg_out = gather_.neg();
    }
    TrialGrid trial_grid(int64_t n_work) const {
        TrialGrid g;
        if (sequential_) {
            g.block = dim3(64);   // one wave walks every work item in order
        } else {
            const int wpc = waves_per_cu_ > 0 ? waves_per_cu_ : (vdim_ <= 256 ? 24 : 16);   // 24: what 75-79 VGPRs / 106 SGPRs admit
            g.grid = dim3(static_cast<unsigned>((std::min(static_cast<int64_t>(num_cus_) * wpc, n_work) + 3) / 4));
        }
        return g;
    }
    void launch_trials(const SgdParams& p, const WarpConsts& c, int S, const TrialGrid& g) {
        using KernelFn = void (*)(SgdParams, WarpConsts);
        static const KernelFn table[5][3] = {   // [K class: 1, 2, 4, 8, 16 dwords per lane][S / 4]
            {warp_update_kernel<1, 0>, warp_update_kernel<1, 4>, warp_update_kernel<1, 8>},
            {warp_update_kernel<2, 0>, warp_update_kernel<2, 4>, warp_update_kernel<2, 8>},
            {warp_update_kernel<4, 0>, warp_update_kernel<4, 4>, warp_update_kernel<4, 8>},
            {warp_update_kernel<8, 0>, warp_update_kernel<8, 4>, warp_update_kernel<8, 8>},
            {warp_update_kernel<16, 0>, warp_update_kernel<16, 4>, warp_update_kernel<16, 8>}};
        BFH_REQUIRE(S == 0 || S == 4 || S == 8, "warp_presample must be -1 (auto), 0, 4 or 8");
        const int K = (vdim_ + 63) / 64;
        const int slot = t_main_.begin(stream);
        hipLaunchKernelGGL(table[K <= 1 ? 0 : K <= 2 ? 1 : K <= 4 ? 2 : K <= 8 ? 3 : 4][S / 4], g.grid, g.block, 0, stream, p, c);
        BFH_HIP(hipGetLastError());
        t_main_.end(slot, stream);
    }
    // gi = Phi * p_u - reg_i q_i, gj = -Phi * p_u - reg_j q_j (warp.cc:30-40); L2 score (Q-11, warp.cc:42-52):
    // gi = Phi * (p_u - q_i) - reg_i q_i, gj = -Phi * (p_u - q_j) - reg_j q_j
    void gather_item_rows(const SgdParams& p, int start_x, int next_x) {
        const int slot = t_aux_.begin(stream);
        acc_build_positive_list(p, start_x, next_x);
        const float sab_pos[3] = {1.f, l2_ ? -1.f : 0.f, -reg_i_}, sab_neg[3] = {-1.f, l2_ ? 1.f : 0.f, -reg_j_};
        acc_gather(p, 1, true, true, sab_pos, sab_neg, false);
        t_aux_.end(slot, stream);
    }
    void harvest(int64_t n, double* loss_sum) {
        unsigned long long cnt[kWarpCounters] = {0, 0, 0};
        BFH_HIP(hipMemcpyAsync(loss_sum, scratch_.get(), sizeof(double), hipMemcpyDeviceToHost, stream));
        BFH_HIP(hipMemcpyAsync(cnt, cnt_.get(), sizeof(cnt), hipMemcpyDeviceToHost, stream));
        sync_stream();
        harvest_timers();
        stats.launches += 1;
        stats.samples += n;
        stats.scored_negatives += static_cast<int64_t>(cnt[kWarpScored]);
        stats.accepted += static_cast<int64_t>(cnt[kWarpAccepted]);
        stats.loaded_rows += static_cast<int64_t>(cnt[kWarpLoaded]);
        last_T_ = static_cast<double>(cnt[kWarpScored]) / static_cast<double>(n);
    }

    int max_trial_ = 0;
    int presample_ = -1;      // "warp_presample": candidates per positive from the pre-pass (0, 4, 8; -1: from the last call's T)
    double last_T_ = 0.0;     // scored negatives per positive of the previous call
    DevBuf<int32_t> cand_, next_;
    double threshold_ = 0;
    bool l2_ = false;
    DevBuf<unsigned long long> cnt_;
};

}  // namespace bfh

using bfh::WarpHandle;

extern "C" {

BFH_ABI_SGD(warp, WarpHandle)

int bfh_warp_get_dim(void* h) {
    return bfh::guarded<WarpHandle>(h, [](WarpHandle& x) { return x.dim(); });
}
int bfh_warp_fold_in(void* h, int n_rows, const int64_t* indptr, const int32_t* keys, int64_t nnz, const int32_t* row_ids, int iters, float lr,
                     const float* init, float* out, int64_t* counts, double* kernel_ms) {
    return bfh::guarded<WarpHandle>(h, [&](WarpHandle& x) { x.fold_in(n_rows, indptr, keys, nnz, row_ids, iters, lr, init, out, counts, kernel_ms); });
}

}  // extern "C"
