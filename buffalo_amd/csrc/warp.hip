// WARP on gfx950: the handle (host path of a partial_update call, compute_loss) and the C ABI.  The device code and the kernel
// shape are in warp_kernels.hpp.
//
// Reference semantics: CWARP::worker / update_parameters / compute_loss
// (/root/reference/lib/algo_impl/warp/warp.cc:103-226).  The reference has no GPU WARP
// (/root/reference/buffalo/algo/warp.py:31-32); the object surface is the one warp.py:212-234
// expects from an accelerator (same as CuBPR).
#include "warp_kernels.hpp"

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

 private:
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

}  // extern "C"
