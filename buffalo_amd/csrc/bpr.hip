// BPRMF on gfx950: the handle (host path of both walks) and the C ABI.  The device code is in bpr_kernels.hpp and bpr_item_major.hpp.
//
// Two walks over the same (u, i, j) triples (the sampler is a pure function of the triple's position, so both see
// the same triples):
//   * bpr_item_major_kernel (bpr_item_major.hpp): the default for optimizer = sgd ("hogwild_atomic" = 3) -- the
//     positive item's row in registers, users owned by XCDs, negatives in per-XCD replicas;
//   * bpr_update_kernel (bpr_kernels.hpp): user-major -- P[u] in registers.  The deterministic parity mode ("sequential"),
//     adam / adagrad gradient accumulation, injected triples and the policies 0 / 1 / 2.
//
// Reference semantics: CBPRMF::worker (/root/reference/lib/algo_impl/bpr/bpr.cc:72-188) -- the CPU
// path, as BASELINE.json's north_star asks -- behind CuBPR's object surface
// (/root/reference/include/buffalo/cuda/bpr/bpr.hpp:29-45).  Not derived from lib/cuda/bpr/bpr.cu:
// that backend materialises (user,pos,neg) arrays in HBM, spends one 128-thread block and two
// block-wide barriers per sample and uses expf instead of the CPU's sigmoid table.
#include "bpr_kernels.hpp"
#include "bpr_item_major.hpp"

#include <algorithm>

#include "sgd_abi.hpp"

namespace bfh {

using ImKernelFn = void (*)(SgdParams, BprConsts, ImQueues);

// What one item-major call decides (BprHandle::im_plan_call); the steps of launch_item_major read it and decide nothing.
struct ImCall {
    int start_x = 0, next_x = 0;
    int64_t n = 0;                  // entries of the staged chunk
    double triples = 0;             // n * num_neg
    bool keeps = false;             // the staged chunk lives on in HBM under csr_generation_: what is built from it may be reused
    // the regrouping
    int nq = 0;                     // queues
    int64_t blocks = 1;             // runs an item's entries are cut into per queue
    int bits = 1;                   // of the sort key (queue, block, item)
    // who holds a user's row
    int64_t users_here = 0;
    bool dual = false;              // two triples per wave
    bool p_rep = false, p_hyb = false;   // per-XCD replicas of P: for every user of the call / for the heavy users
    int spread_mode = 0;            // im_keys_kernel: 0 owner queues, 1 every entry spread, 2 / 3 heavy users' entries spread
    int64_t heavy_deg = 0;
    // the collision rule
    int64_t waves = 0;              // resident waves of the call's kernel
    double inflight = 0, tau = 0;
    // merges
    int64_t sync_updates = 0;       // updates between two merges
    int64_t forced_segments = 0;    // under a communicator: segments = exchange points, identical on every rank (0: the plan's own)
    double cnt_triples = 0, max_stale = 0, stiff_scale = 1;
    bool w_items = false, w_users = false;   // weighted merges of Q / Qb, of the replicated P rows
    int64_t np4 = 0, up4 = 0, uoff4 = 0;     // float4s: replica stride of P, this call's rows and their offset
    // known once the regrouping has the queue bounds (im_plan_queues)
    ImPlan plan;
    double lr_steps_per_count = 0;
};

// ------------------------------------------------------------------------------------------------
class BprHandle : public SgdHandle {
 public:
    BprHandle() : SgdHandle(0) { hogwild_atomic_ = 3; }   // sgd default: the item-major walk (bpr_item_major.hpp)
    ~BprHandle() override {
        if (pre_stream_) {
            (void)hipStreamSynchronize(pre_stream_);
            (void)hipStreamDestroy(pre_stream_);
            (void)hipEventDestroy(pre_done_);
            (void)hipEventDestroy(pre_ready_);
        }
    }
    void parse_specific() override {
        num_neg_ = opt_.integer("num_negative_samples");
        BFH_REQUIRE(num_neg_ >= 1 && num_neg_ <= 255, "num_negative_samples must be in [1,255]");
        verify_neg_ = opt_.boolean_or("verify_neg", true);
        uniform_ = opt_.num_or("sampling_power", 0.0) == 0.0;
        // CBPRMF::build_exp_table bpr.cc:57-63, evaluated on the host exactly like the CPU path
        std::vector<float> t(1000);
        for (int i = 0; i < 1000; ++i) {
            float e = static_cast<float>(std::exp((i / static_cast<float>(1000) * 2 - 1) * 6));
            t[i] = static_cast<float>(1.0 / (e + 1));
        }
        exp_table_.resize(1000);
        BFH_HIP(hipMemcpyAsync(exp_table_.get(), t.data(), 1000 * sizeof(float), hipMemcpyHostToDevice, stream));
        sync_stream();
    }

    // the knobs of policies 2 / 3 are this handle's own; every other name is SgdHandle's
    void set_mode(const std::string& name, int64_t v) override {
        if (name == "xcd_sync_updates") { BFH_REQUIRE(v >= 1, "xcd_sync_updates must be positive"); xcd_sync_updates_ = v; }
        else if (name == "xcd_merge_mean") xcd_merge_mean_ = v != 0;
        else if (name == "xcd_stiff_q" || name == "xcd_stiff_b" || name == "xcd_stiff_p") {
            BFH_REQUIRE(v >= 0 && v <= 100000, name + " is a curvature in permille, 0 (plain sum) .. 100000");
            (name == "xcd_stiff_q" ? xcd_stiff_q_milli_ : name == "xcd_stiff_b" ? xcd_stiff_b_milli_ : xcd_stiff_p_milli_) = static_cast<int>(v);
        }
        else if (name == "im_user_lr_max") { BFH_REQUIRE(v >= 0, "im_user_lr_max is a learning rate in permille >= 0"); im_user_lr_max_milli_ = static_cast<int>(v); }
        else if (name == "xcd_fresh") xcd_fresh_ = v != 0 ? 1 : 0;
        else if (name == "im_drift_budget") { BFH_REQUIRE(v >= 0, "im_drift_budget is a permille value >= 0"); im_drift_budget_milli_ = static_cast<int>(v); }
        else if (name == "im_blocks") { BFH_REQUIRE(v >= 0 && v <= 64, "im_blocks must be in [0,64] (0 = choose from the learning rate)"); im_blocks_ = static_cast<int>(v); }
        else if (name == "im_presample") { BFH_REQUIRE(v >= 0 && v <= 2, "im_presample must be 0 (draw in the walk), 1 (CSR-order array) or 2 (walk-order exceptions)"); im_presample_ = static_cast<int>(v); }
        else if (name == "im_presample_ahead") im_presample_ahead_ = v != 0;
        else if (name == "im_drain_only") im_drain_only_ = v != 0;
        else if (name == "im_single_wave") im_single_wave_ = v != 0;
        else if (name == "im_trace") { BFH_REQUIRE(v >= 0, "im_trace is a capacity in triples"); im_trace_.resize(static_cast<size_t>(v), true, stream); sync_stream(); }
        else if (name == "im_force_queues") { BFH_REQUIRE(v >= 0 && v <= 8, "im_force_queues must be in [0,8]"); im_force_queues_ = static_cast<int>(v); }
        else if (name == "im_p_nt") im_p_nt_ = v != 0;
        else if (name == "im_study") im_study_ = static_cast<int>(v);
        else if (name == "im_dual_generic") im_dual_generic_ = v != 0;
        else if (name == "xcd_stiff_lr_ref") xcd_stiff_lr_ref_micro_ = static_cast<int>(v);
        else if (name == "im_dual") { BFH_REQUIRE(v >= -1 && v <= 1, "im_dual must be -1 (by the call's size), 0 or 1"); im_dual_ = static_cast<int>(v); }
        else if (name == "im_neg_limit") { BFH_REQUIRE(v >= 0, "im_neg_limit must be >= 0"); im_neg_limit_ = static_cast<int>(v); }
        else if (name == "im_user_hybrid") { BFH_REQUIRE(v >= 0 && v <= 2, "im_user_hybrid must be 0 (off), 1 (heavy users over all queues) or 2 (over as few as needed)"); im_user_hybrid_ = static_cast<int>(v); }
        else if (name == "im_user_replicas") { BFH_REQUIRE(v >= -1 && v <= 1, "im_user_replicas must be -1 (by shard size), 0 or 1"); im_user_replicas_ = static_cast<int>(v); }
        else if (name == "im_max_stale") { BFH_REQUIRE(v >= 1, "im_max_stale must be positive"); im_max_stale_ = static_cast<int>(v); }
        else if (name == "xcd_v4") xcd_v4_ = v != 0;
        else if (name == "xcd_hot_tau") { BFH_REQUIRE(v >= 0, "xcd_hot_tau is a permille value >= 0"); xcd_hot_tau_ = static_cast<int>(v); }
        else SgdHandle::set_mode(name, v);
    }
    void device_buffer(const std::string& name, void** p, size_t* bytes) override {
        if (name != "im_trace") return SgdHandle::device_buffer(name, p, bytes);
        finish_for_reader();
        *p = im_trace_.get();
        *bytes = im_trace_.bytes();
    }

    // a side-stream draw may still be reading the matrix that is about to be replaced
    void set_resident_csr(const int64_t* indptr, const int32_t* keys, int64_t nnz) {
        if (pre_stream_) BFH_HIP(hipStreamSynchronize(pre_stream_));
        pre_valid_ = false;
        SgdHandle::set_resident_csr(indptr, keys, nnz);
    }

    BprConsts consts(double lr) {
        BprConsts c{};
        c.lr = static_cast<float>(lr);
        c.lr_d = lr;
        c.reg_b_d = reg_b_d_;
        c.reg_u = reg_u_; c.reg_i = reg_i_; c.reg_j = reg_j_; c.reg_b = reg_b_;
        c.use_bias = use_bias_; c.update_i = update_i_; c.update_j = update_j_;
        c.verify_neg = verify_neg_; c.uniform = uniform_; c.num_neg = num_neg_; c.neg_limit = im_neg_limit_;
        c.pcn = pcn_; c.compute_loss = compute_loss_;
        c.atomic = hogwild_atomic_; c.sequential = sequential_;
        c.cum_total = cum_total_;
        c.exp_table = exp_table_.get();
        c.loss_out = scratch_.get();
        c.chunk = chunk_;
        if (xcd_replicas()) {
            if (!chunk_set_) c.chunk = 64;   // short work items: a segment ends when its slowest wave does
            c.atomic = 2;
            c.fresh = xcd_fresh_ > 0;
        } else if (item_major()) {
            c.atomic = 3;
            c.fresh = xcd_fresh_ != 0;       // default (-1): on
        } else if (c.atomic >= 2) {
            c.atomic = 1;                    // adam/adagrad accumulate exact sums: atomics
        }
        return c;
    }

    using KernelFn = void (*)(SgdParams, BprConsts);

    template <int K, bool INJECT, bool V4>
    KernelFn pick_k() const {
        const bool sgd = optimizer_ == "sgd";
        const bool pipe = prefetch_ != 0 && !sequential_;
        if (sgd && pipe) return bpr_update_kernel<K, true, true, INJECT, V4>;
        if (sgd) return bpr_update_kernel<K, true, false, INJECT, V4>;
        if (pipe) return bpr_update_kernel<K, false, true, INJECT, V4>;
        return bpr_update_kernel<K, false, false, INJECT, V4>;
    }
    // the instantiation for this handle's vdim / optimizer / policy
    template <bool INJECT>
    KernelFn pick(const BprConsts& c) const {
        // write-through Hogwild (policy 0; policy 2 on request) moves item rows as float4 with sc1; the
        // atomic, the replica and the deterministic sequential paths keep the dword-per-lane layout
        const bool v4 = optimizer_ == "sgd" && !sequential_ && (c.atomic == 0 || (c.atomic == 2 && xcd_v4_));
        if (v4) {
            const int KV = (vdim_ + 255) / 256;
            if (KV <= 1) return pick_k<4, INJECT, true>();
            if (KV <= 2) return pick_k<8, INJECT, true>();
            return pick_k<16, INJECT, true>();
        }
        const int K = (vdim_ + 63) / 64;
        if (K <= 1) return pick_k<1, INJECT, false>();
        if (K <= 2) return pick_k<2, INJECT, false>();
        if (K <= 4) return pick_k<4, INJECT, false>();
        if (K <= 8) return pick_k<8, INJECT, false>();
        return pick_k<16, INJECT, false>();
    }
    // waves of `fn` the chip keeps resident at once (256-thread blocks); "waves_per_cu" overrides.  The one occupancy cache: it serves the
    // user-major kernels (policies 0 - 2) and whatever im_kernel names (policy 3)
    int64_t resident_waves(const void* fn) {
        if (waves_per_cu_ > 0) return static_cast<int64_t>(num_cus_) * waves_per_cu_;
        auto it = occupancy_.find(fn);
        if (it == occupancy_.end()) {
            int blocks = 0;
            BFH_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, fn, 256, 0));
            it = occupancy_.emplace(fn, std::max(1, std::min(blocks, 8))).first;
        }
        return static_cast<int64_t>(num_cus_) * it->second * 4;
    }

    bool xcd_replicas() const { return hogwild_atomic_ == 2 && optimizer_ == "sgd" && !sequential_; }
    bool item_major() const { return hogwild_atomic_ == 3 && optimizer_ == "sgd" && !sequential_; }
    // item-major default: no prefetch, rows are read where they are used (narrowest race window, least traffic,
    // 7 waves per SIMD cover the latency); "prefetch" = 1 selects the two-triples-ahead slots
    bool im_prefetch() const { return prefetch_ > 0; }

    // ---------------------------------------------------------------------------------------------
    // the item histogram (policies 2 and 3): itemcnt_[i] = how often item i occurs in what was counted
    // ---------------------------------------------------------------------------------------------
    void count_items(const int32_t* idx, int64_t n) {
        hipLaunchKernelGGL(item_count_kernel, dim3(static_cast<unsigned>(std::min<int64_t>((n + 255) / 256, 4096))), dim3(256), 0, stream, idx, n,
                           itemcnt_.get());
    }
    // Is the histogram counted under (gen, start_x, next_x) still there?  If not it is zeroed and stamped with that identity, and the
    // caller counts into it.  gen = -1: what is counted now is never reused.
    bool itemcnt_kept(int64_t gen, int start_x, int next_x) {
        itemcnt_.resize(static_cast<size_t>(Q_rows_));
        if (gen >= 0 && itemcnt_gen_ == gen && itemcnt_start_ == start_x && itemcnt_next_ == next_x) return true;
        BFH_HIP(hipMemsetAsync(itemcnt_.get(), 0, itemcnt_.bytes(), stream));
        itemcnt_gen_ = gen;
        itemcnt_start_ = start_x; itemcnt_next_ = next_x;
        return false;
    }
    // popularity of the positives: of the whole resident matrix (counted once per generation), else of the staged chunk, whose histogram
    // is kept under `chunk_gen` (-1: counted anew by every call)
    void count_positives(const SgdParams& p, int64_t chunk_gen, int start_x, int next_x) {
        if (resident_) {
            if (!itemcnt_kept(csr_generation_, -1, -1)) count_items(keys_.get(), resident_nnz_);
        } else if (!itemcnt_kept(chunk_gen, start_x, next_x)) {
            count_items(p.keys, p.chunk_nnz);
        }
    }

    // ---------------------------------------------------------------------------------------------
    // policy 3 (bpr_item_major.hpp)
    // ---------------------------------------------------------------------------------------------
    void im_probe() {   // which XCC ids do workgroups of this device report?
        if (im_nq_ > 0) return;
        DevBuf<int> seen;
        seen.resize(16, true, stream);
        hipLaunchKernelGGL(xcd_probe_kernel, dim3(4096), dim3(64), 0, stream, seen.get());
        BFH_HIP(hipGetLastError());
        int host[16];
        BFH_HIP(hipMemcpyAsync(host, seen.get(), sizeof(host), hipMemcpyDeviceToHost, stream));
        sync_stream();
        int n = 0;
        for (int i = 0; i < 16; ++i) im_xcd_queue_[i] = host[i] ? n++ : -1;
        BFH_REQUIRE(n >= 1 && n <= kImMaxQueues, "hogwild_atomic=3: unexpected number of XCDs reported by HW_REG_XCC_ID");
        im_nq_ = n;
    }

    // whole 32-element groups per row: the instantiation without per-lane guards ("im_dual_generic" = 1 keeps the guarded one: A/B)
    int im_dual_nk() const { return (vdim_ % 32 == 0 && vdim_ <= 128 && !im_dual_generic_) ? vdim_ / 32 : 0; }
    // two triples per wave (bpr_item_major_dual_kernel): vdim <= 128, rows read where they are used, not a test-hook run
    // Measured (profiles/r02_dual_triples_per_wave.txt, same box): 4.95 -> 4.56 ms per launch (4.20 without the hot-user atomics, whose
    // share grows because twice as many rows are held per queue); 16, 20 and 24 waves per CU give the same time -- the walk is at the
    // fabric's ceiling there, so the kernel is built for 5 waves per SIMD (81 VGPRs, no scratch).  "im_dual" = 0 keeps the one-triple walk.
    // On small shards it used to lose (per-rank epoch at 4 shards 2.42 -> 2.54 ms, at 8 shards 1.31 -> 1.37: twice the rows held per queue
    // on few users turns more of them hot) and was used from 6144 users per queue up.  After the kernel's diet it wins there too
    // (profiles/r06_walk_variance.txt, call 32: 4 shards 2.29 -> 1.94 ms, 8 shards 1.42 -> 1.29), so the default is 1024 users per queue.
    bool im_choose_dual(int64_t users_here, int nq) const {
        return im_dual_ != 0 && vdim_ <= 128 && !im_prefetch() && !im_single_wave_ && !im_drain_only_ &&
               (im_dual_ > 0 || users_here >= static_cast<int64_t>(nq) * 1024);
    }
    // THE item-major kernel of a call: the walk -- two triples per wave where the call chose so (`dual`), else by row width and
    // prefetch -- or its drain instantiation.  im_launch launches what this returns and the occupancy query asks about it.
    ImKernelFn im_kernel(bool dual, bool drain) const {
        if (dual && !drain) {
            switch (im_dual_nk()) {
                case 1: return bpr_item_major_dual_kernel<1>;
                case 2: return bpr_item_major_dual_kernel<2>;
                case 3: return bpr_item_major_dual_kernel<3>;
                case 4: return bpr_item_major_dual_kernel<4>;
                default: return bpr_item_major_dual_kernel<0>;
            }
        }
        static const ImKernelFn drains[3] = {bpr_item_major_kernel<4, false, true>, bpr_item_major_kernel<8, false, true>, bpr_item_major_kernel<16, false, true>};
        static const ImKernelFn pipe[3] = {bpr_item_major_kernel<4, true, false>, bpr_item_major_kernel<8, true, false>, bpr_item_major_kernel<16, true, false>};
        static const ImKernelFn plain[3] = {bpr_item_major_kernel<4, false, false>, bpr_item_major_kernel<8, false, false>, bpr_item_major_kernel<16, false, false>};
        const int KV = (vdim_ + 255) / 256;
        return (drain ? drains : (im_prefetch() ? pipe : plain))[KV <= 1 ? 0 : (KV <= 2 ? 1 : 2)];
    }
    void im_launch(const SgdParams& p, const BprConsts& c, const ImQueues& q, const ImCall& k, int64_t waves, bool drain) {
        // "im_single_wave" (test hook): one wave drains every queue in ticket order -- a deterministic sequential run
        const dim3 grid(im_single_wave_ ? 1u : static_cast<unsigned>((waves + 3) / 4)), block(im_single_wave_ ? 64 : 256);
        hipLaunchKernelGGL(im_kernel(k.dual, drain), grid, block, 0, stream, p, c, q);
        BFH_HIP(hipGetLastError());
    }

    // The item-major regrouping sorts 32-bit keys (queue, block, item) with 32-bit entry indices.  Null when a call of n entries fits, else
    // the limit it exceeds: partial_update then falls back to policy 1 instead of failing (about 33 M items at lr >= 0.1, or 2^31
    // interactions per call).  `blocks`: the runs an item's entries are cut into per queue.
    const char* im_limit(const BprConsts& c, int64_t n, int64_t* blocks) const {
        // what a run of consecutive positive steps does to a row grows with lr x run length (DESIGN.md "burst length": invisible at
        // lr 0.002, a 7 % worse sampled loss at lr 0.05 with one run, gone with 8), so the default follows the call's learning rate;
        // "im_blocks" pins it
        *blocks = im_blocks_ > 0 ? im_blocks_ : std::min<int64_t>(16, std::max<int64_t>(1, static_cast<int64_t>(std::ceil(c.lr * 160.0))));
        if (n >= (int64_t(1) << 31)) return "hogwild_atomic=3: chunk of 2^31 or more interactions";
        if (static_cast<int64_t>(im_nq_) * *blocks * Q_rows_ >= (int64_t(1) << 32)) return "hogwild_atomic=3: too many items for the 32-bit sort key";
        return nullptr;
    }
    bool im_fits(const BprConsts& c, int64_t n) {
        im_probe();
        int64_t blocks;
        return im_limit(c, n, &blocks) == nullptr;
    }

    // Everything one call over the staged chunk [start_x, next_x) decides, before anything is launched.  (The slice schedule alone needs the
    // queue bounds, which the regrouping's sort produces: im_plan_queues.)
    ImCall im_plan_call(const SgdParams& p, const BprConsts& c, int start_x, int next_x, int64_t comm_points) {
        im_probe();
        ImCall k;
        k.start_x = start_x; k.next_x = next_x;
        k.n = p.chunk_nnz;
        k.triples = static_cast<double>(c.total);
        const char* over = im_limit(c, k.n, &k.blocks);
        BFH_REQUIRE(!over, over);
        k.nq = (im_single_wave_ && im_force_queues_ > 0) ? std::min(im_force_queues_, kImMaxQueues) : im_nq_;
        // the weight of n replicas assumes the merge sums exactly those: nq <= kXcdReplicas
        BFH_REQUIRE(k.nq <= kXcdReplicas, "hogwild_atomic=3: more queues than per-XCD replicas");
        while ((int64_t(1) << k.bits) < static_cast<int64_t>(k.nq) * k.blocks * Q_rows_) ++k.bits;
        k.keeps = chunk_kept();
        k.users_here = next_x - start_x;
        k.dual = im_choose_dual(k.users_here, k.nq);   // before the occupancy query: which kernel is asked depends on it
        // Small shards (multi-GPU): the same waves work on an N-times smaller user set, and with one owner XCD per user most
        // triples fall under the collision rule and pay a user-row atomic (8 shards of ML-20M: 3/4 of them, 1.44 vs 1.15 ms).
        // There the users get what the negatives have: per-XCD replicas of P, entries spread over the queues by position (a
        // user's share of one queue is nq times smaller), plain stores through the XCD's own L2, the delta rule at the merges.
        // Measured (profiles/r02_shard_times_user_replicas.txt, ML-20M / d=128, per-rank epoch): 8 shards 1.73 -> 1.31 ms (walk 1.52 -> 1.07);
        // 4 shards 2.43 -> 2.65, 2 shards 4.32 -> 5.45, whole matrix 9.2 -> 10.2: eight copies of a big P fall out of the Infinity Cache,
        // so the rule is "fewer than 3072 users per queue".  Statistics (profiles/r02_gate_study_user_replicas.txt, whole matrix, 8 copies):
        // at the reference's lr the gate metrics stay inside the oracle pair's spread; at lr 0.05 the sum of eight deltas of a heavy
        // user overshoots (|P| 390 vs 430, one run in three diverging), so above lr 0.01 the owner form stays.
        const float user_lr_max = im_user_lr_max_milli_ * 1e-3f;
        k.p_rep = im_user_replicas_ > 0 ||
                  (im_user_replicas_ < 0 && !im_single_wave_ && k.users_here < static_cast<int64_t>(k.nq) * 3072 && c.lr <= user_lr_max);
        k.waves = resident_waves(reinterpret_cast<const void*>(im_kernel(k.dual, false)));
        // rows a queue's waves hold between the load and the store of one update: the current and the prefetched
        // triple's, or -- when the row is re-read right before the store -- one L2 round trip out of a triple's time
        k.inflight = (!im_prefetch() ? 0.25 : (c.fresh ? 0.5 : 2.0)) * (static_cast<double>(k.waves) / k.nq) * (k.dual ? 2.0 : 1.0);
        k.tau = xcd_hot_tau_ * 1e-3;
        // Whole matrices keep one owner XCD per user -- except for the HEAVY users, the ones the collision rule would put on
        // fp32 atomics (ML-20M shape: degree >= ~780, 2 % of the users, 17 % of the triples; `xcd_hot_tau = 0` showed those atomics
        // cost 8 % of the walk).  They alone get the replica treatment: their entries are spread over the queues, so a heavy user's
        // share of one queue is nq times smaller and its row is updated with plain stores on the XCD's replica; 13 MB of replicas
        // instead of 640, merged by the delta rule with the item replicas.  Same lr bound as the all-user form.
        k.p_hyb = !k.p_rep && im_user_hybrid_ && !im_single_wave_ && c.lr <= user_lr_max && k.tau > 0.0 && k.inflight > 0.0 && k.nq > 1;
        // degree from which the owner-share rule fires: deg * num_neg / (triples / nq) * inflight >= tau
        k.heavy_deg = k.p_hyb ? std::max<int64_t>(1, static_cast<int64_t>(std::ceil(k.tau * (static_cast<double>(c.total) / k.nq) / (k.inflight * num_neg_)))) : 0;
        k.spread_mode = k.p_rep ? 1 : (k.p_hyb ? (im_user_hybrid_ >= 2 ? 3 : 2) : 0);
        k.sync_updates = xcd_sync_updates_ > 0 ? xcd_sync_updates_ : int64_t(1) << 23;
        if (has_comm()) {
            // multi-GPU: every merge segment is an exchange point.  By default a call is ONE segment whose exchange is finished
            // before it returns (blocking).  "comm_segments" = k cuts the call into k segments whose exchanges travel behind the
            // NEXT segment's walk (one segment late; the last one stays in flight until the next exchange point or reader).
            // Measured / simulated (profiles/r02_shard_times_*, r02_local_sgd_study_*): a segment costs ~0.2 ms of merge / drain /
            // launch-tail work on top of its walk -- as much as the 14 MB all-reduce it hides -- so on ML-20M pipelining loses at
            // every N (N = 2: 5.1 ms per epoch with four segments against 4.2 + ~0.2 blocking); and a delta that lands one
            // interval late needs >= 4 exchange points per epoch to match the blocking exchange's statistics (8 ranks, lr 0.002:
            // the popular items' biases end 40 % off with one delayed exchange, 14 % with two, 1.5 % with four; blocking: 6 %).
            // It pays only where a walk is long against the fixed cost (large d, WARP-sized shards).
            // Every rank must run the SAME number of exchange points per call (each is a collective): the knob, not local sizes.
            k.forced_segments = comm_points;
            k.sync_updates = std::min<int64_t>(k.sync_updates, std::max<int64_t>(1, (c.total + comm_points - 1) / comm_points));
        }
        // what the item counts are normalised by
        k.cnt_triples = resident_ ? static_cast<double>(resident_nnz_) * num_neg_ : k.triples;
        // the staleness budgets are stated for lr = 0.05 and scale with 1 / lr: what matters is how far a row moves
        const double lr_scale = c.lr > 0.f ? 0.05 / static_cast<double>(c.lr) : 1e9;
        k.max_stale = std::min(1e9, static_cast<double>(im_max_stale_) * lr_scale);
        // The stiffness constants model a row that contracts towards a local equilibrium by exp(-lr k) per step with k = the curvature of the
        // sigmoid (<= 1/4).  They were calibrated at the reference's default lr (0.002).  A row whose steps are large -- a higher lr -- sits in
        // the flat part of the sigmoid for most of them (the reference path's own biases at lr 0.05: logits of a few per cent), its curvature is a
        // fraction of 1/4, and the constant over-damps: measured on the reference benchmark's schedule (lr 0.05 -> 0.0001, 10 epochs) the merged
        // negative steps of the biases were scaled by ~0.36 in the middle epochs and |Qb| ended at 147.7 against 183.0 for the reference path at
        // EVERY pool width and for this library's own all-atomic kernel (profiles/r06_bpr_lr005_width_and_knobs.txt, r06_bpr_lr005_bias_rows.txt).
        // Above the calibration lr the constants therefore shrink like lr_ref / lr: the argument x = lr k m of the saturation weight stays what it
        // is at lr_ref.  ("xcd_stiff_lr_ref" = 0: the constants at every lr.)
        const double lr_ref = xcd_stiff_lr_ref_micro_ * 1e-6;
        k.stiff_scale = (lr_ref > 0.0 && static_cast<double>(c.lr) > lr_ref) ? lr_ref / static_cast<double>(c.lr) : 1.0;
        // weights of the merges' sums (off = plain sum): not for the single-wave test hook (one wave takes every step there, in ONE replica,
        // and the sum is already the sequential result), nor with "xcd_merge_mean" (the mean already scales the sum by 1 / n, and a
        // saturation weight between 1 / n and 1 on top of it would damp the rows twice)
        k.w_items = (xcd_stiff_q_milli_ > 0 || xcd_stiff_b_milli_ > 0) && !im_single_wave_ && !xcd_merge_mean_;
        k.w_users = xcd_stiff_p_milli_ > 0 && k.spread_mode != 0 && !im_single_wave_ && !xcd_merge_mean_;
        k.np4 = static_cast<int64_t>(P_rows_) * vdim_ / 4;
        k.up4 = k.users_here * vdim_ / 4;
        k.uoff4 = static_cast<int64_t>(start_x) * vdim_ / 4;
        return k;
    }
    // ... and, once im_regroup has the queue bounds, the slice schedule and what follows from its number of merge segments
    void im_plan_queues(const BprConsts& c, ImCall& k) const {
        int64_t q_entries[kImMaxQueues] = {0};
        for (int x = 0; x < k.nq; ++x) q_entries[x] = im_qbeg_[x + 1] - im_qbeg_[x];
        k.plan = im_make_plan(k.nq, q_entries, num_neg_, k.sync_updates);
        if (k.forced_segments > 0) k.plan.segments = k.forced_segments;   // not left to the rounding of local sizes
        // positive steps of a row between two merges, in units of lr: counts (of `cnt_triples` triples) -> this call's share
        k.lr_steps_per_count = static_cast<double>(num_neg_) * (k.triples / k.cnt_triples) / static_cast<double>(k.plan.segments) * c.lr;
    }

    // ---- the steps of a call, in stream order ----
    // entries grouped by (owner queue of the user, item); cached for a chunk that lives on in HBM
    void im_regroup(const SgdParams& p, const ImCall& k) {
        const int64_t n = k.n;
        if (k.keeps && im_gen_ == csr_generation_ && im_start_ == k.start_x && im_next_ == k.next_x && im_n_ == n && im_built_blocks_ == k.blocks &&
            im_built_nq_ == k.nq && im_built_spread_mode_ == k.spread_mode && im_built_heavy_deg_ == k.heavy_deg)
            return;
        // a side-stream draw in the walk-order layout reads the inverse of the sort that is rebuilt below
        if (pre_valid_) BFH_HIP(hipStreamSynchronize(pre_stream_));
        im_key_a_.resize(static_cast<size_t>(n)); im_key_b_.resize(static_cast<size_t>(n));
        im_pos_a_.resize(static_cast<size_t>(n)); im_pos_b_.resize(static_cast<size_t>(n));
        im_qbeg_dev_.resize(kImMaxQueues + 1);
        hipLaunchKernelGGL(im_keys_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, stream, p.rows, p.keys, n, k.nq,
                           static_cast<uint32_t>(k.blocks), static_cast<uint32_t>(Q_rows_), k.spread_mode, p.indptr, k.heavy_deg, im_key_a_.get(), im_pos_a_.get());
        BFH_HIP(hipGetLastError());
        device_sort_pairs_u32(im_key_a_.get(), im_key_b_.get(), im_pos_a_.get(), im_pos_b_.get(), n, k.bits, im_tmp_, stream);
        hipLaunchKernelGGL(im_bounds_kernel, dim3(1), dim3(64), 0, stream, im_key_b_.get(), n, k.nq, static_cast<uint32_t>(k.blocks * Q_rows_),
                           im_qbeg_dev_.get());
        BFH_HIP(hipGetLastError());
        if (k.keeps) {   // what the walk-order layout needs beside the sort; lives and dies with the cached regrouping
            im_ent_user_.resize(static_cast<size_t>(n)); im_ent_inv_.resize(static_cast<size_t>(n));
            hipLaunchKernelGGL(im_entry_users_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, stream, p.rows, im_pos_b_.get(), n,
                               im_ent_user_.get(), im_ent_inv_.get());
            BFH_HIP(hipGetLastError());
        }
        BFH_HIP(hipMemcpyAsync(im_qbeg_, im_qbeg_dev_.get(), (k.nq + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, stream));
        sync_stream();
        im_regroup_id_ += 1;
        im_gen_ = k.keeps ? csr_generation_ : -1;
        im_start_ = k.start_x; im_next_ = k.next_x; im_n_ = n; im_built_blocks_ = k.blocks; im_built_nq_ = k.nq;
        im_built_spread_mode_ = k.spread_mode; im_built_heavy_deg_ = k.heavy_deg;
    }
    // per-row policy flags: hot item rows and their flush intervals, hot / replicated users
    void im_row_flags(const SgdParams& p, const ImCall& k) {
        hot_.resize(static_cast<size_t>(Q_rows_));
        im_flush_.resize(static_cast<size_t>(Q_rows_));
        im_hot_user_.resize(static_cast<size_t>(P_rows_));
        hipLaunchKernelGGL(im_item_flags_kernel, dim3((Q_rows_ + 255) / 256), dim3(256), 0, stream, itemcnt_.get(),
                           uniform_ ? nullptr : p.cum_table, cum_total_, Q_rows_, static_cast<double>(num_neg_), k.cnt_triples,
                           uniform_ ? 1.0 / Q_rows_ : 0.0, k.inflight, k.tau, static_cast<double>(k.waves) * (k.dual ? 2.0 : 1.0), k.max_stale, k.lr_steps_per_count,
                           im_drift_budget_milli_ * 1e-3, hot_.get(), im_flush_.get());
        BFH_HIP(hipMemsetAsync(im_hot_user_.get(), 0, im_hot_user_.bytes(), stream));
        hipLaunchKernelGGL(im_user_flags_kernel, dim3((k.users_here + 255) / 256), dim3(256), 0, stream, p.indptr, k.start_x, static_cast<int>(k.users_here),
                           static_cast<double>(num_neg_), k.triples / k.nq, k.triples, k.inflight, k.tau, k.spread_mode >= 2 ? 2 : k.spread_mode, k.heavy_deg, im_hot_user_.get());
        BFH_HIP(hipGetLastError());
    }
    // weights of the merges' sums (ImCall::w_items / w_users)
    void im_merge_weights(const SgdParams& p, const BprConsts& c, const ImCall& k) {
        const double segments = static_cast<double>(k.plan.segments);
        if (k.w_items) {
            xcd_wq_.resize(static_cast<size_t>(Q_rows_));
            xcd_wb_.resize(static_cast<size_t>(Q_rows_));
            hipLaunchKernelGGL(xcd_item_weight_kernel, dim3((Q_rows_ + 255) / 256), dim3(256), 0, stream, uniform_ ? nullptr : p.cum_table, cum_total_, Q_rows_,
                               k.triples / segments, uniform_ ? 1.0 / Q_rows_ : 0.0, static_cast<double>(c.lr), xcd_stiff_q_milli_ * 1e-3 * k.stiff_scale,
                               xcd_stiff_b_milli_ * 1e-3 * k.stiff_scale, k.nq, xcd_wq_.get(), xcd_wb_.get());
        }
        if (k.w_users) {
            xcd_wp_.resize(static_cast<size_t>(P_rows_));
            hipLaunchKernelGGL(xcd_user_weight_kernel, dim3((k.users_here + 255) / 256), dim3(256), 0, stream, p.indptr, k.start_x, static_cast<int>(k.users_here),
                               static_cast<double>(num_neg_) / segments, static_cast<double>(c.lr), xcd_stiff_p_milli_ * 1e-3 * k.stiff_scale, k.nq, k.spread_mode,
                               k.heavy_deg, xcd_wp_.get());
        }
        BFH_HIP(hipGetLastError());
    }
    // replicas of the item factors (+ the copy they started from), and of the P rows of the users that have them
    void im_replicas_begin(BprConsts& c, const ImCall& k) {
        xcd_alloc(true);
        c.rep_Q = repQ_.get();
        c.rep_Qb = repQb_.get();
        c.rep_stride = static_cast<int64_t>(Q_rows_) * vdim_;
        c.rep_bstride = rep_bstride();
        c.hot = hot_.get();
        xcd_broadcast(true);
        if (!k.p_rep && !k.p_hyb) return;
        // eight replicas + the copy they started from, addressed like P (only the rows of users with flag 2 are ever touched);
        // P itself receives the hot users' atomics and whatever the drain launch does
        if (repP_.size() < static_cast<size_t>(kXcdReplicas + 1) * P_rows_ * vdim_) repP_.resize(static_cast<size_t>(kXcdReplicas + 1) * P_rows_ * vdim_);
        hipLaunchKernelGGL((xcd_broadcast_rows_kernel<float4>), dim3(static_cast<unsigned>(std::min<int64_t>((k.up4 + 255) / 256, 8192))), dim3(256), 0, stream,
                           reinterpret_cast<const float4*>(P_.get()) + k.uoff4, reinterpret_cast<float4*>(repP_.get()) + k.uoff4, k.up4, k.np4, kXcdReplicas + 1,
                           static_cast<const uint8_t*>(im_hot_user_.get()) + k.start_x, vdim_ / 4, 2);
        BFH_HIP(hipGetLastError());
    }
    // P <- P + sum_x (P_x - B) for the users that have replicas (flag 2); the others were updated in P itself
    void im_merge_users(const ImCall& k, bool write_replicas) {
        hipLaunchKernelGGL((xcd_merge_kernel<float4>), dim3(static_cast<unsigned>(std::min<int64_t>((k.up4 + 255) / 256, 8192))), dim3(256), 0, stream,
                           reinterpret_cast<float4*>(P_.get()) + k.uoff4, reinterpret_cast<float4*>(repP_.get()) + k.uoff4, k.up4, k.np4, 1.0f,
                           write_replicas ? 1 : 0, static_cast<const uint8_t*>(im_hot_user_.get()) + k.start_x, vdim_ / 4,
                           reinterpret_cast<float4*>(repP_.get()) + kXcdReplicas * k.np4 + k.uoff4, 2, k.w_users ? xcd_wp_.get() + k.start_x : nullptr);
        BFH_HIP(hipGetLastError());
    }
    // The call's negatives, drawn in CSR order before the walk ("im_presample" = 0: nothing, the walk draws its own).  Two layouts:
    //   1: every triple's negative at its nnz position (bpr_presample_kernel) -- the walk gathers rows[pos] and neg_pre[pos];
    //   2: the walk computes the first draw itself and is told, in ITS order, only where that draw was rejected (one bit per triple
    //      + the final negative: bpr_presample_exceptions_kernel); with the entry's user beside the entry (im_regroup) nothing in the
    //      walk's prologue is a gather.  The library's choice when sampling is uniform (a first draw is one multiply; the popularity
    //      sampler's is a binary search) and the chunk lives on in HBM (the inverse of the sort is cached with the regrouping).
    //      In-process A/B against layout 1 on the ML-20M shape, counters and the no-gather ceiling: profiles/bpr_walk_order_metadata.txt.
    // A draw is a pure function of (seed, nnz position, slot, epoch, attempt) -- not of the model -- so the negatives of
    // the NEXT epoch over this same chunk can be drawn on a side stream while this epoch's walk runs (0.35 ms per
    // ML-20M epoch off the critical path).  The speculation is keyed on everything the draws depend on -- in layout 2 that includes
    // the regrouping they were written against: im_limit derives `blocks` from the learning rate, so on a decaying schedule the sort
    // can change between two epochs.  A call the speculation does not match (another chunk, the same epoch again, changed keys,
    // another layout or regrouping) draws its own on the main stream.
    int im_neg_layout(const BprConsts& c, const ImCall& k) const { return !im_presample_ ? 0 : ((im_presample_ == 2 && c.uniform && k.keeps) ? 2 : 1); }
    struct ImNegatives {
        const int32_t* pre = nullptr;
        const uint32_t* bits = nullptr;
        const int32_t* exc = nullptr;
    };
    void im_presample_launch(const SgdParams& p, const BprConsts& c, int layout, int buf, hipStream_t s) {
        const dim3 pgrid(static_cast<unsigned>((c.total + 255) / 256)), pblock(256);
        if (layout == 2) {
            BFH_HIP(hipMemsetAsync(im_neg_bits_[buf].get(), 0, im_neg_bits_[buf].bytes(), s));
            hipLaunchKernelGGL(bpr_presample_exceptions_kernel, pgrid, pblock, 0, s, p, c, im_ent_inv_.get(), im_neg_bits_[buf].get(), im_neg_[buf].get());
        } else {
            hipLaunchKernelGGL(bpr_presample_kernel, pgrid, pblock, 0, s, p, c, im_neg_[buf].get());
        }
        BFH_HIP(hipGetLastError());
    }
    ImNegatives im_draw_negatives(const SgdParams& p, const BprConsts& c, const ImCall& k) {
        const int layout = im_neg_layout(c, k);
        if (!layout) return ImNegatives{};
        const PreKey want{static_cast<int64_t>(p.epoch), k.start_x, k.next_x, c.total, csr_generation_, p.nnz_offset, p.shift, static_cast<int64_t>(p.seed),
                          (c.uniform ? 1 : 0) | (c.verify_neg ? 2 : 0) | (c.num_neg << 2), c.cum_total, layout, layout == 2 ? im_regroup_id_ : 0};
        // the buffers at their size before anything is launched into them (a resize frees): this call's, and the speculation's
        const bool ahead = im_presample_ahead_ && k.keeps;
        const size_t words = static_cast<size_t>((c.total + 31) / 32);
        bool grow_now = false;
        for (int b = 0; b < (ahead ? 2 : 1); ++b)
            grow_now = grow_now || im_neg_[b].size() < static_cast<size_t>(c.total) || (layout == 2 && im_neg_bits_[b].size() < words);
        if (grow_now) {
            if (pre_stream_) BFH_HIP(hipStreamSynchronize(pre_stream_));
            pre_valid_ = false;
            for (int b = 0; b < (ahead ? 2 : 1); ++b) {
                grow(im_neg_[b], static_cast<size_t>(c.total));
                if (layout == 2) grow(im_neg_bits_[b], words);
            }
        }
        int buf = 0;
        if (pre_valid_ && pre_key_ == want) {
            buf = pre_buf_;
            BFH_HIP(hipStreamWaitEvent(stream, pre_done_, 0));
        } else {
            if (pre_valid_) BFH_HIP(hipStreamSynchronize(pre_stream_));   // a stale speculation may still be writing the other buffer
            im_presample_launch(p, c, layout, 0, stream);
        }
        pre_valid_ = false;
        if (ahead) {
            if (!pre_stream_) {
                BFH_HIP(hipStreamCreateWithFlags(&pre_stream_, hipStreamNonBlocking));
                BFH_HIP(hipEventCreateWithFlags(&pre_done_, hipEventDisableTiming));
                BFH_HIP(hipEventCreateWithFlags(&pre_ready_, hipEventDisableTiming));
            }
            const int other = 1 - buf;
            SgdParams p2 = p;
            p2.epoch = p.epoch + 1;
            BFH_HIP(hipEventRecord(pre_ready_, stream));                   // the staged chunk (keys, row ids) and the regrouping are in place behind this point
            BFH_HIP(hipStreamWaitEvent(pre_stream_, pre_ready_, 0));
            im_presample_launch(p2, c, layout, other, pre_stream_);
            BFH_HIP(hipEventRecord(pre_done_, pre_stream_));
            pre_key_ = want;
            pre_key_.epoch = static_cast<int64_t>(p.epoch) + 1;
            pre_buf_ = other;
            pre_valid_ = true;
        }
        ImNegatives ng;
        if (layout == 2) { ng.bits = im_neg_bits_[buf].get(); ng.exc = im_neg_[buf].get(); }
        else ng.pre = im_neg_[buf].get();
        return ng;
    }
    // the queue descriptor from plan and buffers (the ticket range of a segment is set by im_run_segments); zeroes the done counter and the tickets
    ImQueues im_fill_queues(const BprConsts& c, const ImCall& k, const ImNegatives& ng) {
        ImQueues q{};
        q.ent_key = im_key_b_.get();
        q.ent_pos = im_pos_b_.get();
        q.ent_user = k.keeps ? im_ent_user_.get() : nullptr;
        q.nq = k.nq;
        for (int i = 0; i < 16; ++i) q.xcd_queue[i] = im_xcd_queue_[i];
        q.p_nt = im_p_nt_;
        q.study = im_study_;
        q.hot_user = im_hot_user_.get();
        q.rep_P = (k.p_rep || k.p_hyb) ? repP_.get() : nullptr;
        q.rep_pstride = static_cast<int64_t>(P_rows_) * vdim_;
        q.flush_every = im_flush_.get();
        q.strict = im_single_wave_;
        q.trace = (im_single_wave_ && im_trace_.size() >= static_cast<size_t>(c.total)) ? im_trace_.get() : nullptr;
        q.done = reinterpret_cast<unsigned long long*>(scratch_.get() + 1);
        q.neg_pre = ng.pre;
        q.neg_bits = ng.bits;
        q.neg_exc = ng.exc;
        BFH_HIP(hipMemsetAsync(scratch_.get() + 1, 0, sizeof(double), stream));
        q.slice_len = k.plan.slice_len;
        for (int x = 0; x < k.nq; ++x) {
            q.q_beg[x] = im_qbeg_[x];
            q.q_triples[x] = k.plan.q_triples[x];
            q.q_slices[x] = k.plan.q_slices[x];
            q.q_stride[x] = k.plan.q_stride[x];
        }
        im_tickets_.resize(static_cast<size_t>(k.plan.segments) * kImMaxQueues);
        BFH_HIP(hipMemsetAsync(im_tickets_.get(), 0, im_tickets_.bytes(), stream));
        return q;
    }
    // per merge segment: the walk (t_main_), then drain, the other ranks' deltas, the merges (one t_aux_ slot), then this segment's exchange
    void im_run_segments(const SgdParams& p, const BprConsts& c, ImQueues& q, const ImCall& k) {
        const int64_t segments = k.plan.segments;
        for (int64_t sgm = 0; sgm < segments; ++sgm) {
            int64_t seg_slices = 0;
            for (int x = 0; x < k.nq; ++x) {
                im_segment_tickets(k.plan, x, sgm, &q.t_beg[x], &q.t_end[x]);
                seg_slices += q.t_end[x] - q.t_beg[x];
            }
            q.tickets = im_tickets_.get() + sgm * kImMaxQueues;
            const int64_t grid_waves = std::max<int64_t>(4, std::min(k.waves, seg_slices));
            int slot = t_main_.begin(stream);
            if (!im_drain_only_ && !im_single_wave_) im_launch(p, c, q, k, grid_waves, false);
            t_main_.end(slot, stream);
            stats.launches += 1;
            slot = t_aux_.begin(stream);
            im_launch(p, c, q, k, grid_waves, true);
            // multi-GPU: the other ranks' deltas of the previous exchange point land in Q before the replicas are folded in and
            // refreshed; this segment's own delta goes out behind the merge and travels while the next walk runs
            exchange_finish(true);
            xcd_merge(sgm + 1 < segments, c.hot, true, k.w_items);
            if (k.p_rep || k.p_hyb) im_merge_users(k, sgm + 1 < segments);
            t_aux_.end(slot, stream);
            stats.merges += 1;
            if (has_comm()) {
                exchange_weights(static_cast<double>(seg_slices) * k.plan.slice_len, c.lr, num_neg_, uniform_);
                exchange_begin();
            }
        }
    }

    // one call of the item-major path over the staged chunk [start_x, next_x); `comm_points`: exchange points of the call under a communicator
    void launch_item_major(const SgdParams& p, BprConsts c, int start_x, int next_x, int64_t comm_points) {
        ImCall k = im_plan_call(p, c, start_x, next_x, comm_points);
        const int slot = t_aux_.begin(stream);
        im_regroup(p, k);
        im_plan_queues(c, k);
        count_positives(p, k.keeps ? csr_generation_ : -1, start_x, next_x);
        im_row_flags(p, k);
        im_merge_weights(p, c, k);
        im_replicas_begin(c, k);
        ImQueues q = im_fill_queues(c, k, im_draw_negatives(p, c, k));
        t_aux_.end(slot, stream);
        im_run_segments(p, c, q, k);
        im_expect_done_ = c.total;
    }
    // after the stream was synchronised: every triple must have been processed exactly once
    void im_check_done() {
        if (im_expect_done_ < 0) return;
        unsigned long long done = 0;
        BFH_HIP(hipMemcpy(&done, scratch_.get() + 1, sizeof(done), hipMemcpyDeviceToHost));
        const int64_t want = im_expect_done_;
        im_expect_done_ = -1;
        if (static_cast<int64_t>(done) != want)
            throw Error(BFH_ERR_HIP, "hogwild_atomic=3: " + std::to_string(done) + " of " + std::to_string(want) + " updates were processed");
    }

    // stream-ordered helpers of policy 2
    // `with_base`: a ninth copy keeps what the replicas started from (policy 3)
    void xcd_alloc(bool with_base) {
        const size_t copies = kXcdReplicas + (with_base ? 1 : 0);
        if (repQ_.size() < copies * Q_rows_ * vdim_) repQ_.resize(copies * Q_rows_ * vdim_);
        if (repQb_.size() < copies * rep_bstride()) repQb_.resize(copies * rep_bstride());
    }
    void xcd_broadcast(bool with_base) {
        const int64_t nq4 = static_cast<int64_t>(Q_rows_) * vdim_ / 4;
        const int copies = kXcdReplicas + (with_base ? 1 : 0);
        hipLaunchKernelGGL((xcd_broadcast_kernel<float4>), dim3(static_cast<unsigned>(std::min<int64_t>((nq4 + 255) / 256, 8192))), dim3(256), 0, stream,
                           reinterpret_cast<const float4*>(Q_.get()), reinterpret_cast<float4*>(repQ_.get()), nq4, nq4, copies);
        hipLaunchKernelGGL((xcd_broadcast_kernel<float>), dim3((Q_rows_ + 255) / 256), dim3(256), 0, stream,
                           static_cast<const float*>(Qb_.get()), repQb_.get(), static_cast<int64_t>(Q_rows_), rep_bstride(), copies);
        BFH_HIP(hipGetLastError());
    }
    void xcd_merge(bool write_replicas, const uint8_t* hot, bool with_base, bool weighted = false) {
        const int64_t nq4 = static_cast<int64_t>(Q_rows_) * vdim_ / 4;
        const float scale = xcd_merge_mean_ ? 1.0f / kXcdReplicas : 1.0f;
        float4* base4 = with_base ? reinterpret_cast<float4*>(repQ_.get()) + kXcdReplicas * nq4 : nullptr;
        float* baseb = with_base ? repQb_.get() + kXcdReplicas * rep_bstride() : nullptr;
        hipLaunchKernelGGL((xcd_merge_kernel<float4>), dim3(static_cast<unsigned>(std::min<int64_t>((nq4 + 255) / 256, 8192))), dim3(256), 0, stream,
                           reinterpret_cast<float4*>(Q_.get()), reinterpret_cast<float4*>(repQ_.get()), nq4, nq4, scale, write_replicas ? 1 : 0,
                           hot, vdim_ / 4, base4, 0, weighted ? xcd_wq_.get() : nullptr);
        hipLaunchKernelGGL((xcd_merge_kernel<float>), dim3((Q_rows_ + 255) / 256), dim3(256), 0, stream, Qb_.get(), repQb_.get(),
                           static_cast<int64_t>(Q_rows_), rep_bstride(), scale, write_replicas ? 1 : 0, hot, 1, baseb, 0, weighted ? xcd_wb_.get() : nullptr);
        BFH_HIP(hipGetLastError());
    }
    // hot-row flags for this call (policy 2); returns null when the split is disabled
    template <bool INJECT>
    const uint8_t* xcd_hot_rows(const SgdParams& p, const BprConsts& c, int64_t seg_work) {
        if (xcd_hot_tau_ <= 0) return nullptr;
        hot_.resize(static_cast<size_t>(Q_rows_));
        double pos_mult = num_neg_, triples = static_cast<double>(c.total), neg_uniform = uniform_ ? 1.0 / Q_rows_ : 0.0;
        const int64_t* cum = (!INJECT && !uniform_) ? p.cum_table : nullptr;
        if (INJECT) {
            itemcnt_kept(-1, -1, -1);
            count_items(c.inj_p, c.total);
            count_items(c.inj_n, c.total);
            pos_mult = 1.0;
            neg_uniform = 0.0;
        } else {
            count_positives(p, -1, -1, -1);   // this policy never reuses a chunk's histogram
            if (resident_) triples = static_cast<double>(resident_nnz_) * num_neg_;
        }
        const double waves = static_cast<double>(std::min<int64_t>(resident_waves(reinterpret_cast<const void*>(pick<INJECT>(c))), seg_work));
        const double inflight = 2.0 * waves / kXcdReplicas;     // a wave holds the two item rows of its next triple
        hipLaunchKernelGGL(xcd_hot_kernel, dim3((Q_rows_ + 255) / 256), dim3(256), 0, stream, itemcnt_.get(), cum, cum_total_, Q_rows_, pos_mult,
                           triples, neg_uniform, inflight, xcd_hot_tau_ * 1e-3, hot_.get());
        BFH_HIP(hipGetLastError());
        return hot_.get();
    }
    int64_t rep_bstride() const { return (static_cast<int64_t>(Q_rows_) + 63) / 64 * 64; }

    template <bool INJECT>
    void launch(const SgdParams& p, const BprConsts& c_in, int start_x = 0, int next_x = 0) {
        BprConsts c = c_in;
        const int64_t n_work = (c.total + c.chunk - 1) / c.chunk;
        const bool reps = c.atomic == 2;
        // adam / adagrad: P, Q are frozen, so the item-side gradients are summed by the sorted gather (no per-triple atomics)
        const bool two_pass = !INJECT && optimizer_ != "sgd" && accum_two_pass_ != 0;
        if (two_pass) {
            acc_prepare(c.total);
            c.two_pass = 1;
            c.uc_out = gather_.uc();
            c.neg_out = gather_.neg();
        }
        int64_t seg_work = n_work;          // work items per launch
        if (reps) {
            xcd_alloc(false);
            c.rep_Q = repQ_.get();
            c.rep_Qb = repQb_.get();
            c.rep_stride = static_cast<int64_t>(Q_rows_) * vdim_;
            c.rep_bstride = rep_bstride();
            // a segment is a whole number of work items per resident wave: it ends when its slowest wave does
            const int64_t waves = resident_waves(reinterpret_cast<const void*>(pick<INJECT>(c)));
            const int64_t sync_updates = xcd_sync_updates_ > 0 ? xcd_sync_updates_ : int64_t(1) << 21;
            seg_work = std::max<int64_t>(1, (sync_updates / c.chunk + waves / 2) / waves) * waves;
            const int slot = t_aux_.begin(stream);
            c.hot = xcd_hot_rows<INJECT>(p, c, std::min(seg_work, n_work));
            xcd_broadcast(false);
            t_aux_.end(slot, stream);
        }
        for (int64_t w0 = 0; w0 < n_work; w0 += seg_work) {
            c.work_begin = w0;
            c.work_end = std::min(n_work, w0 + seg_work);
            launch_segment<INJECT>(p, c);
            if (reps) {
                const int slot = t_aux_.begin(stream);
                xcd_merge(c.work_end < n_work, c.hot, false);
                t_aux_.end(slot, stream);
                stats.merges += 1;
            }
        }
        if (two_pass) {
            const int slot = t_aux_.begin(stream);
            acc_build_positive_list(p, start_x, next_x);
            const float sab_pos[3] = {1.f, 0.f, 0.f}, sab_neg[3] = {-1.f, 0.f, 0.f};
            acc_gather(p, num_neg_, update_i_, update_j_, sab_pos, sab_neg, use_bias_);
            t_aux_.end(slot, stream);
        }
    }

    template <bool INJECT>
    void launch_segment(const SgdParams& p, const BprConsts& c) {
        const int64_t n_work = c.work_end - c.work_begin;
        const KernelFn fn = pick<INJECT>(c);
        dim3 block(256), grid(1);
        if (sequential_) {
            block = dim3(64);
        } else {
            int64_t waves = resident_waves(reinterpret_cast<const void*>(fn));
            if (waves > n_work) waves = n_work;
            grid = dim3(static_cast<unsigned>((waves + 3) / 4));
        }
        const int slot = t_main_.begin(stream);
        hipLaunchKernelGGL(fn, grid, block, 0, stream, p, c);
        BFH_HIP(hipGetLastError());
        t_main_.end(slot, stream);
        stats.launches += 1;
    }

    // exchange points of one partial_update call: every rank must enter the SAME number of collectives ("comm_segments"; 0 = one, blocking)
    int64_t comm_points() const { return comm_segments_ > 0 ? comm_segments_ : 1; }
    // k exchange points this rank enters with a zero delta (no local work since the last begin: Q <- Z exactly)
    void exchange_idle_points(int64_t k, double lr) {
        for (; k > 0; --k) {
            exchange_finish();
            exchange_weights(0.0, lr, num_neg_, uniform_);
            exchange_begin();
        }
    }

    void partial_update(int start_x, int next_x, const int64_t* indptr, const int32_t* keys, double* loss_sum, double* n_samples) {
        SgdParams p;
        const int64_t n = stage_chunk(start_x, next_x, indptr, keys, &p);
        *loss_sum = 0.0;
        *n_samples = static_cast<double>(n) * num_neg_;
        if (has_comm()) exchange_arm();   // Z = the replicated state (sgd: Q | Qb, else the gradient buffers) before this rank changes it
        if (n == 0) {
            // an empty chunk of this rank's shard: nothing to walk, but every exchange point of the call is a collective the
            // other ranks enter -- take part with a zero delta
            if (has_comm() && optimizer_ == "sgd") {
                exchange_histogram(resident_ ? keys_.get() : p.keys, resident_ ? resident_nnz_ : 0);
                exchange_idle_points(comm_points(), current_lr());
                if (!comm_overlap_ || comm_points() == 1) exchange_finish();
                sync_stream();
            }
            return;
        }
        BFH_REQUIRE(uniform_ || have_cum_, "sampling_power != 0 needs set_cumulative_table");
        BFH_REQUIRE(uniform_ || cum_total_ > 0, "cumulative table is empty");
        BprConsts c = consts(current_lr());
        c.total = n * num_neg_;
        if (compute_loss_) BFH_HIP(hipMemsetAsync(scratch_.get(), 0, sizeof(double), stream));
        if (has_comm() && optimizer_ == "sgd") {
            // the popularity every rank weighs its rows by: the resident matrix when there is one, else this call's chunk
            exchange_histogram(resident_ ? keys_.get() : p.keys, resident_ ? resident_nnz_ : n);
        }
        if (c.atomic == 3 && !im_fits(c, n)) c.atomic = 1;   // 32-bit sort key / entry index exhausted: the user-major atomic walk
        if (c.atomic == 3) {
            launch_item_major(p, c, start_x, next_x, comm_points());
        } else {
            if (optimizer_ == "sgd") exchange_finish();
            launch<false>(p, c, start_x, next_x);
            if (has_comm() && optimizer_ == "sgd") {
                // the user-major walks make one exchange point per call; with "comm_segments" = k every rank must still enter k
                // collectives (a rank whose chunk does not fit the item-major plan lands here while the others cut theirs)
                exchange_weights(static_cast<double>(c.total), c.lr, num_neg_, uniform_);
                exchange_begin();
                exchange_idle_points(comm_points() - 1, c.lr);
            }
        }
        // a call of one exchange point is blocking: its exchange is finished before it returns
        if (has_comm() && (!comm_overlap_ || comm_points() == 1)) exchange_finish();
        if (compute_loss_) BFH_HIP(hipMemcpyAsync(loss_sum, scratch_.get(), sizeof(double), hipMemcpyDeviceToHost, stream));
        sync_stream();
        im_check_done();
        harvest_timers();
        stats.samples += c.total;
        advance_progress(start_x, next_x, indptr);
    }

    void update_triples(int64_t n, const int32_t* users, const int32_t* pos, const int32_t* neg, double lr) {
        BFH_REQUIRE(model_on_gpu_, "update_triples before initialize_model(..., set_gpu=True)");
        if (n <= 0) return;
        exchange_finish();
        const int32_t* inj = upload_triples(n, users, pos, neg);
        SgdParams p{};
        p.P = P_.get(); p.Q = Q_.get(); p.Qb = Qb_.get();
        p.gradP = gradP_.get(); p.gradQ = gradQ_.get(); p.gradQb = gradQb_.get();
        p.cntP = cntP_.get(); p.cntQ = cntQ_.get();
        p.P_rows = P_rows_; p.Q_rows = Q_rows_; p.d = d_; p.vdim = vdim_;
        BprConsts c = consts(lr);
        if (c.atomic == 3) c.atomic = 1;   // injected triples have no CSR to regroup: atomics
        c.compute_loss = 0;
        c.num_neg = 1;
        c.total = n;
        c.inj_u = inj; c.inj_p = inj + n; c.inj_n = inj + 2 * n;
        launch<true>(p, c);
        sync_stream();
        harvest_timers();
        stats.samples += n;
    }

    double compute_loss(int n, const int32_t* users, const int32_t* pos, const int32_t* neg) {
        BFH_REQUIRE(model_on_gpu_, "compute_loss before initialize_model(..., set_gpu=True)");
        if (n <= 0) return 0.0;  // the reference divides by zero here (bpr.cc:243); callers guard (bpr.py:141)
        exchange_finish();
        const int32_t* inj = upload_triples(n, users, pos, neg);
        BFH_HIP(hipMemsetAsync(scratch_.get(), 0, sizeof(double), stream));
        const int slot = t_aux_.begin(stream);
        hipLaunchKernelGGL(bpr_loss_kernel, dim3((n + 3) / 4), dim3(256), 0, stream, P_.get(), Q_.get(), Qb_.get(), inj,
                           inj + n, inj + 2 * n, n, vdim_, static_cast<int>(use_bias_), scratch_.get());
        BFH_HIP(hipGetLastError());
        t_aux_.end(slot, stream);
        double l = 0.0;
        BFH_HIP(hipMemcpyAsync(&l, scratch_.get(), sizeof(double), hipMemcpyDeviceToHost, stream));
        sync_stream();
        harvest_timers();
        return l / static_cast<double>(n);
    }

    int num_neg_ = 1;
    bool verify_neg_ = true, uniform_ = true;
    // knobs of policies 2 / 3 (set_mode)
    // policy 2 (BPRMF sgd): updates between two merges of the per-XCD item-factor replicas, and
    // whether the merge sums (0) or averages (1) the replicas' deltas
    int64_t xcd_sync_updates_ = -1;   // default: 2^21 (policy 2), 2^23 (policy 3)
    int xcd_merge_mean_ = 0;
    // policy 3: curvature (permille) the merge's per-row saturation weights assume for Q / Qb / the replicated P rows (xcd_item_weight_kernel); 0 = plain sum.
    // Biases: 250 = the logistic loss's own curvature bound (1/4), the constant the multi-GPU exchange uses ("comm_stiffness").  Measured at
    // BASELINE scale against the threaded oracle pair (profiles/r04_bpr_merge_weights_study.txt): at the reference's lr |Qb| 93.04 -> 91.93 (oracles
    // 90.21 / 92.06), sampled loss 0.2075 -> 0.2081 (oracles 0.2075 / 0.2084), kernel time unchanged; the factor rows sit far below saturation there
    // (a weight on Q moves |Q| AWAY from the oracles, one on the replicated P rows changes nothing), and at lr 0.05 the drift rule has the item
    // rows chip-wide, so no weight reaches them.
    int xcd_stiff_q_milli_ = 0, xcd_stiff_b_milli_ = 250, xcd_stiff_p_milli_ = 0;
    // the learning rate (in units of 1e-6) the stiffness constants were calibrated at: above it they shrink like lr_ref / lr, i.e. the saturation
    // argument x = lr k m stops growing with the learning rate (0: the constants apply at every lr -- the form up to round 5, which damped the
    // negatives' bias steps to 0.36 of their sum at lr 0.035 and left |Qb| 19 % low on the reference benchmark's schedule: profiles/r06_bpr_lr005_*)
    // Measured (profiles/r06_bpr_lr005_stiffness_rule.txt): refbench |Qb| 147.7 (off) / 159.6 (5000) / 171.6 (2000) / 176.1 (1000) / 180.8 (no weight at all) against 183.0;
    // the bench case (lr 0.002) 91.93 / 91.93 / 91.93 / 92.34 / 93.04 against oracle pairs 90.2 .. 92.8 on four boxes -- 1000 sits inside every pair's band.
    int xcd_stiff_lr_ref_micro_ = 1000;
    // learning rate (permille) up to which users get per-XCD replicas.  Above it (study at lr 0.05): plain sums end at |Qb| 109 against the oracles'
    // 91.6; with xcd_stiff_p = 50 |P| 424 / |Qb| 95.5 against 428.7 / 94.8 for the owner form (oracle 430.6 / 91.6) for 6 % of the walk -- not taken.
    int im_user_lr_max_milli_ = 10;
    DevBuf<float> xcd_wq_, xcd_wb_, xcd_wp_;
    int im_single_wave_ = 0, im_force_queues_ = 0;   // test hooks: one wave drains all queues in order; number of queues for that run
    int im_drain_only_ = 0;        // test hook: skip the owner-XCD launch, the atomic drain launch does everything
    DevBuf<int32_t> im_trace_;     // test hook ("im_trace" = capacity): table index of every triple of a single-wave call
    int im_drift_budget_milli_ = 1000;  // policy 3: lr-weighted positive steps of a row per merge interval above which its negatives go chip-wide
    int im_presample_ = 2;         // policy 3: draw the call's negatives in CSR order before the walk: 1 = all of them, at their nnz positions;
                                   // 2 = only the rejected first draws, in walk order (uniform sampling, kept chunks; else 1): im_draw_negatives
    int im_presample_ahead_ = 1;   // ... and the next epoch's on a side stream while this epoch's walk runs
    int im_blocks_ = 0;            // policy 3: runs an item's entries are cut into inside a queue (0 = from the learning rate)
    int im_dual_ = -1;             // policy 3: two triples per wave at vdim <= 128 (bpr_item_major_dual_kernel); -1: from 1024 users per queue up (6144 until round 6), 1: always, 0: never
    int im_neg_limit_ = 0;         // policy 3 study knob: fold the uniform negatives into the first rows of Q
    bool im_dual_generic_ = false; // "im_dual_generic": the two-triples walk with per-lane guards at every vdim (A/B against the whole-group instantiations)
    int im_study_ = 0;             // policy 3 measurement knob (never set by a front): bit 0 drops the chip-wide atomics of the negatives' rows (profiles/r06_bpr_lr005_*)
    int im_p_nt_ = 0;              // policy 3 study knob: non-temporal hint on the per-triple P rows
    int im_user_replicas_ = -1;    // policy 3: per-XCD replicas of P instead of one owner XCD per user (-1: for small shards, 0 / 1)
    int im_user_hybrid_ = 2;       // policy 3, whole matrices: per-XCD replicas of P for the HEAVY users only (the ones the collision rule would put on
                                   // atomics): 1 = their entries over all queues, 2 = over as few neighbouring queues as bring the share under the threshold
    int im_built_spread_mode_ = 0; // what the cached item-major keys were built with: 0 owner queues, 1 every entry spread, 2 heavy users' entries spread
    int64_t im_built_heavy_deg_ = 0;
    int im_max_stale_ = 16;        // policy 3: updates of one item row that may be in flight unseen by the other waves (at lr 0.05; x 0.05 / lr)
                                   // 16: |P| within 0.1 % of the threaded oracle's after 24 epochs at lr 0.05 (64: -1.1 %), no cost at lr 0.002
    int xcd_fresh_ = -1, xcd_v4_ = 0;  // re-read before store; float4-per-lane rows (hot-row atomics then cost 4x the line operations)
    int xcd_hot_tau_ = 100;        // permille: tolerated collision probability of a replica row (0 = no hot rows)
    DevBuf<float> exp_table_;
    DevBuf<float> repQ_, repQb_;   // policy 2: [8][Q_rows][vdim], [8][ceil64(Q_rows)]
    DevBuf<float> repP_;           // policy 3 on small shards: [8 + 1][P_rows][vdim]
    DevBuf<int> itemcnt_;          // policy 2: updates per item row (popularity)
    DevBuf<uint8_t> hot_;
    int64_t itemcnt_gen_ = -1;
    int itemcnt_start_ = -1, itemcnt_next_ = -1;
    std::map<const void*, int> occupancy_;   // kernel -> resident 256-thread blocks per CU
    // policy 3
    int im_nq_ = 0, im_xcd_queue_[16];
    DevBuf<uint32_t> im_key_a_, im_key_b_;
    DevBuf<int32_t> im_pos_a_, im_pos_b_;
    DevBuf<char> im_tmp_;
    DevBuf<int64_t> im_qbeg_dev_;
    DevBuf<uint8_t> im_flush_, im_hot_user_;
    DevBuf<int> im_tickets_;
    DevBuf<int32_t> im_ent_user_, im_ent_inv_;   // user of every sorted entry; place of every nnz position in the sort (kept chunks)
    int64_t im_regroup_id_ = 0;    // counts the regroupings built: what a walk-order draw was written against
    DevBuf<int32_t> im_neg_[2];    // pre-drawn negatives (layout 1) or exceptions (layout 2): this call's, and the speculation for the next epoch
    DevBuf<uint32_t> im_neg_bits_[2];   // layout 2: one bit per triple
    struct PreKey {
        int64_t epoch;
        int start_x, next_x;
        int64_t total, gen, nnz_offset, shift, seed;
        int flags;
        int64_t cum_total;
        int layout;                // 1: CSR order, 2: walk order
        int64_t regroup;           // layout 2: im_regroup_id_ of the sort the draw was written against (0 otherwise)
        bool operator==(const PreKey& o) const {
            return epoch == o.epoch && start_x == o.start_x && next_x == o.next_x && total == o.total && gen == o.gen && nnz_offset == o.nnz_offset &&
                   shift == o.shift && seed == o.seed && flags == o.flags && cum_total == o.cum_total && layout == o.layout && regroup == o.regroup;
        }
    };
    PreKey pre_key_{};
    bool pre_valid_ = false;
    int pre_buf_ = 0;
    hipStream_t pre_stream_ = nullptr;
    hipEvent_t pre_done_ = nullptr, pre_ready_ = nullptr;
    int64_t im_qbeg_[kImMaxQueues + 1] = {0};
    int64_t im_gen_ = -1, im_n_ = -1, im_expect_done_ = -1, im_built_blocks_ = -1;
    int im_built_nq_ = -1;
    int im_start_ = -1, im_next_ = -1;
};

}  // namespace bfh

using bfh::BprHandle;

extern "C" {

BFH_ABI_SGD(bpr, BprHandle)

int bfh_bpr_update_triples(void* h, int64_t n, const int32_t* users, const int32_t* positives, const int32_t* negatives, double lr) {
    return bfh::guarded<BprHandle>(h, [&](BprHandle& x) { x.update_triples(n, users, positives, negatives, lr); });
}
int bfh_bpr_item_major_plan(int num_queues, const int64_t* queue_entries, int num_negative_samples, int64_t sync_updates, int* slice_len,
                            int64_t* segments, int64_t* queue_slices, int64_t* queue_stride) {
    if (num_queues < 1 || num_queues > bfh::kImMaxQueues || !queue_entries || num_negative_samples < 1 || !slice_len || !segments ||
        !queue_slices || !queue_stride)
        return BFH_ERR_INVALID;
    const bfh::ImPlan pl = bfh::im_make_plan(num_queues, queue_entries, num_negative_samples, sync_updates);
    *slice_len = pl.slice_len;
    *segments = pl.segments;
    for (int x = 0; x < num_queues; ++x) {
        queue_slices[x] = pl.q_slices[x];
        queue_stride[x] = pl.q_stride[x];
    }
    return BFH_OK;
}

}  // extern "C"
