// The host side of the SGD base shared by the BPRMF and WARP backends, in its parts: the two-pass gradient gather, the exchange
// between ranks, and SgdHandle -- the device-resident model, the staging of chunks with the lr schedule, the epoch-end optimizer
// step.  The kernels are in sgd_kernels.hpp.
#include "sgd_kernels.hpp"

#include <algorithm>

#include "comm.hpp"

namespace bfh {

// ------------------------------------------------------------------------------------------------
// TwoPassGather (sgd_base.hpp)
// ------------------------------------------------------------------------------------------------
void TwoPassGather::prepare(int64_t triples, hipStream_t s) {
    const size_t n = static_cast<size_t>(triples);
    grow(uc_, n); grow(neg_, n);
    grow(nkey_, n); grow(nidx_, n);
    if (iota_n_ < triples) {
        iota_.resize(n);
        launch_incidence_iota(triples, iota_.get(), s);
        iota_n_ = triples;
    }
}

void TwoPassGather::build_positive_list(const SgdParams& p, int start_x, int next_x, int64_t generation, hipStream_t s) {
    const int64_t n = p.chunk_nnz;
    BFH_REQUIRE(n < (int64_t(1) << 31), "gradient gather: chunk of 2^31 or more interactions");
    if (generation >= 0 && pos_gen_ == generation && pos_start_ == start_x && pos_next_ == next_x && pos_n_ == n) return;
    grow(pkey_, static_cast<size_t>(n)); grow(pidx_, static_cast<size_t>(n));
    // the chunk's keys are the sort keys as they are (item ids are non-negative int32)
    device_sort_pairs_u32(reinterpret_cast<const uint32_t*>(p.keys), pkey_.get(), iota_.get(), pidx_.get(), n, bits_for(p.Q_rows), tmp_, s);
    pos_gen_ = generation;
    pos_start_ = start_x; pos_next_ = next_x; pos_n_ = n;
}

void TwoPassGather::gather(const SgdParams& p, int num_neg, bool do_pos, bool do_neg, const float sab_pos[3], const float sab_neg[3], float* gradQb,
                           int* cntQ, int64_t max_waves, hipStream_t s) {
    const int64_t n = p.chunk_nnz, triples = n * num_neg;
    GatherParams g{};
    g.uc = uc_.get();
    g.P = p.P; g.Q = p.Q;
    g.gradQ = p.gradQ;
    g.gradQb = gradQb;
    g.cntQ = cntQ;
    g.num_neg = num_neg; g.vdim = p.vdim; g.Q_rows = p.Q_rows;
    if (do_pos) {
        g.inc_key = pkey_.get(); g.inc_idx = pidx_.get(); g.n = n; g.pos_list = 1;
        g.sign = sab_pos[0]; g.a = sab_pos[1]; g.b = sab_pos[2];
        launch_grad_gather(g, max_waves, s);
    } else if (cntQ) {
        launch_incidence_count(reinterpret_cast<const uint32_t*>(p.keys), n, p.Q_rows, cntQ, s);
    }
    if (!do_neg && cntQ) launch_incidence_count(neg_.get(), triples, p.Q_rows, cntQ, s);
    if (do_neg) {
        device_sort_pairs_u32(neg_.get(), nkey_.get(), iota_.get(), nidx_.get(), triples, bits_for(static_cast<int64_t>(p.Q_rows) + 1), tmp_, s);
        g.inc_key = nkey_.get(); g.inc_idx = nidx_.get(); g.n = triples; g.pos_list = 0;
        g.sign = sab_neg[0]; g.a = sab_neg[1]; g.b = sab_neg[2];
        launch_grad_gather(g, max_waves, s);
    }
}

void SgdHandle::acc_gather(const SgdParams& p, int num_neg, bool do_pos, bool do_neg, const float sab_pos[3], const float sab_neg[3], bool with_bias) {
    // a streaming gather: 26-67 VGPRs leave room for 8 waves per SIMD, and latency hiding is all this kernel needs
    const int64_t waves = static_cast<int64_t>(num_cus_) * (gather_waves_per_cu_ > 0 ? gather_waves_per_cu_ : 32);
    gather_.gather(p, num_neg, do_pos, do_neg, sab_pos, sab_neg, with_bias ? p.gradQb : nullptr, pcn_ ? p.cntQ : nullptr, waves, stream);
}

// ------------------------------------------------------------------------------------------------
// RankExchange (sgd_exchange.hpp)
// ------------------------------------------------------------------------------------------------
// One step over the matrix segment of the pair and then over its bias segment, which lies behind it in the exchange buffers:
// fn(segment, its offset in Z / S / R, its elements, is it the bias)
template <typename F>
static void over_segments(const ReplicatedPair& q, F&& fn) {
    const size_t nq = static_cast<size_t>(q.rows) * q.vdim;
    fn(q.X, size_t(0), static_cast<int64_t>(nq), false);
    fn(q.Xb, nq, static_cast<int64_t>(q.rows), true);
}

RankExchange::~RankExchange() {
    if (pending_ && done_) (void)hipEventSynchronize(done_);
    if (ready_) (void)hipEventDestroy(ready_);
    if (done_) (void)hipEventDestroy(done_);
}

void RankExchange::set_comm(Comm* c, int device) {
    comm_ = c;
    armed_ = false;
    if (c) {
        BFH_REQUIRE(c->device == device, "set_comm: the communicator lives on another device than this handle");
        if (!ready_) BFH_HIP(hipEventCreateWithFlags(&ready_, hipEventDisableTiming));
        if (!done_) BFH_HIP(hipEventCreateWithFlags(&done_, hipEventDisableTiming));
    }
}

void RankExchange::reset() {
    if (pending_ && done_) (void)hipEventSynchronize(done_);
    pending_ = false;
    armed_ = false;
}

void RankExchange::capture(const ReplicatedPair& q) {
    over_segments(q, [&](const float* x, size_t off, int64_t n, bool) {
        BFH_HIP(hipMemcpyAsync(Z_.get() + off, x, static_cast<size_t>(n) * sizeof(float), hipMemcpyDeviceToDevice, q.stream));
    });
}

void RankExchange::publish(const ReplicatedPair& q) {
    over_segments(q, [&](const float* x, size_t off, int64_t n, bool) {
        hipLaunchKernelGGL(delta_begin_kernel, stream_grid(n), dim3(256), 0, q.stream, x, Z_.get() + off, S_.get() + off, n);
    });
}

// Called before the first local change of a model (initialize_model uploaded the same Q / Qb on every rank; the gradient buffers
// start at zero), so Z is identical on every rank.
void RankExchange::arm(const ReplicatedPair& q, bool weighted) {
    if (!comm_ || armed_) return;
    const size_t n = count(q), rows = static_cast<size_t>(q.rows);
    if (Z_.size() < n) { Z_.resize(n, true, q.stream); S_.resize(n, true, q.stream); R_.resize(n, true, q.stream); }
    capture(q);
    if (weighted) {
        // per-row combination weights (1 until `finish` computes them) and the popularity of every item over ALL ranks
        W_.resize(rows);
        Wb_.resize(rows);
        std::vector<float> ones(rows, 1.0f);
        BFH_HIP(hipMemcpyAsync(W_.get(), ones.data(), ones.size() * sizeof(float), hipMemcpyHostToDevice, q.stream));
        BFH_HIP(hipMemcpyAsync(Wb_.get(), ones.data(), ones.size() * sizeof(float), hipMemcpyHostToDevice, q.stream));
        BFH_HIP(hipStreamSynchronize(q.stream));
        gcnt_ready_ = false;
    }
    armed_ = true;
    pending_ = false;
}

// Global item popularity (positives per item over every rank's shard) from this rank's keys: one int all-reduce, once per model.
void RankExchange::histogram(const ReplicatedPair& q, const int32_t* keys, int64_t n) {
    if (!comm_ || gcnt_ready_) return;
    gcnt_.resize(static_cast<size_t>(q.rows), true, q.stream);
    launch_incidence_count(reinterpret_cast<const uint32_t*>(keys), n, q.rows, gcnt_.get(), q.stream);
    comm_->all_reduce_i32(gcnt_.get(), gcnt_.get(), static_cast<size_t>(q.rows), q.stream);
    BFH_HIP(hipStreamSynchronize(q.stream));
    double tot[1] = {static_cast<double>(n)};
    if (comm_->size() > 1) {
        DevBuf<double> d;
        d.resize(1);
        BFH_HIP(hipMemcpyAsync(d.get(), tot, sizeof(double), hipMemcpyHostToDevice, q.stream));
        comm_->all_reduce_f64(d.get(), d.get(), 1, q.stream);
        BFH_HIP(hipMemcpyAsync(tot, d.get(), sizeof(double), hipMemcpyDeviceToHost, q.stream));
        BFH_HIP(hipStreamSynchronize(q.stream));
    }
    gcnt_total_ = tot[0];
    gcnt_ready_ = true;
}

// what the exchange that begins next covers: `interval_triples` = this rank's triples inside it, `lr` = its learning rate.
// The weights themselves are computed in `finish` from the sums over the ranks (exchange_weight_kernel).
void RankExchange::weights(double interval_triples, double lr, int num_neg, bool uniform) {
    w_interval_ = interval_triples;
    w_lr_ = lr;
    w_num_neg_ = num_neg;
    w_uniform_ = uniform;
}

// the pair -> S, one all-reduce on the communicator's stream behind everything issued on the pair's stream so far
void RankExchange::begin(const ReplicatedPair& q, bfh_stats& stats) {
    if (!comm_ || comm_->size() < 1) return;
    BFH_REQUIRE(armed_, "exchange_begin before exchange_arm");
    const int xk = t_xk_.begin(q.stream);
    publish(q);
    hipLaunchKernelGGL(exchange_scalars_kernel, dim3(1), dim3(1), 0, q.stream, S_.get() + scalars_at(q), static_cast<float>(w_interval_),
                       static_cast<float>(w_lr_));
    BFH_HIP(hipGetLastError());
    t_xk_.end(xk, q.stream);
    BFH_HIP(hipEventRecord(ready_, q.stream));
    BFH_HIP(hipStreamWaitEvent(comm_->comm_stream(), ready_, 0));
    const int ar = t_ar_.begin(comm_->comm_stream());
    comm_->all_reduce_f32(S_.get(), R_.get(), count(q), comm_->comm_stream());
    t_ar_.end(ar, comm_->comm_stream());
    BFH_HIP(hipEventRecord(done_, comm_->comm_stream()));
    p_num_neg_ = w_num_neg_;   // what `finish` weighs THIS exchange with (`weights` may be called for a later one meanwhile)
    p_uniform_ = w_uniform_;
    pending_ = true;
    stats.exchanges += 1;
}

void RankExchange::finish(const ReplicatedPair& q, bool progressed, int64_t num_nnz, const int64_t* cum, int64_t cum_total) {
    if (!pending_) return;
    BFH_HIP(hipStreamWaitEvent(q.stream, done_, 0));
    const int xk = t_xk_.begin(q.stream);
    if (gcnt_ready_) {
        const double glob_triples = static_cast<double>(num_nnz) * p_num_neg_;          // one epoch over all ranks
        const double pos_scale = gcnt_total_ > 0 ? static_cast<double>(num_nnz) / gcnt_total_ * p_num_neg_ : 0.0;   // counted keys -> the whole matrix
        hipLaunchKernelGGL(exchange_weight_kernel, dim3(blocks_of(q.rows)), dim3(256), 0, q.stream, gcnt_.get(), p_uniform_ ? nullptr : cum, cum_total,
                           q.rows, pos_scale, glob_triples, p_uniform_ ? 1.0 / q.rows : 0.0, R_.get() + scalars_at(q), stiffness_q_milli_ * 1e-3,
                           stiffness_milli_ * 1e-3, comm_->size(), W_.get(), Wb_.get());
    }
    over_segments(q, [&](float* x, size_t off, int64_t n, bool bias) {
        hipLaunchKernelGGL(delta_finish_kernel, stream_grid(n), dim3(256), 0, q.stream, x, Z_.get() + off, S_.get() + off, R_.get() + off,
                           bias ? Wb_.get() : W_.get(), bias ? 1 : q.vdim, n, progressed ? 1 : 0);
    });
    BFH_HIP(hipGetLastError());
    t_xk_.end(xk, q.stream);
    pending_ = false;
}

// sum what every rank accumulated into the pair (| counts) since the last optimizer step
void RankExchange::gradients(const ReplicatedPair& g, int* counts, bfh_stats& stats) {
    if (!comm_) return;
    int xk = t_xk_.begin(g.stream);
    // Z holds the residue the gradient buffers kept after the last step (Q-6: they are never re-zeroed); zero before the first
    publish(g);
    BFH_HIP(hipGetLastError());
    t_xk_.end(xk, g.stream);
    const int ar = t_ar_.begin(g.stream);
    comm_->group_start();
    comm_->all_reduce_f32(S_.get(), R_.get(), static_cast<size_t>(g.rows) * g.vdim + static_cast<size_t>(g.rows), g.stream);
    if (counts) comm_->all_reduce_i32(counts, counts, static_cast<size_t>(g.rows), g.stream);
    comm_->group_end();
    t_ar_.end(ar, g.stream);
    xk = t_xk_.begin(g.stream);
    over_segments(g, [&](float* x, size_t off, int64_t n, bool) {
        hipLaunchKernelGGL(delta_apply_kernel, stream_grid(n), dim3(256), 0, g.stream, x, Z_.get() + off, R_.get() + off, n);
    });
    BFH_HIP(hipGetLastError());
    t_xk_.end(xk, g.stream);
    stats.exchanges += 1;
}

// what the gradient buffers keep after the step (Q-6) is the base of the next delta
void RankExchange::rebase(const ReplicatedPair& g) {
    if (comm_ && armed_) capture(g);
}

void RankExchange::drain_timers(bfh_stats& stats) {
    stats.exchange_kernel_ms += t_xk_.drain();
    stats.allreduce_ms += t_ar_.drain();
}

// ---- SgdHandle's forwarding methods: which pair, and what of the handle a call reads ----
void SgdHandle::set_comm(Comm* c) {
    exchange_finish();
    exchange_.set_comm(c, device);
}

void SgdHandle::exchange_begin() {
    if (!has_comm() || !model_on_gpu_) return;
    exchange_finish(true);
    BFH_REQUIRE(hogwild(), "exchange_begin is the Hogwild (sgd) exchange");
    exchange_.begin(model_pair(), stats);
}

void SgdHandle::exchange_finish(bool progressed) { exchange_.finish(model_pair(), progressed, num_nnz_, cum_.get(), cum_total_); }

void SgdHandle::finish_for_reader() {
    if (!exchange_.pending()) return;
    exchange_finish();
    sync_stream();
}

// ------------------------------------------------------------------------------------------------
// SgdHandle: the model -- options, host binding, pinning, copy-back
// ------------------------------------------------------------------------------------------------
void SgdHandle::unpin_host() {
    // nothing of this handle may still be writing into a page-locked array when its registration goes (every entry point synchronises
    // before it returns, so this costs nothing; it is the belt to that pair of braces)
    if (!pinned_.empty() && stream) (void)hipStreamSynchronize(stream);
    for (auto& p : pinned_) (void)hipHostUnregister(p.first);
    if (!pinned_.empty()) (void)hipGetLastError();   // an array that was freed while pinned must not leave a sticky error behind
    pinned_.clear();
}

SgdHandle::~SgdHandle() {
    if (host_stale_ && model_on_gpu_ && hostP_) {   // lazy_sync: the deferred copy-back happens at the latest here
        try { synchronize(true, true); } catch (...) {}
    }
    unpin_host();
    if (stream) (void)hipStreamDestroy(stream);
}

bool SgdHandle::init(const char* opt_path) {
    std::string err;
    if (!opt_.load(opt_path ? opt_path : "", &err)) {
        last_error = err;
        return false;
    }
    BFH_HIP(hipSetDevice(device));
    if (!stream) BFH_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    hipDeviceProp_t prop;
    BFH_HIP(hipGetDeviceProperties(&prop, device));
    num_cus_ = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;

    d_ = opt_.integer("d");
    BFH_REQUIRE(d_ > 0, "option d must be positive");
    vdim_ = vdim_of(d_);
    BFH_REQUIRE(vdim_ <= 1024, "d > 1024 is not supported by the gfx950 kernels yet");
    num_iters_ = opt_.integer("num_iters");
    optimizer_ = opt_.str("optimizer");
    BFH_REQUIRE(optimizer_ == "sgd" || optimizer_ == "adam" || optimizer_ == "adagrad",
                "optimizer must be one of sgd, adam, adagrad");
    lr_ = opt_.num("lr");
    min_lr_ = opt_.num_or("min_lr", lr_);
    beta1_ = opt_.num_or("beta1", 0.9);
    reg_u_ = static_cast<float>(opt_.num("reg_u"));
    reg_i_ = static_cast<float>(opt_.num("reg_i"));
    reg_j_ = static_cast<float>(opt_.num("reg_j"));
    reg_b_d_ = opt_.num_or("reg_b", 0.0);
    reg_b_ = static_cast<float>(reg_b_d_);
    update_i_ = opt_.boolean_or("update_i", true);
    update_j_ = opt_.boolean_or("update_j", true);
    use_bias_ = opt_.boolean_or("use_bias", false);
    pcn_ = opt_.boolean_or("per_coordinate_normalize", false);
    compute_loss_ = opt_.boolean_or("compute_loss_on_training", false);
    // the reference's CUDA backend reads a non-existent key "rand_seed" (bpr.cu:262, Q-19);
    // this backend follows the CPU path and uses "random_seed" (bpr.cc:83).
    seed_ = static_cast<uint32_t>(opt_.num_or("random_seed", 0));
    parse_specific();
    scratch_.resize(8, true, stream);
    inited_ = true;
    return true;
}

void SgdHandle::initialize_model(float* P, int P_rows, float* Q, float* Qb, int Q_rows, int64_t num_nnz, bool set_gpu) {
    BFH_REQUIRE(inited_, "initialize_model called before init");
    BFH_REQUIRE(P && Q && Qb && P_rows > 0 && Q_rows > 0, "initialize_model: null factors or empty shapes");
    if (host_stale_ && model_on_gpu_ && hostP_) synchronize(true, true);   // lazy_sync: the previous model's arrays are still owed
    hostP_ = P; hostQ_ = Q; hostQb_ = Qb;
    P_rows_ = P_rows; Q_rows_ = Q_rows;
    num_nnz_ = num_nnz;
    if (!set_gpu) return;  // bpr.cu:293-298: only record host pointers
    const size_t np = static_cast<size_t>(P_rows) * vdim_, nq = static_cast<size_t>(Q_rows) * vdim_;
    unpin_host();
    if (pin_host_) {   // opt-in ("pin_host" = 1; the default copies back through the library's own pinned ring, HostStager).  Best effort: a refusal just leaves the copies pageable
        // only arrays of a MiB or more: those sit in pages of their own (malloc hands them out by mmap); a small array shares its
        // pages with whatever else lives on the heap -- including arrays another handle has registered -- and overlapping
        // registrations have aborted inside the runtime (seen once in tests/test_errors_gpu.py, on 1.5 KB factors)
        auto pin = [&](void* p, size_t bytes) {
            if (bytes < (size_t(1) << 20)) return;
            if (hipHostRegister(p, bytes, hipHostRegisterDefault) == hipSuccess) pinned_.emplace_back(p, bytes);
            else (void)hipGetLastError();
        };
        pin(P, np * sizeof(float));
        pin(Q, nq * sizeof(float));
        pin(Qb, static_cast<size_t>(Q_rows) * sizeof(float));
    }
    P_.resize(np); Q_.resize(nq); Qb_.resize(Q_rows);
    BFH_HIP(hipMemcpyAsync(P_.get(), P, np * sizeof(float), hipMemcpyHostToDevice, stream));
    BFH_HIP(hipMemcpyAsync(Q_.get(), Q, nq * sizeof(float), hipMemcpyHostToDevice, stream));
    BFH_HIP(hipMemcpyAsync(Qb_.get(), Qb, Q_rows * sizeof(float), hipMemcpyHostToDevice, stream));
    stats.h2d_bytes += static_cast<double>((np + nq + Q_rows) * sizeof(float));
    if (!hogwild()) {  // lib/algo.cc:221-255
        gradP_.resize(np, true, stream); gradQ_.resize(nq, true, stream); gradQb_.resize(Q_rows, true, stream);
        velP_.resize(np, true, stream); velQ_.resize(nq, true, stream); velQb_.resize(Q_rows, true, stream);
        if (optimizer_ == "adam") {
            momP_.resize(np, true, stream); momQ_.resize(nq, true, stream); momQb_.resize(Q_rows, true, stream);
        }
        if (pcn_) {
            cntP_.resize(P_rows, true, stream);
            cntQ_.resize(Q_rows, true, stream);
        }
    }
    iters_ = 0;
    epoch_ = 0;
    processed_ = 0;
    model_on_gpu_ = true;
    exchange_.reset();
    sync_stream();
}

void SgdHandle::synchronize(bool device_to_host, bool force) {
    BFH_REQUIRE(hostP_ && model_on_gpu_, "synchronize before initialize_model(..., set_gpu=True)");
    exchange_finish();
    if (device_to_host && lazy_sync_ && !force) {   // the copy is owed until synchronize(2) / destroy / the next initialize_model
        host_stale_ = true;
        sync_stream();
        return;
    }
    if (device_to_host) host_stale_ = false;
    const size_t np = static_cast<size_t>(P_rows_) * vdim_, nq = static_cast<size_t>(Q_rows_) * vdim_;
    const hipMemcpyKind kind = device_to_host ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice;
    if (device_to_host) {
        // through the library's own pinned ring (HostStager, common.hpp) unless the caller asked for its arrays to be registered
        // ("pin_host" = 1); an array that is no longer mapped is an error, not a fault
        for (auto& c : {std::make_pair(static_cast<void*>(hostP_), np * sizeof(float)), std::make_pair(static_cast<void*>(hostQ_), nq * sizeof(float)),
                        std::make_pair(static_cast<void*>(hostQb_), static_cast<size_t>(Q_rows_) * sizeof(float))})
            if (!host_range_mapped(c.first, c.second))
                throw Error(BFH_ERR_INVALID, "the caller's factor array is no longer mapped (freed while the model still owes it a copy?)");
        if (!pinned_.empty()) {
            BFH_HIP(hipMemcpyAsync(hostP_, P_.get(), np * sizeof(float), kind, stream));
            BFH_HIP(hipMemcpyAsync(hostQ_, Q_.get(), nq * sizeof(float), kind, stream));
        } else {
            stager_.d2h(hostP_, P_.get(), np * sizeof(float), stream, device);
            stager_.d2h(hostQ_, Q_.get(), nq * sizeof(float), stream, device);
        }
        BFH_HIP(hipMemcpyAsync(hostQb_, Qb_.get(), Q_rows_ * sizeof(float), kind, stream));
        stats.d2h_bytes += static_cast<double>((np + nq + Q_rows_) * sizeof(float));
    } else {
        BFH_HIP(hipMemcpyAsync(P_.get(), hostP_, np * sizeof(float), kind, stream));
        BFH_HIP(hipMemcpyAsync(Q_.get(), hostQ_, nq * sizeof(float), kind, stream));
        BFH_HIP(hipMemcpyAsync(Qb_.get(), hostQb_, Q_rows_ * sizeof(float), kind, stream));
        stats.h2d_bytes += static_cast<double>((np + nq + Q_rows_) * sizeof(float));
    }
    sync_stream();
}

void SgdHandle::device_buffer(const std::string& name, void** p, size_t* bytes) {
    finish_for_reader();
    struct { const char* n; void* ptr; size_t b; } tab[] = {
        {"P", P_.get(), P_.bytes()}, {"Q", Q_.get(), Q_.bytes()}, {"Qb", Qb_.get(), Qb_.bytes()},
        {"gradP", gradP_.get(), gradP_.bytes()}, {"gradQ", gradQ_.get(), gradQ_.bytes()}, {"gradQb", gradQb_.get(), gradQb_.bytes()},
        {"countP", cntP_.get(), cntP_.bytes()}, {"countQ", cntQ_.get(), cntQ_.bytes()},
        {"velP", velP_.get(), velP_.bytes()}, {"velQ", velQ_.get(), velQ_.bytes()},
        {"momP", momP_.get(), momP_.bytes()}, {"momQ", momQ_.get(), momQ_.bytes()},
        {"velQb", velQb_.get(), velQb_.bytes()}, {"momQb", momQb_.get(), momQb_.bytes()},
    };
    for (auto& t : tab)
        if (name == t.n) {
            *p = t.ptr;
            *bytes = t.b;
            return;
        }
    throw Error(BFH_ERR_INVALID, "unknown device buffer '" + name + "'");
}

void SgdHandle::set_mode(const std::string& name, int64_t v) {
    if (name == "sequential") sequential_ = static_cast<int>(v);
    else if (name == "hogwild_atomic") {
        BFH_REQUIRE(v == 0 || v == 1 || ((v == 2 || v == 3) && kind_ == 0),
                    "hogwild_atomic must be 0 (write-through stores), 1 (fp32 atomics) or, for BPRMF, 2 (per-XCD replicas) / 3 (item-major)");
        hogwild_atomic_ = static_cast<int>(v);
    }
    else if (name == "accum_two_pass") accum_two_pass_ = v != 0;
    else if (name == "gather_waves_per_cu") gather_waves_per_cu_ = static_cast<int>(v);
    else if (name == "auto_resident") auto_resident_ = v != 0;
    else if (name == "lazy_sync") lazy_sync_ = v != 0;
    else if (name == "pin_host") pin_host_ = v != 0;
    else if (name == "comm_overlap") comm_overlap_ = v != 0;
    else if (name == "comm_stiffness") { BFH_REQUIRE(v >= 0, "comm_stiffness is a permille value >= 0 (0: plain sum of the deltas)"); exchange_.set_stiffness(static_cast<int>(v)); }
    else if (name == "comm_stiffness_q") { BFH_REQUIRE(v >= 0, "comm_stiffness_q is a permille value >= 0"); exchange_.set_stiffness_q(static_cast<int>(v)); }
    else if (name == "comm_segments") { BFH_REQUIRE(v >= 0 && v <= 64, "comm_segments must be in [0,64] (0 = one blocking exchange per call)"); comm_segments_ = static_cast<int>(v); }
    else if (name == "prefetch") prefetch_ = static_cast<int>(v);
    else if (name == "waves_per_cu") waves_per_cu_ = static_cast<int>(v);
    else if (name == "chunk") { BFH_REQUIRE(v >= 64 && v % 64 == 0, "chunk must be a positive multiple of 64"); chunk_ = static_cast<int>(v); chunk_set_ = true; }
    else if (name == "timing") timing = v != 0;
    else if (name == "epoch") epoch_ = static_cast<uint32_t>(v);
    else throw Error(BFH_ERR_INVALID, "unknown mode '" + name + "'");
}

void SgdHandle::harvest_timers() {
    stats.kernel_ms += t_main_.drain();
    stats.optimizer_ms += t_opt_.drain();
    stats.aux_ms += t_aux_.drain();
    exchange_.drain_timers(stats);
}

// ------------------------------------------------------------------------------------------------
// SgdHandle: staging -- placeholders, the resident matrix, chunks and their residency, the lr schedule
// ------------------------------------------------------------------------------------------------
void SgdHandle::set_placeholder(const int64_t* indptr, size_t batch_size) {
    BFH_REQUIRE(P_rows_ > 0, "set_placeholder called before initialize_model");
    BFH_REQUIRE(indptr, "set_placeholder: null indptr");
    indptr_host_.assign(indptr, indptr + P_rows_);
    indptr_.resize(P_rows_);
    BFH_HIP(hipMemcpyAsync(indptr_.get(), indptr, P_rows_ * sizeof(int64_t), hipMemcpyHostToDevice, stream));
    stats.h2d_bytes += static_cast<double>(P_rows_ * sizeof(int64_t));
    if (!resident_) {
        keys_.resize(batch_size);
        rows_.resize(batch_size);
        chunks_.clear();
    }
    placeholder_set_ = true;
    sync_stream();
}

void SgdHandle::set_resident_csr(const int64_t* indptr, const int32_t* keys, int64_t nnz) {
    BFH_REQUIRE(P_rows_ > 0, "set_resident_csr called before initialize_model");
    BFH_REQUIRE(indptr && keys && nnz >= 0, "set_resident_csr: null arrays");
    BFH_REQUIRE(indptr[P_rows_ - 1] == nnz, "set_resident_csr: indptr[-1] != nnz");
    indptr_host_.assign(indptr, indptr + P_rows_);
    indptr_.resize(P_rows_);
    keys_.resize(static_cast<size_t>(nnz));
    rows_.resize(static_cast<size_t>(nnz));
    BFH_HIP(hipMemcpyAsync(indptr_.get(), indptr, P_rows_ * sizeof(int64_t), hipMemcpyHostToDevice, stream));
    BFH_HIP(hipMemcpyAsync(keys_.get(), keys, nnz * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    stats.h2d_bytes += static_cast<double>(P_rows_ * sizeof(int64_t) + nnz * sizeof(int32_t));
    launch_fill_rows(indptr_.get(), 0, P_rows_, 0, nnz, rows_.get(), stream);
    resident_ = true;
    csr_generation_ += 1;
    resident_nnz_ = nnz;
    placeholder_set_ = true;
    sync_stream();
}

void SgdHandle::set_cumulative_table(const int64_t* table) {
    BFH_REQUIRE(Q_rows_ > 0, "set_cumulative_table called before initialize_model");
    BFH_REQUIRE(table, "set_cumulative_table: null table");
    cum_.resize(Q_rows_);
    BFH_HIP(hipMemcpyAsync(cum_.get(), table, Q_rows_ * sizeof(int64_t), hipMemcpyHostToDevice, stream));
    cum_total_ = table[Q_rows_ - 1];
    have_cum_ = true;
    sync_stream();
}

int64_t SgdHandle::stage_chunk(int start_x, int next_x, const int64_t* indptr, const int32_t* keys, SgdParams* pr) {
    BFH_REQUIRE(model_on_gpu_, "partial_update before initialize_model(..., set_gpu=True)");
    BFH_REQUIRE(placeholder_set_, "partial_update before set_placeholder");
    BFH_REQUIRE(0 <= start_x && start_x <= next_x && next_x <= P_rows_, "partial_update: bad row range");
    const int64_t* ip = indptr ? indptr : indptr_host_.data();
    const int64_t beg = start_x == 0 ? 0 : ip[start_x - 1];
    const int64_t end = next_x == 0 ? 0 : ip[next_x - 1];
    const int64_t n = end - beg;
    std::memset(pr, 0, sizeof(*pr));
    pr->P = P_.get(); pr->Q = Q_.get(); pr->Qb = Qb_.get();
    pr->gradP = gradP_.get(); pr->gradQ = gradQ_.get(); pr->gradQb = gradQb_.get();
    pr->cntP = cntP_.get(); pr->cntQ = cntQ_.get();
    pr->indptr = indptr_.get();
    pr->cum_table = have_cum_ ? cum_.get() : nullptr;
    pr->chunk_nnz = n;
    pr->shift = beg;
    pr->nnz_offset = nnz_offset_;
    pr->P_rows = P_rows_; pr->Q_rows = Q_rows_; pr->d = d_; pr->vdim = vdim_;
    pr->seed = seed_; pr->epoch = epoch_;
    if (n == 0) return 0;
    if (keys) {
        if (resident_) {
            // caller insists on passing keys although a resident CSR exists: honour the resident copy
            pr->keys = keys_.get() + beg;
            pr->rows = rows_.get() + beg;
        } else if (auto_resident_) {
            // every chunk keeps its place in a full-size device copy of the matrix; it is uploaded when its row range is new or
            // the 64-bit hash over the whole host buffer differs from the one it was uploaded with
            const int64_t total = indptr_host_.empty() ? n : indptr_host_.back();
            BFH_REQUIRE(end <= total, "partial_update: indptr disagrees with the placeholder's");
            if (keys_.size() < static_cast<size_t>(total)) {
                keys_.resize(static_cast<size_t>(total));
                rows_.resize(static_cast<size_t>(total));
                chunks_.clear();
            }
            const uint64_t sig = content_signature(keys, n);
            auto it = chunks_.find({start_x, next_x});
            if (it == chunks_.end() || it->second.n != n || it->second.sig != sig) {
                BFH_HIP(hipMemcpyAsync(keys_.get() + beg, keys, n * sizeof(int32_t), hipMemcpyHostToDevice, stream));
                stats.h2d_bytes += static_cast<double>(n * sizeof(int32_t));
                launch_fill_rows(indptr_.get(), start_x, next_x, beg, n, rows_.get() + beg, stream);
                chunks_[{start_x, next_x}] = ChunkSig{n, sig};
                csr_generation_ += 1;   // whatever was derived from the old content (item-major regrouping, incidence lists) is stale
            }
            pr->keys = keys_.get() + beg;
            pr->rows = rows_.get() + beg;
        } else {
            BFH_REQUIRE(static_cast<size_t>(n) <= keys_.size(), "partial_update: chunk larger than the placeholder batch_size");
            BFH_HIP(hipMemcpyAsync(keys_.get(), keys, n * sizeof(int32_t), hipMemcpyHostToDevice, stream));
            stats.h2d_bytes += static_cast<double>(n * sizeof(int32_t));
            launch_fill_rows(indptr_.get(), start_x, next_x, beg, n, rows_.get(), stream);
            pr->keys = keys_.get();
            pr->rows = rows_.get();
        }
    } else {
        BFH_REQUIRE(resident_, "partial_update: keys == NULL needs bfh_*_set_resident_csr first");
        pr->keys = keys_.get() + beg;
        pr->rows = rows_.get() + beg;
    }
    return n;
}

const int32_t* SgdHandle::upload_triples(int64_t n, const int32_t* users, const int32_t* pos, const int32_t* neg) {
    inj_.resize(static_cast<size_t>(3) * n);
    BFH_HIP(hipMemcpyAsync(inj_.get(), users, n * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    BFH_HIP(hipMemcpyAsync(inj_.get() + n, pos, n * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    BFH_HIP(hipMemcpyAsync(inj_.get() + 2 * n, neg, n * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    return inj_.get();
}

// Deterministic form of the reference's lr decay (lib/algo.cc:280-287, Q-8): the lr of a call is
// the one the progress thread would publish after all previously submitted jobs completed.  Same
// rule as CuBPR's host-side decay (bpr.cu:399-401) but with the CPU path's progress accounting.
double SgdHandle::current_lr() const {
    const double total = static_cast<double>(num_nnz_) * static_cast<double>(num_iters_);
    const double progress = total > 0 ? processed_ / total : 0.0;
    double a = lr_ - (lr_ - min_lr_) * progress;
    return a > min_lr_ ? a : min_lr_;
}

void SgdHandle::advance_progress(int start_x, int next_x, const int64_t* ip_arg) {
    const int64_t* ip = ip_arg ? ip_arg : indptr_host_.data();
    // job.size = 1 (user slot) + n_pos for every non-empty user (include/buffalo/algo.hpp:38-42)
    int64_t sz = 0;
    int64_t prev = start_x == 0 ? 0 : ip[start_x - 1];
    for (int x = start_x; x < next_x; ++x) {
        const int64_t e = ip[x];
        if (e > prev) sz += 1 + (e - prev);
        prev = e;
    }
    processed_ += static_cast<double>(sz) * num_shards_;
}

// ------------------------------------------------------------------------------------------------
// SgdHandle: the epoch-end optimizer step (adam / adagrad / WARP) over P, Qb and Q
// ------------------------------------------------------------------------------------------------
void SgdHandle::optimizer_step() {
    const bool adam = optimizer_ == "adam";
    const double beta1 = beta1_, beta2 = beta1_;  // Q-5: beta2 is read from "beta1" (lib/algo.cc:396)
    OptConsts k;
    k.lr = static_cast<float>(lr_);
    k.b1 = static_cast<float>(beta1); k.omb1 = static_cast<float>(1.0 - beta1);
    k.b2 = static_cast<float>(beta2); k.omb2 = static_cast<float>(1.0 - beta2);
    k.c1 = static_cast<float>(1.0 - std::pow(beta1, iters_ + 1));
    k.c2 = static_cast<float>(1.0 - std::pow(beta2, iters_ + 1));
    const int G = lane_group_of(vdim_), rpw = 64 / G;
    const bool proj = project_unit_ball();
    auto rows_step = [&](float* X, float* g, float* m, float* v, const int* cnt, int rows, float reg) {
        k.reg2 = static_cast<float>(2.0 * static_cast<double>(reg));
        const int waves = (rows + rpw - 1) / rpw;
        const int blocks = (waves + 3) / 4;
        if (adam && proj) hipLaunchKernelGGL((sgd_update_rows_kernel<true, true>), dim3(blocks), dim3(256), 0, stream, X, g, m, v, cnt, rows, vdim_, G, k);
        else if (adam) hipLaunchKernelGGL((sgd_update_rows_kernel<true, false>), dim3(blocks), dim3(256), 0, stream, X, g, m, v, cnt, rows, vdim_, G, k);
        else if (proj) hipLaunchKernelGGL((sgd_update_rows_kernel<false, true>), dim3(blocks), dim3(256), 0, stream, X, g, m, v, cnt, rows, vdim_, G, k);
        else hipLaunchKernelGGL((sgd_update_rows_kernel<false, false>), dim3(blocks), dim3(256), 0, stream, X, g, m, v, cnt, rows, vdim_, G, k);
        BFH_HIP(hipGetLastError());
    };
    auto bias_step = [&](float* X, float* g, float* m, float* v, const int* cnt, int rows, float reg) {
        k.reg2 = static_cast<float>(2.0 * static_cast<double>(reg));
        if (adam) hipLaunchKernelGGL((sgd_update_bias_kernel<true>), dim3(blocks_of(rows)), dim3(256), 0, stream, X, g, m, v, cnt, rows, use_bias_, k);
        else hipLaunchKernelGGL((sgd_update_bias_kernel<false>), dim3(blocks_of(rows)), dim3(256), 0, stream, X, g, m, v, cnt, rows, use_bias_, k);
        BFH_HIP(hipGetLastError());
    };
    rows_step(P_.get(), gradP_.get(), momP_.get(), velP_.get(), pcn_ ? cntP_.get() : nullptr, P_rows_, reg_u_);
    // reference order: Q rows, with the bias handled inside the same loop (algo.cc:407-420)
    bias_step(Qb_.get(), gradQb_.get(), momQb_.get(), velQb_.get(), pcn_ ? cntQ_.get() : nullptr, Q_rows_, reg_b_);
    rows_step(Q_.get(), gradQ_.get(), momQ_.get(), velQ_.get(), pcn_ ? cntQ_.get() : nullptr, Q_rows_, reg_i_);
    if (pcn_) {   // the counts are spent
        BFH_HIP(hipMemsetAsync(cntP_.get(), 0, cntP_.bytes(), stream));
        BFH_HIP(hipMemsetAsync(cntQ_.get(), 0, cntQ_.bytes(), stream));
    }
}

void SgdHandle::update_parameters() {
    BFH_REQUIRE(model_on_gpu_, "update_parameters before initialize_model(..., set_gpu=True)");
    if (!hogwild()) {
        exchange_arm();
        exchange_.gradients(gradient_pair(), pcn_ ? cntQ_.get() : nullptr, stats);
        const int slot = t_opt_.begin(stream);
        optimizer_step();
        exchange_.rebase(gradient_pair());
        t_opt_.end(slot, stream);
    }
    iters_ += 1;
    epoch_ += 1;
    sync_stream();
    harvest_timers();
}

}  // namespace bfh

// Host-only: the incidences one wave of grad_gather_kernel owns (the tests build their run lengths around it)
extern "C" int bfh_sgd_gather_chunk() { return bfh::kGatherChunk; }
