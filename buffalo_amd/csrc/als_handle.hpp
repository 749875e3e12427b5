// ALS handle (gfx950): the host side of the kernels in als_kernels.hpp -- the model and its host arrays, the placeholder and the
// resident matrices, the plan of one partial_update call and its launch sequence, fold-in, the row exchange.  What it shares with
// CfrHandle and EalsHandle (options, stream, Gramian, the slot path) is AlsCore (als_core.hpp).
#pragma once
#include "als_core.hpp"
#include "comm.hpp"

namespace bfh {

class AlsHandle : public AlsCore {
 public:   // the entry points of als.hip
    ~AlsHandle() override { unpin_host(); }   // (~AlsCore closes the stream)
    int vdim() const { return vdim_; }

    bool init(const char* opt_path) {
        if (!init_common(opt_path, 1024, 2)) return false;
        adaptive_reg_ = opt_.boolean_or("adaptive_reg", false);
        compute_loss_ = opt_.boolean_or("compute_loss_on_training", false);
        eps_ = static_cast<float>(opt_.num_or("eps", 1e-10));
        cg_tol_ = static_cast<float>(opt_.num_or("cg_tolerance", 1e-10));
        num_cg_max_iters_ = static_cast<int>(opt_.num_or("num_cg_max_iters", 3));
        block_size_ = static_cast<int>(opt_.num_or("block_size", 32));
        BFH_REQUIRE(block_size_ > 0, "block_size must be positive");
        std::string optimizer = opt_.str("optimizer");
        if (d_ >= 128) optimizer = "ialspp";  // als.cc:46 (Q-13)
        if (optimizer == "llt") code_ = 0;
        else if (optimizer == "ldlt") code_ = 1;
        else if (optimizer == "manual_cg") code_ = 2;
        else if (optimizer == "ialspp") code_ = 8;
        else throw Error(BFH_ERR_UNSUPPORTED, "optimizer '" + optimizer + "' is not implemented on gfx950 (supported: llt, ldlt, manual_cg, ialspp)");
        inited_ = true;
        return true;
    }

    void initialize_model(float* P, int P_rows, float* Q, int Q_rows) {
        BFH_REQUIRE(inited_, "initialize_model called before init");
        BFH_REQUIRE(P && Q && P_rows > 0 && Q_rows > 0, "initialize_model: null factors or empty shapes");
        hostP_ = P; hostQ_ = Q; P_rows_ = P_rows; Q_rows_ = Q_rows;
        const size_t np = static_cast<size_t>(P_rows) * vdim_, nq = static_cast<size_t>(Q_rows) * vdim_;
        unpin_host();
        if (pin_host_) {   // opt-in ("pin_host" = 1): page-lock the caller's arrays; the default goes through the library's own pinned ring
            for (auto pr : {std::make_pair(static_cast<void*>(P), np * sizeof(float)), std::make_pair(static_cast<void*>(Q), nq * sizeof(float))}) {
                if (pr.second < (size_t(1) << 20)) continue;   // small arrays share heap pages with other objects: see SgdHandle::initialize_model
                if (hipHostRegister(pr.first, pr.second, hipHostRegisterDefault) == hipSuccess) pinned_.push_back(pr.first);
                else (void)hipGetLastError();
            }
        }
        P_.resize(np); Q_.resize(nq);
        BFH_HIP(hipMemcpyAsync(P_.get(), P, np * sizeof(float), hipMemcpyHostToDevice, stream));
        BFH_HIP(hipMemcpyAsync(Q_.get(), Q, nq * sizeof(float), hipMemcpyHostToDevice, stream));
        stats.h2d_bytes += static_cast<double>((np + nq) * sizeof(float));
        BFH_HIP(hipStreamSynchronize(stream));
        ++fver_[0]; ++fver_[1];
        model_ = true;
    }

    void set_placeholder(const int64_t* lindptr, const int64_t* rindptr, size_t batch_size) {
        BFH_REQUIRE(model_, "set_placeholder called before initialize_model");
        BFH_REQUIRE(lindptr && rindptr, "set_placeholder: null indptr");
        const int64_t* ip[2] = {lindptr, rindptr};
        const int rows[2] = {P_rows_, Q_rows_};
        for (int a = 0; a < 2; ++a) {
            ax_[a].indptr_host.assign(ip[a], ip[a] + rows[a]);
            ax_[a].indptr.resize(rows[a]);
            BFH_HIP(hipMemcpyAsync(ax_[a].indptr.get(), ip[a], rows[a] * sizeof(int64_t), hipMemcpyHostToDevice, stream));
        }
        keys_.resize(batch_size);
        vals_.resize(batch_size);
        yui_.resize(batch_size);
        ax_[0].chunks.clear();
        ax_[1].chunks.clear();
        BFH_HIP(hipStreamSynchronize(stream));
        work_cache_.clear();
        placeholder_ = true;
    }

    void set_resident_csr(int axis, const int64_t* indptr, const int32_t* keys, const float* vals, int64_t nnz) {
        BFH_REQUIRE(model_, "set_resident_csr called before initialize_model");
        BFH_REQUIRE(axis == 0 || axis == 1, "axis must be 0 or 1");
        BFH_REQUIRE(indptr && keys && vals, "set_resident_csr: null arrays");
        const int rows = axis == 0 ? P_rows_ : Q_rows_;
        BFH_REQUIRE(indptr[rows - 1] == nnz, "set_resident_csr: indptr[-1] != nnz");
        Axis& A = ax_[axis];
        A.indptr_host.assign(indptr, indptr + rows);
        A.indptr.resize(rows);
        A.keys.resize(static_cast<size_t>(nnz));
        A.vals.resize(static_cast<size_t>(nnz));
        BFH_HIP(hipMemcpyAsync(A.indptr.get(), indptr, rows * sizeof(int64_t), hipMemcpyHostToDevice, stream));
        BFH_HIP(hipMemcpyAsync(A.keys.get(), keys, nnz * sizeof(int32_t), hipMemcpyHostToDevice, stream));
        BFH_HIP(hipMemcpyAsync(A.vals.get(), vals, nnz * sizeof(float), hipMemcpyHostToDevice, stream));
        stats.h2d_bytes += static_cast<double>(rows * sizeof(int64_t) + nnz * 8);
        if (yui_.size() < static_cast<size_t>(nnz)) yui_.resize(static_cast<size_t>(nnz));
        BFH_HIP(hipStreamSynchronize(stream));
        work_cache_.clear();
        ++vals_ver_;
        A.resident = true;
    }

    void precompute(int axis) {
        BFH_REQUIRE(model_, "precompute before initialize_model");
        BFH_REQUIRE(axis == 0 || axis == 1, "axis must be 0 or 1");
        gramian_of(axis == 0 ? Q_.get() : P_.get(), axis == 0 ? Q_rows_ : P_rows_);
        // a new half-epoch: whatever was derived from the other factor (its interleaved copy, the split scale) is rebuilt by the next
        // partial_update -- the factor may have been written through a device pointer handed out earlier (row exchange of a sharded
        // run), which no version counter of this handle sees; the chunks of ONE half-epoch still share the copy
        qi_side_ = -1;
    }

    // One call = the rows [start_x, next_x) of one side: bind the chunk, choose the kernel family, launch it, collect.
    void partial_update(int start_x, int next_x, const int64_t* indptr, const int32_t* keys, const float* vals, int axis,
                        double* nume, double* deno) {
        BFH_REQUIRE(model_, "partial_update before initialize_model");
        BFH_REQUIRE(axis == 0 || axis == 1, "axis must be 0 or 1");
        Axis& A = ax_[axis];
        const int rows = axis == 0 ? P_rows_ : Q_rows_;
        BFH_REQUIRE(A.resident || placeholder_, "partial_update before set_placeholder");
        BFH_REQUIRE(0 <= start_x && start_x <= next_x && next_x <= rows, "partial_update: bad row range");
        *nume = 0.0;
        *deno = 0.0;
        last_plan_ = Plan{};   // a call without rows runs no kernel: als_last_path reads 0
        if (next_x == start_x) return;  // als.cc:219-222
        const int64_t* ip = indptr ? indptr : A.indptr_host.data();
        const int64_t beg = start_x == 0 ? 0 : ip[start_x - 1];
        const int64_t n = ip[next_x - 1] - beg;
        const int nrows = next_x - start_x;
        AlsParams p = make_params(axis, start_x, next_x, beg);
        bind_chunk(axis, p, start_x, next_x, beg, n, keys, vals);
        BFH_HIP(hipMemsetAsync(loss_.get(), 0, 2 * sizeof(double), stream));
        BFH_HIP(hipMemsetAsync(ticket_.get(), 0, sizeof(int), stream));
        // every path but the fallback walks a work list
        WorkList* wl = (vdim_ <= 128 || (vdim_ <= 256 && inplace_rows())) ? &work_list(axis == 0 ? WorkId::AlsUsers : WorkId::AlsItems, start_x, next_x, ip, beg) : nullptr;
        if (wl) grow(scratch_, std::max<size_t>(1, wl->n_heavy) * als_slot_floats(vdim_));   // the heavy rows' slots (scan_deferred adds the deferred rows')
        const int slot = t_main_.begin(stream);   // before the plan: the weight scan's kernel and its host round trip are part of kernel_ms
        const Plan plan = last_plan_ = choose_plan(axis, wl, p);
        // The slots that chunk tiles are SUMMED into start from zero: the heavy rows', then (pairs) the deferred rows'.  Zeroed here, after
        // everything that can grow scratch_ (its sizing above, scan_deferred: a new buffer, neither copied nor zeroed) and before every kernel of the call.
        const size_t nslots = wl ? static_cast<size_t>(wl->n_heavy) + (plan.path == Path::Pairs ? wl->n_def_rows : 0) : 0;
        if (nslots) BFH_HIP(hipMemsetAsync(scratch_.get(), 0, nslots * als_slot_floats(vdim_) * sizeof(float), stream));
        switch (plan.path) {
            case Path::Pairs: launch_pairs(p, *wl, plan, axis, start_x, nrows); break;
            case Path::GramInreg: launch_gram_inreg(p, *wl, plan, axis, start_x, nrows); break;
            case Path::GramScratch: launch_gram_scratch(p, *wl, nrows); break;
            case Path::Wide: launch_wide(p, *wl, plan, axis, start_x, nrows); break;
            case Path::Fallback: launch_ialspp(p, nrows); break;
            case Path::None: break;
        }
        BFH_HIP(hipGetLastError());
        t_main_.end(slot, stream);
        finish_call(p, plan.path == Path::Pairs, axis, start_x, nrows, n, nume, deno);
    }

    // ---- fold-in: factor rows for histories that are not in the model (bfh_als_fold_in) ---------------------------------------------
    // out[b] = (FF + alpha sum v q q^T + reg ada I)^-1 sum (1 + alpha v) q over row b of the CSR, q = rows of the OTHER factor (axis 0: Q).
    // Steps: refuse bad input on the host -> the fold-in Gramian of that factor (kept per axis while the factor does not change) -> upload ->
    // per sub-batch: row pass to slots (als_gram_kernel, dense form, fp32 instruction) -> exact solve -> copy out.  Everything it writes is
    // its own (FoldState); of the training state it reads P_ / Q_ and the options.
    void fold_in(int axis, int n_rows, const int64_t* indptr, const int32_t* keys, const float* vals, int64_t nnz, float* out) {
        BFH_REQUIRE(model_, "fold_in before initialize_model");
        fold_check(axis, n_rows, indptr, keys, vals, nnz);
        if (vdim_ > 128) throw Error(BFH_ERR_UNSUPPORTED, "fold_in: no dense solve above vdim 128 (d <= 128 is the limit; this model has d = " + std::to_string(d_) + ")");
        FoldState& f = fold_;
        f.rows = n_rows;
        if (n_rows == 0) return;
        fold_gramian(axis);
        if (f.ticket.size() < 1) f.ticket.resize(1);
        const size_t nout = static_cast<size_t>(n_rows) * vdim_;
        grow(f.out, nout);
        BFH_HIP(hipMemsetAsync(f.out.get(), 0, nout * sizeof(float), stream));   // empty rows and the padding columns stay 0
        grow(f.keys, static_cast<size_t>(std::max<int64_t>(nnz, 1)));
        grow(f.vals, static_cast<size_t>(std::max<int64_t>(nnz, 1)));
        if (nnz) {
            BFH_HIP(hipMemcpyAsync(f.keys.get(), keys, nnz * sizeof(int32_t), hipMemcpyHostToDevice, stream));
            BFH_HIP(hipMemcpyAsync(f.vals.get(), vals, nnz * sizeof(float), hipMemcpyHostToDevice, stream));
            stats.h2d_bytes += static_cast<double>(nnz * 8);
        }
        const std::vector<FoldBatch> batches = fold_plan(n_rows, indptr);
        AlsParams p{};
        p.P = f.out.get();
        p.Q = axis == 0 ? Q_.get() : P_.get();
        p.FF = f.ff[axis].get();
        p.d = d_; p.vdim = vdim_;
        p.op_rows = axis == 0 ? Q_rows_ : P_rows_;
        p.block_size = block_size_;
        p.alpha = alpha_;
        p.reg = axis == 0 ? reg_u_ : reg_i_;
        p.eps = eps_; p.cg_tol = cg_tol_;
        p.adaptive_reg = adaptive_reg_; p.axis = axis;   // compute_loss stays 0: no loss terms
        p.num_cg_max_iters = num_cg_max_iters_;
        p.loss = loss_.get();                             // (never written: compute_loss == 0)
        p.ticket = f.ticket.get();
        p.out_scale = 1.0f;
        p.ff_scale = 1.0f;
        const size_t per_slot = als_slot_floats(vdim_);
        const int tslot = t_main_.begin(stream);
        for (const FoldBatch& b : batches) {
            if (b.n_work == 0) continue;
            const int nrows = b.r1 - b.r0;
            p.start_x = b.r0; p.next_x = b.r1;
            p.keys = f.keys.get() + b.beg;
            p.vals = f.vals.get() + b.beg;
            if (b.n_heavy) BFH_HIP(hipMemsetAsync(f.slots.get() + static_cast<size_t>(nrows) * per_slot, 0, b.n_heavy * per_slot * sizeof(float), stream));
            BFH_HIP(hipMemsetAsync(f.ticket.get(), 0, sizeof(int), stream));
            launch_gram_to_slots(p, f.work.get() + b.work_off, b.n_work, f.slots.get(), nrows, false);
            const int sslot = f.t_solve.begin(stream);
            if (fold_solve_) launch_fold_solve(p, f.solve.get() + b.solve_off, b.n_solve, f.slots.get());
            else launch_solve(p, f.solve.get() + b.solve_off, b.n_solve, f.slots.get(), true, 0);
            f.t_solve.end(sslot, stream);
        }
        t_main_.end(tslot, stream);
        if (out) copy_out(out, f.out.get(), nout * sizeof(float));
        BFH_HIP(hipStreamSynchronize(stream));
        drain_aux();
        stats.kernel_ms += t_main_.drain();
        stats.optimizer_ms += f.t_solve.drain();   // the solve kernel alone (part of kernel_ms)
        stats.launches += 1;
        stats.samples += nnz;
    }

    void synchronize(bool d2h) {
        BFH_REQUIRE(model_, "synchronize before initialize_model");
        const size_t np = static_cast<size_t>(P_rows_) * vdim_, nq = static_cast<size_t>(Q_rows_) * vdim_;
        if (d2h) {
            copy_out(hostP_, P_.get(), np * sizeof(float));
            copy_out(hostQ_, Q_.get(), nq * sizeof(float));
        } else {
            BFH_HIP(hipMemcpyAsync(P_.get(), hostP_, np * sizeof(float), hipMemcpyHostToDevice, stream));
            BFH_HIP(hipMemcpyAsync(Q_.get(), hostQ_, nq * sizeof(float), hipMemcpyHostToDevice, stream));
            stats.h2d_bytes += static_cast<double>((np + nq) * sizeof(float));
            ++fver_[0]; ++fver_[1];
        }
        BFH_HIP(hipStreamSynchronize(stream));
    }

    // Multi-GPU: rows of the side being solved are sharded, both factor matrices replicated.
    // After a half-epoch in which rank r solved rows [bounds[r], bounds[r+1]) every rank receives every block: the uneven
    // all-gather as one group of ncclBroadcast calls (direct xGMI copies).  Every row is solved by exactly one rank from
    // identical inputs, so the replicas stay bit-identical to the single-GPU run.
    void publish_rows(int axis, const int* bounds, int n_bounds) {
        BFH_REQUIRE(model_, "publish_rows before initialize_model");
        BFH_REQUIRE(comm_, "publish_rows before bfh_als_set_comm");
        BFH_REQUIRE(axis == 0 || axis == 1, "axis must be 0 or 1");
        BFH_REQUIRE(bounds && n_bounds == comm_->size() + 1, "publish_rows: need world_size + 1 row boundaries");
        const int rows = axis == 0 ? P_rows_ : Q_rows_;
        BFH_REQUIRE(bounds[0] == 0 && bounds[n_bounds - 1] == rows, "publish_rows: boundaries must cover [0, rows)");
        for (int r = 0; r + 1 < n_bounds; ++r) BFH_REQUIRE(bounds[r] <= bounds[r + 1], "publish_rows: boundaries must ascend");   // before the group opens
        float* F = axis == 0 ? P_.get() : Q_.get();
        comm_->group_start();
        for (int r = 0; r + 1 < n_bounds; ++r) {
            const size_t cnt = static_cast<size_t>(bounds[r + 1] - bounds[r]) * vdim_;
            comm_->broadcast_bytes(F + static_cast<size_t>(bounds[r]) * vdim_, cnt * sizeof(float), r, stream);
        }
        comm_->group_end();
        BFH_HIP(hipStreamSynchronize(stream));
        ++fver_[axis];
        stats.exchanges += 1;
    }
    void set_comm(Comm* c) {
        BFH_REQUIRE(!c || c->device == device, "set_comm: the communicator lives on another device than this handle");
        comm_ = c;
    }

    void set_mode(const std::string& name, int64_t v) {
        if (name == "als_writeback") writeback_ = v != 0;
        else if (name == "auto_resident") auto_resident_ = v != 0;
        else if (name == "pin_host") pin_host_ = v != 0;
        else if (name == "als_wide_split") wide_split_ = v != 0;         // 128 < vdim <= 224: 1 = split-f16 Gramian in als_wide_kernel (default), 0 = the fp32 instruction
        else if (name == "als_split_wcut") split_wcut_ = static_cast<float>(v);   // weights above this take the fp32 side path (default 2^15; tests lower it)
        else if (name == "als_split_f16") split_f16_ = v != 0;             // 0: the in-place iALS++ rows keep the fp32 matrix instruction
        else if (name == "als_pc") {
            BFH_REQUIRE(v >= 0 && v <= 2, "als_pc must be 0, 1 or 2");
            pc_ = static_cast<int>(v);
        }   // 0: round 3's wave-per-row split kernel; 1: producer / consumer pairs where they win (d = 96, 128); 2: also at d = 64
        else if (name == "als_inreg") no_inreg_ = v == 0;                 // 0: iALS++ rows go through the scratch + solve kernel instead of the in-register solve
        else if (name == "timing") timing = v != 0;
        else if (name == "als_fold_solve") fold_solve_ = v != 0;         // fold_in's solve: 1 = als_fold_solve_kernel (default), 0 = als_solve_kernel with mode 0
        else if (name == "als_fold_slot_bytes") {                          // fold_in: bound on the slot scratch of one sub-batch (default 512 MiB; tests lower it)
            BFH_REQUIRE(v > 0, "als_fold_slot_bytes must be positive");
            fold_slot_bytes_ = v;
        }
        else throw Error(BFH_ERR_INVALID, "unknown mode '" + name + "'");
    }

    void device_buffer(const std::string& name, void** p, size_t* bytes) {
        // the plan of the last partial_update, as values (no pointer leaves, so no cached view is dropped): als_last_path 0 none, 1 pairs,
        // 2 wave per row solved in registers, 3 scratch + solve, 4 wide, 5 fallback
        if (name.compare(0, 9, "als_last_") == 0) {
            const Plan& lp = last_plan_;
            const std::string f = name.substr(9);
            size_t v;
            if (f == "path") v = lp.path == Path::None ? 0 : static_cast<size_t>(lp.path) + 1;
            else if (f == "split") v = lp.split;
            else if (f == "n_work") v = static_cast<size_t>(lp.n_work);
            else if (f == "n_heavy") v = static_cast<size_t>(lp.n_heavy);
            else if (f == "n_def") v = static_cast<size_t>(lp.n_def);
            else if (f == "n_def_rows") v = static_cast<size_t>(lp.n_def_rows);
            else throw Error(BFH_ERR_INVALID, "unknown device buffer '" + name + "'");
            *p = nullptr; *bytes = v;
            return;
        }
        if (name == "fold") {   // the rows of the last fold_in (which returned with the stream drained); no factor is handed out, so no cached view is dropped
            *p = fold_.rows ? fold_.out.get() : nullptr;
            *bytes = static_cast<size_t>(fold_.rows) * vdim_ * sizeof(float);
            return;
        }
        ++fver_[0]; ++fver_[1];   // whoever holds a raw pointer may write through it: cached views of the factors are dropped
        if (name == "als_pc_same_simd") { *p = nullptr; *bytes = static_cast<size_t>(pc_same_simd_); return; }   // placement statistic of the last als_pc_kernel launch
        // whoever takes a raw pointer reads it on ANOTHER stream (torch's): everything this handle has queued is finished first
        // (precompute no longer blocks: round 6)
        if (stream) BFH_HIP(hipStreamSynchronize(stream));
        if (name == "P") { *p = P_.get(); *bytes = P_.bytes(); }
        else if (name == "Q") { *p = Q_.get(); *bytes = Q_.bytes(); }
        else if (name == "FF") { *p = FF_.get(); *bytes = FF_.bytes(); }
        else throw Error(BFH_ERR_INVALID, "unknown device buffer '" + name + "'");
    }

 private:
    // iALS++ with block_size 32 and no padded columns: the form whose rows the fused kernels solve from their accumulators
    bool inplace_rows() const { return code_ == 8 && block_size_ == 32 && d_ == vdim_; }

    AlsParams make_params(int axis, int start_x, int next_x, int64_t beg) {
        AlsParams p{};
        p.P = axis == 0 ? P_.get() : Q_.get();
        p.Q = axis == 0 ? Q_.get() : P_.get();
        p.FF = FF_.get();
        p.indptr = ax_[axis].indptr.get();
        p.shift = beg;
        p.start_x = start_x; p.next_x = next_x;
        p.d = d_; p.vdim = vdim_;
        p.op_rows = axis == 0 ? Q_rows_ : P_rows_;
        p.block_size = block_size_;
        p.alpha = alpha_;
        p.reg = axis == 0 ? reg_u_ : reg_i_;
        p.eps = eps_; p.cg_tol = cg_tol_;
        p.adaptive_reg = adaptive_reg_; p.compute_loss = compute_loss_; p.axis = axis;
        p.num_cg_max_iters = num_cg_max_iters_;
        p.loss = loss_.get();
        p.ticket = ticket_.get();
        p.solver = static_cast<int>(code_);
        p.out_scale = 1.0f;
        p.ff_scale = 1.0f;
        return p;
    }

    // Where the chunk's keys / vals live on the device: the resident matrix, its auto-resident copy, or the placeholder
    // (uploaded now).  Bumps vals_ver_ whenever confidence values were uploaded.
    void bind_chunk(int axis, AlsParams& p, int start_x, int next_x, int64_t beg, int64_t n, const int32_t* keys, const float* vals) {
        Axis& A = ax_[axis];
        if (A.resident) {
            p.keys = A.keys.get() + beg;
            p.vals = A.vals.get() + beg;
        } else if (auto_resident_ && keys && vals && !A.indptr_host.empty()) {
            // the reference hands keys / vals over on every call (cuda/_als.pyx:52-67): a chunk seen before -- same row range,
            // same length, same 64-bit hash over both host buffers -- is served from its place in a full-size device copy
            const int64_t total = A.indptr_host.back();
            BFH_REQUIRE(beg + n <= total, "partial_update: indptr disagrees with the placeholder's");
            if (A.keys.size() < static_cast<size_t>(total)) {
                A.keys.resize(static_cast<size_t>(total));
                A.vals.resize(static_cast<size_t>(total));
                A.chunks.clear();
            }
            if (yui_.size() < static_cast<size_t>(n)) yui_.resize(static_cast<size_t>(n));
            const uint64_t sig = content_signature(keys, n) * 31u + content_signature(reinterpret_cast<const int32_t*>(vals), n);
            auto it = A.chunks.find({start_x, next_x});
            if (it == A.chunks.end() || it->second.first != n || it->second.second != sig) {
                if (n) {
                    BFH_HIP(hipMemcpyAsync(A.keys.get() + beg, keys, n * sizeof(int32_t), hipMemcpyHostToDevice, stream));
                    BFH_HIP(hipMemcpyAsync(A.vals.get() + beg, vals, n * sizeof(float), hipMemcpyHostToDevice, stream));
                    stats.h2d_bytes += static_cast<double>(n * 8);
                    ++vals_ver_;
                }
                A.chunks[{start_x, next_x}] = {n, sig};
            }
            p.keys = A.keys.get() + beg;
            p.vals = A.vals.get() + beg;
        } else {
            BFH_REQUIRE(keys && vals, "partial_update: keys/vals == NULL needs bfh_als_set_resident_csr first");
            BFH_REQUIRE(static_cast<size_t>(n) <= keys_.size(), "partial_update: chunk larger than the placeholder batch_size");
            if (n) {
                BFH_HIP(hipMemcpyAsync(keys_.get(), keys, n * sizeof(int32_t), hipMemcpyHostToDevice, stream));
                BFH_HIP(hipMemcpyAsync(vals_.get(), vals, n * sizeof(float), hipMemcpyHostToDevice, stream));
                stats.h2d_bytes += static_cast<double>(n * 8);
            }
            ++vals_ver_;
            p.keys = keys_.get();
            p.vals = vals_.get();
        }
        p.yui = yui_.get();
    }

    enum class Path {
        Pairs,         // als_pc_kernel: producer / consumer pairs, split-f16, rows solved in place (als_pc.hpp)
        GramInreg,     // als_gram_kernel<INREG>: wave per row, rows solved from the accumulators
        GramScratch,   // als_gram_kernel -> one HBM slot per row -> als_solve_kernel (the dense solvers; iALS++ with padding or another block_size)
        Wide,          // 128 < vdim <= 256: block-per-row kernel with the tiles spread over ceil(T/2) waves (als_wide_kernel)
        Fallback,      // als_ialspp_kernel: everything else (vdim > 256, or 128 < vdim <= 256 with padding or another block_size)
        None           // no partial_update yet, or one without rows
    };
    struct Plan {
        Path path = Path::None;
        bool split = false;   // the Gramian through the f16 matrix cores at fp32 accuracy (see als_gram_kernel); always on the pairs
        bool big = false;     // 64-bit gather offsets into the other factor
        bool loss = false;    // loss terms wanted from the row kernels (compute_loss_on_training, item half-epoch)
        // what the call's work list held when the plan was made (read back as "als_last_*", device_buffer): work items, rows above HEAVY
        // entries, and -- where this plan scanned the weights, 0 elsewhere -- the items / whole rows sent to the fp32 instruction
        int n_work = 0, n_heavy = 0, n_def = 0, n_def_rows = 0;
    };

    // Which kernel family runs this call, and in which form.  The one place that scans the weights (scan_deferred) and looks at its counts.
    Plan choose_plan(int axis, WorkList* wl, const AlsParams& p) {
        Plan plan;
        plan.path = Path::Fallback;
        plan.big = big_gather(p);
        plan.loss = compute_loss_ && axis == 1;
        if (!wl) return plan;
        const int T = vdim_ / 32, items = wl->n_work;
        plan.n_work = wl->n_work;
        plan.n_heavy = wl->n_heavy;
        if (vdim_ > 128) {
            plan.path = Path::Wide;
            // "als_wide_split" (default on; vdim 160 .. 224, ALS_WIDE_SPLIT_MAX_T): the Gramian through the f16 matrix cores at fp32 accuracy, rows gathered once
            // per block by a producer wave (als_wide_item<SPLIT>); from T = 6 up with the fourth product l l (d = 192 stayed on the fp32 form while
            // the three-product form put one ill-conditioned tiny case at 5.9x the oracle's distance from float64: with l l it lands at 3.8x, bound 4x).
            // For calls whose weights all fit the f16 path; als_defer_scan_kernel says so (cached per chunk while the values do not change)
            plan.split = wide_split_ && split_f16_ && T >= 5 && T <= ALS_WIDE_SPLIT_MAX_T && items > 0;
            if (plan.split) {
                scan_deferred(*wl, p, items);
                plan.n_def = wl->n_def; plan.n_def_rows = wl->n_def_rows;
                plan.split = wl->n_def == 0;
            }
            return plan;
        }
        // wave-per-row Gramian pass; rows are solved from the accumulators (iALS++, block_size 32, d == vdim) or
        // go through an HBM scratch slot to the dense-solve kernel (see als_gram_kernel)
        plan.path = inplace_rows() && !no_inreg_ ? Path::GramInreg : Path::GramScratch;
        if (plan.path == Path::GramScratch || items == 0 || !split_f16_ || T < 2) return plan;
        plan.split = true;   // als_split_f16 (default on, d >= 64)
        // producer / consumer pairs (als_pc.hpp): the default for the in-place iALS++ rows at d = 96 / 128
        // (measured on the ML-20M shape, profiles/r04_als_pc_steps.txt: d = 128 4.53 vs 5.08 ms, d = 96 3.47 vs 3.95, d = 64 2.47 vs 2.06 --
        //  at T = 2 the wave-per-row kernel already runs two waves per SIMD, and the pairs only add their hand-off: "als_pc" = 2 forces them)
        if (pc_ >= 2 || (pc_ == 1 && T >= 3)) {
            scan_deferred(*wl, p, items);
            plan.n_def = wl->n_def; plan.n_def_rows = wl->n_def_rows;
            if (wl->n_def_rows > 4096 || wl->n_def * 4 > items) {
                // weights mostly outside the f16 path (negative confidences, ...): every row of the call takes the route the flagged
                // ones would take -- fp32 instruction, scratch slot, dense-solve kernel
                plan.path = Path::GramScratch;
                plan.split = false;
            } else {
                plan.path = Path::Pairs;
            }
        }
        return plan;
    }

    // The scale of the split pass, decided on the device (no host round trip) -- with_interleave: together with the block-interleaved copy of
    // the other factor the producers gather from; both are kept while that factor does not change (the chunks of one half-epoch share them)
    void prepare_split(AlsParams& p, int axis, int T, bool with_interleave) {
        const int oside = axis == 0 ? 1 : 0;   // which factor is "the other side"
        if (split_out_.size() < 4) { split_part_.resize(ALS_STAT_BLOCKS); split_out_.resize(4); }
        p.split = split_out_.get();
        if (with_interleave) {
            const size_t nq = static_cast<size_t>(p.op_rows) * vdim_;
            if (qi_.size() < nq) { qi_.resize(nq); qi_side_ = -1; }
            if (qi_side_ == oside && qi_ver_ == fver_[oside] && qi_wcut_ == split_wcut_) return;
            dispatch_int<2, 8>(T, [&](auto tt) {
                hipLaunchKernelGGL(als_interleave_stats_kernel<decltype(tt)::value>, dim3(ALS_STAT_BLOCKS), dim3(256), 0, stream, p.Q, static_cast<size_t>(p.op_rows),
                                   qi_.get(), split_part_.get());
            });
            qi_side_ = oside; qi_ver_ = fver_[oside]; qi_wcut_ = split_wcut_;
        } else {
            hipLaunchKernelGGL(als_split_stats_kernel, dim3(ALS_STAT_BLOCKS), dim3(256), 0, stream, p.Q, static_cast<size_t>(p.op_rows) * vdim_, split_part_.get());
            qi_side_ = -1;   // split_out_ is rewritten for another matrix
        }
        hipLaunchKernelGGL(als_split_scale_kernel, dim3(1), dim3(64), 0, stream, split_part_.get(), ALS_STAT_BLOCKS, split_wcut_, split_out_.get());
        BFH_HIP(hipGetLastError());
    }

    // FF p0 for every row of the call (the residual-first gradient starts from it: als_gram_kernel<SPLIT>, als_pc_kernel, als_wide_item)
    void launch_rowff(AlsParams& p, int T, int start_x, int nrows) {
        const size_t need0 = static_cast<size_t>(nrows) * vdim_;
        if (rowff_.size() < need0) rowff_.resize(need0);
        const int quads = (nrows + 3) / 4;
        const int rb = std::max(1, std::min((quads + 3) / 4, num_cus_ * 8));
        dispatch_int<2, 8>(T, [&](auto tt) {
            hipLaunchKernelGGL(als_rowff_kernel<decltype(tt)::value>, dim3(rb), dim3(256), 0, stream, p.P, start_x, nrows, FF_.get(), rowff_.get());
        });
        BFH_HIP(hipGetLastError());
        p.F0 = rowff_.get();
    }

    // als_fold_solve_kernel over the n slots of a list: the block-wide Cholesky, persistent
    void launch_fold_solve(const AlsParams& p, const AlsHeavy* list, int n, const float* scratch) {
        const size_t lds = als_gs_lds_bytes(vdim_);
        BFH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(als_fold_solve_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
        hipLaunchKernelGGL(als_fold_solve_kernel, dim3(std::min(n, persistent_solve_blocks(lds))), dim3(256), lds, stream, p, list, n, scratch);
        BFH_HIP(hipGetLastError());
    }

    void launch_pairs(AlsParams& p, const WorkList& wl, const Plan& plan, int axis, int start_x, int nrows) {
        const int T = vdim_ / 32, items = wl.n_work;
        prepare_split(p, axis, T, true);
        launch_rowff(p, T, start_x, nrows);
        p.batch = 16;   // rows per ticket at most (fewer where the rows are long)
        if (pc_err_.size() < 2) pc_err_.resize(2);   // [0] error bits, [1] placement statistic
        BFH_HIP(hipMemsetAsync(pc_err_.get(), 0, 2 * sizeof(int), stream));
        const int pblocks = std::max(1, std::min((items + 3) / 4, num_cus_));
        dispatch_int<2, 4>(T, [&](auto tt) { dispatch_bool(plan.big, [&](auto bg) { dispatch_bool(plan.loss, [&](auto ls) {
            constexpr int TT = decltype(tt)::value;
            constexpr bool BG = decltype(bg)::value, LS = decltype(ls)::value;
            BFH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(als_pc_kernel<TT, BG, LS>), hipFuncAttributeMaxDynamicSharedMemorySize, AlsPc<TT>::LDS_B));
            hipLaunchKernelGGL((als_pc_kernel<TT, BG, LS>), dim3(pblocks), dim3(512), AlsPc<TT>::LDS_B, stream, p, wl.work.get(), items, scratch_.get(), qi_.get(),
                               wl.defer.get(), pc_err_.get());
        }); }); });
        BFH_HIP(hipGetLastError());
        if (wl.n_def > 0) {   // items with weights outside the f16 path: fp32 instruction, tiles into their scratch slots
            BFH_HIP(hipMemsetAsync(ticket_.get(), 0, sizeof(int), stream));
            launch_gram_to_slots(p, wl.dlist.get(), wl.n_def, scratch_.get(), 0, true);
        }
        if (wl.n_heavy) launch_solve(p, wl.heavy.get(), wl.n_heavy, scratch_.get(), false);
        if (wl.n_def_rows) launch_solve(p, wl.dsolve.get(), wl.n_def_rows, scratch_.get(), false);
    }

    void launch_gram_inreg(AlsParams& p, const WorkList& wl, const Plan& plan, int axis, int start_x, int nrows) {
        const int T = vdim_ / 32, items = wl.n_work;
        if (items == 0) return;
        if (plan.split) {
            prepare_split(p, axis, T, false);
            launch_rowff(p, T, start_x, nrows);
            p.batch = 16;   // rows per ticket at most (fewer where the rows are long)
        }
        const int blocks = std::min((items + 3) / 4, num_cus_ * 4);   // as launch_gram_to_slots
        dispatch_int<1, 4>(T, [&](auto tt) { dispatch_bool(plan.split, [&](auto sp) { dispatch_bool(plan.big, [&](auto bg) { dispatch_bool(plan.big || plan.loss, [&](auto ls) {
            constexpr int TT = decltype(tt)::value;
            constexpr bool SP = decltype(sp)::value, BG = decltype(bg)::value, LS = decltype(ls)::value;
            // the split form exists from T = 2; BIG is only built with the loss terms: three forms per (T, SPLIT), not four
            if constexpr ((TT >= 2 || !SP) && (LS || !BG))
                hipLaunchKernelGGL((als_gram_kernel<TT, true, true, BG, LS, SP>), dim3(blocks), dim3(256), 0, stream, p, wl.work.get(), items, scratch_.get(), 0);
        }); }); }); });
        BFH_HIP(hipGetLastError());
        if (wl.n_heavy) launch_solve(p, wl.heavy.get(), wl.n_heavy, scratch_.get(), false);   // heavy rows: their chunks' partials were summed in scratch_
    }

    void launch_gram_scratch(const AlsParams& p, const WorkList& wl, int nrows) {
        if (wl.n_work == 0) return;
        // one slot per row of the chunk, then one (zeroed) accumulation slot per heavy row
        const size_t per_row = als_slot_floats(vdim_);
        const size_t need = (static_cast<size_t>(nrows) + wl.n_heavy) * per_row;
        if (gscratch_.size() < need) gscratch_.resize(need);
        if (wl.n_heavy)
            BFH_HIP(hipMemsetAsync(gscratch_.get() + static_cast<size_t>(nrows) * per_row, 0, wl.n_heavy * per_row * sizeof(float), stream));
        launch_gram_to_slots(p, wl.work.get(), wl.n_work, gscratch_.get(), nrows, code_ == 8);
        launch_solve(p, wl.solve.get(), wl.n_solve, gscratch_.get(), true);
    }

    void launch_wide(AlsParams& p, const WorkList& wl, const Plan& plan, int axis, int start_x, int nrows) {
        const int T = vdim_ / 32;
        if (plan.split) {
            prepare_split(p, axis, T, true);
            p.Qi = qi_.get();
        }
        launch_rowff(p, T, start_x, nrows);
        auto launch = [&](const AlsWork* items, int n, int finalize) {
            dispatch_int<5, 8>(T, [&](auto tt) { dispatch_bool(plan.big, [&](auto bg) { dispatch_bool(plan.split, [&](auto sp) {
                constexpr int TT = decltype(tt)::value;
                constexpr bool BG = decltype(bg)::value, SP = decltype(sp)::value;
                if constexpr (!SP || TT <= ALS_WIDE_SPLIT_MAX_T)   // (choose_plan never asks for the split form above the limit)
                    hipLaunchKernelGGL((als_wide_kernel<TT, BG, SP>), dim3(std::max(1, std::min(n, num_cus_ * als_wide_blocks_per_cu(TT, SP)))),
                                   dim3(64 * ((TT + 1) / 2 + (SP ? 1 : 0))), als_wide_lds_bytes(vdim_, SP), stream, p, items, n, scratch_.get(), finalize);
            }); }); });
            BFH_HIP(hipGetLastError());
        };
        if (wl.n_work > 0) launch(wl.work.get(), wl.n_work, 0);
        if (wl.n_heavy) {   // heavy rows: FF + summed chunk tiles -> solve
            BFH_HIP(hipMemsetAsync(ticket_.get(), 0, sizeof(int), stream));
            launch(wl.heavy_work.get(), wl.n_heavy, 1);
        }
    }

    // als_ialspp_kernel<K, KB>: a wave per row, K = dwords per lane of a row (1, 2, 4, 8, 16), KB = of a block (1, 2).  KB outside, K ascending inside:
    // the kernels are instantiated in that order, and the compiler's output for <1, 1> is not the same when <2, 1> comes before it
    void launch_ialspp(const AlsParams& p, int nrows) {
        const int bs = block_size_ < d_ ? block_size_ : d_;
        const int KB = (bs + 63) / 64;
        if (KB > 2) throw Error(BFH_ERR_UNSUPPORTED, "block_size > 128 is not implemented on gfx950");
        int lg = 0;
        while (lg < 4 && (64 << lg) < vdim_) ++lg;
        const int waves = std::min(num_cus_ * 16, nrows);
        const dim3 grid((waves + 3) / 4), block(256);
        dispatch_int<1, 2>(KB, [&](auto kb) { dispatch_int<0, 4>(lg, [&](auto l2) {
            constexpr int KKB = decltype(kb)::value, K2 = 1 << decltype(l2)::value, KK = K2 < KKB ? KKB : K2;   // a row is never shorter than its block: (1, 2) runs as (2, 2)
            hipLaunchKernelGGL((als_ialspp_kernel<KK, KKB>), grid, block, 0, stream, p);
        }); });
    }

    // What every call ends with: loss, the pairs' error word, write-back, the one synchronisation, versions, timers, stats.
    void finish_call(const AlsParams& p, bool pairs, int axis, int start_x, int nrows, int64_t n, double* nume, double* deno) {
        double l[2] = {0, 0};
        if (compute_loss_) BFH_HIP(hipMemcpyAsync(l, loss_.get(), 2 * sizeof(double), hipMemcpyDeviceToHost, stream));
        int pe[2] = {0, 0};
        if (pairs) BFH_HIP(hipMemcpyAsync(pe, pc_err_.get(), 2 * sizeof(int), hipMemcpyDeviceToHost, stream));
        if (writeback_) {  // als.cu:403: updated rows go back to the caller's array
            float* hostF = axis == 0 ? hostP_ : hostQ_;
            const size_t off = static_cast<size_t>(start_x) * vdim_, cnt = static_cast<size_t>(nrows) * vdim_;
            copy_out(hostF + off, p.P + off, cnt * sizeof(float));
        }
        BFH_HIP(hipStreamSynchronize(stream));
        ++fver_[axis];   // the side just solved changed
        drain_aux();
        stats.kernel_ms += t_main_.drain();
        stats.launches += 1;
        stats.samples += n;
        if (pairs) {
            pc_same_simd_ = pe[1];
            if (pe[0] & 1) throw Error(BFH_ERR_HIP, "als_pc_kernel: a producer / consumer hand-off timed out (results of this call are invalid)");
            if (pe[0] & 2) throw Error(BFH_ERR_HIP, "als_pc_kernel: a weight outside the f16 path reached the kernel (stale weight scan)");
        }
        *nume = l[0];
        *deno = l[1];
    }

    // Which work items hold weights the split pass cannot carry (als_defer_scan_kernel)?  Depends on the chunk's values only, so it is
    // kept with the work list and redone when values were uploaded since (or the cut moved); the one host round trip it costs buys
    // launch shapes the host knows.
    void scan_deferred(WorkList& wl, const AlsParams& p, int items) {
        if (wl.scan_ver == vals_ver_ && wl.scan_wcut == split_wcut_ && wl.scan_vals == p.vals) return;
        if (wl.defer.size() < static_cast<size_t>(items)) {
            wl.defer.resize(items);
            wl.dlist.resize(items);
            wl.dsolve.resize(items);
            wl.dcount.resize(2);
        }
        BFH_HIP(hipMemsetAsync(wl.dcount.get(), 0, 2 * sizeof(int), stream));
        hipLaunchKernelGGL(als_defer_scan_kernel, dim3((items + 3) / 4), dim3(256), 0, stream, wl.work.get(), items, p.vals, p.alpha, split_wcut_, wl.n_heavy,
                           wl.defer.get(), wl.dlist.get(), wl.dsolve.get(), wl.dcount.get());
        BFH_HIP(hipGetLastError());
        int c[2] = {0, 0};
        BFH_HIP(hipMemcpyAsync(c, wl.dcount.get(), 2 * sizeof(int), hipMemcpyDeviceToHost, stream));
        BFH_HIP(hipStreamSynchronize(stream));
        wl.n_def = c[0];
        wl.n_def_rows = c[1];
        wl.scan_ver = vals_ver_;
        wl.scan_wcut = split_wcut_;
        wl.scan_vals = p.vals;
        const size_t need = std::max<size_t>(1, static_cast<size_t>(wl.n_heavy) + (wl.n_def_rows <= 4096 ? wl.n_def_rows : 0)) * als_slot_floats(vdim_);
        if (scratch_.size() < need) scratch_.resize(need);   // grow-only, neither copied nor zeroed: partial_update zeroes the slots of every call after this
    }

    // Everything bfh_als_fold_in refuses, before anything is uploaded or launched.  The key check is a host scan of all nnz keys.
    void fold_check(int axis, int n_rows, const int64_t* indptr, const int32_t* keys, const float* vals, int64_t nnz) const {
        BFH_REQUIRE(axis == 0 || axis == 1, "fold_in: axis must be 0 or 1");
        BFH_REQUIRE(n_rows >= 0, "fold_in: n_rows is negative");
        BFH_REQUIRE(nnz >= 0, "fold_in: nnz is negative");
        BFH_REQUIRE(n_rows == 0 || indptr, "fold_in: null indptr");
        BFH_REQUIRE(nnz == 0 || (keys && vals), "fold_in: null keys / vals with nnz > 0");
        int64_t prev = 0;
        for (int b = 0; b < n_rows; ++b) {
            BFH_REQUIRE(indptr[b] >= prev, "fold_in: indptr decreases at row " + std::to_string(b));
            prev = indptr[b];
        }
        BFH_REQUIRE(prev == nnz, "fold_in: indptr[n_rows - 1] != nnz");
        const int op_rows = axis == 0 ? Q_rows_ : P_rows_;
        for (int64_t i = 0; i < nnz; ++i)
            if (keys[i] < 0 || keys[i] >= op_rows)
                throw Error(BFH_ERR_INVALID, "fold_in: key " + std::to_string(keys[i]) + " at position " + std::to_string(i) + " is outside [0, " +
                                                 std::to_string(op_rows) + ")");
    }

    // The fold-in Gramian of the factor the rows are solved against, recomputed only when that factor has changed (fver_)
    void fold_gramian(int axis) {
        FoldState& f = fold_;
        const int oside = axis == 0 ? 1 : 0;
        const size_t nff = static_cast<size_t>(vdim_) * vdim_;
        if (f.ff[axis].size() == nff && f.ff_ver[axis] == fver_[oside]) return;
        f.ff[axis].resize(nff);
        f.ff64.resize(nff);
        gramian_into(axis == 0 ? Q_.get() : P_.get(), axis == 0 ? Q_rows_ : P_rows_, f.ff64, f.ff[axis]);
        f.ff_ver[axis] = fver_[oside];
    }

    // One sub-batch of a fold_in call: rows [r0, r1), their entries from `beg`, and where their work items / solve entries lie in the call's lists
    struct FoldBatch {
        int r0, r1;
        int64_t beg;
        size_t work_off, solve_off;
        int n_work, n_solve, n_heavy;
    };
    // Cuts the call's rows into sub-batches whose slots (one per row + one per row above HEAVY entries) fit fold_slot_bytes_ -- at least one row
    // each -- and whose entries fit the work items' 32-bit positions; builds and uploads every sub-batch's work items (longest first) and
    // solve list (slot = row - r0, heavy slots behind), and sizes the slot scratch.  Row b's work items and slot contents do not depend on the cuts.
    std::vector<FoldBatch> fold_plan(int n_rows, const int64_t* indptr) {
        FoldState& f = fold_;
        const size_t slot_bytes = als_slot_floats(vdim_) * sizeof(float);
        const int64_t max_slots = std::max<int64_t>(1, fold_slot_bytes_ / static_cast<int64_t>(slot_bytes));
        constexpr int64_t MAX_ENTRIES = int64_t(1) << 30;
        std::vector<FoldBatch> batches;
        std::vector<AlsWork> work;
        std::vector<AlsHeavy> solve;
        int64_t slots_needed = 1;
        int r0 = 0;
        while (r0 < n_rows) {
            const int64_t beg = r0 == 0 ? 0 : indptr[r0 - 1];
            int r1 = r0;
            int64_t slots = 0;
            while (r1 < n_rows) {
                const int64_t n = indptr[r1] - (r1 == 0 ? 0 : indptr[r1 - 1]);
                const int64_t s = 1 + (n > HEAVY ? 1 : 0);
                if (r1 > r0 && (slots + s > max_slots || indptr[r1] - beg > MAX_ENTRIES)) break;
                slots += s;
                ++r1;
            }
            BFH_REQUIRE(indptr[r1 - 1] - beg < (int64_t(1) << 31), "fold_in: a row of 2^31 entries or more");
            FoldBatch b{r0, r1, beg, work.size(), solve.size(), 0, 0, 0};
            for (int x = r0; x < r1; ++x) {
                const int64_t prev = x == 0 ? 0 : indptr[x - 1], n = indptr[x] - prev;
                if (n == 0) continue;   // an empty history: the zero row
                const int heavy_slot = n > HEAVY ? b.n_heavy++ : -1;
                push_row_items(work, x, prev - beg, n, heavy_slot);
                solve.push_back({x, heavy_slot < 0 ? x - r0 : (r1 - r0) + heavy_slot, n});
            }
            std::stable_sort(work.begin() + b.work_off, work.end(), [](const AlsWork& a, const AlsWork& c) { return (a.kend - a.kbeg) > (c.kend - c.kbeg); });
            std::stable_sort(solve.begin() + b.solve_off, solve.end(), [](const AlsHeavy& a, const AlsHeavy& c) { return a.n > c.n; });
            b.n_work = static_cast<int>(work.size() - b.work_off);
            b.n_solve = static_cast<int>(solve.size() - b.solve_off);
            slots_needed = std::max<int64_t>(slots_needed, (r1 - r0) + b.n_heavy);
            batches.push_back(b);
            r0 = r1;
        }
        grow(f.work, std::max<size_t>(1, work.size()));
        grow(f.solve, std::max<size_t>(1, solve.size()));
        grow(f.slots, static_cast<size_t>(slots_needed) * als_slot_floats(vdim_));
        if (!work.empty()) BFH_HIP(hipMemcpyAsync(f.work.get(), work.data(), work.size() * sizeof(AlsWork), hipMemcpyHostToDevice, stream));
        if (!solve.empty()) BFH_HIP(hipMemcpyAsync(f.solve.get(), solve.data(), solve.size() * sizeof(AlsHeavy), hipMemcpyHostToDevice, stream));
        BFH_HIP(hipStreamSynchronize(stream));   // the two vectors end with this function
        stats.h2d_bytes += static_cast<double>(work.size() * sizeof(AlsWork) + solve.size() * sizeof(AlsHeavy));
        return batches;
    }

    struct Axis {
        std::vector<int64_t> indptr_host;
        DevBuf<int64_t> indptr;
        DevBuf<int32_t> keys;
        DevBuf<float> vals;
        bool resident = false;
        std::map<std::pair<int, int>, std::pair<int64_t, uint64_t>> chunks;   // auto-residency: row range -> (length, checksum)
    };
    // device -> the caller's array: through the library's own pinned ring (HostStager, common.hpp) unless the caller asked for its arrays
    // to be registered ("pin_host" = 1); an array that is no longer mapped is an error, not a fault
    void copy_out(void* dst, const void* src_dev, size_t bytes) {
        if (!host_range_mapped(dst, bytes)) throw Error(BFH_ERR_INVALID, "the caller's factor array is no longer mapped (freed while the model still writes to it?)");
        if (!pinned_.empty()) BFH_HIP(hipMemcpyAsync(dst, src_dev, bytes, hipMemcpyDeviceToHost, stream));
        else stager_.d2h(dst, src_dev, bytes, stream, device);
        stats.d2h_bytes += static_cast<double>(bytes);
    }
    HostStager stager_;
    void unpin_host() {
        if (!pinned_.empty() && stream) (void)hipStreamSynchronize(stream);   // (see SgdHandle::unpin_host)
        for (void* q : pinned_) (void)hipHostUnregister(q);
        if (!pinned_.empty()) (void)hipGetLastError();
        pinned_.clear();
    }
    std::vector<void*> pinned_;
    bool auto_resident_ = true, pin_host_ = false;   // pin_host: opt-in since round 5 (HostStager, common.hpp)

    bool model_ = false, placeholder_ = false, writeback_ = true;
    int P_rows_ = 0, Q_rows_ = 0, block_size_ = 32;
    bool adaptive_reg_ = false, compute_loss_ = false;
    float *hostP_ = nullptr, *hostQ_ = nullptr;
    DevBuf<float> P_, Q_, vals_, yui_;
    DevBuf<int32_t> keys_;
    Axis ax_[2];
    bool wide_split_ = true;
    bool no_inreg_ = false;
    bool split_f16_ = true;
    int pc_ = 1;
    // the split-f16 wide kernel up to vdim 32 * this.  Measured (profiles/r06_als_wide_split_192_256.txt, ML-20M, ms per epoch of row kernels, split | fp32):
    // d = 192 11.8 | 23.1, d = 224 23.3 | 26.0, d = 256 37.0 | 30.6 -- above T = 6 a CU holds ONE workgroup (128 / 144 accumulators want 256 registers) and
    // the producer's three row sets spill (110 registers at T = 7, 600 at T = 8): T = 8 stays on the fp32 instruction
    static constexpr int ALS_WIDE_SPLIT_MAX_T = 7;
    float split_wcut_ = 32768.0f;
    uint64_t fver_[2] = {1, 1};     // bumped whenever P (0) / Q (1) may have changed on the device
    uint64_t vals_ver_ = 1;         // bumped whenever confidence values were uploaded
    DevBuf<float> qi_;              // block-interleaved copy of the other factor (als_interleave_stats_kernel)
    int qi_side_ = -1;
    uint64_t qi_ver_ = 0;
    float qi_wcut_ = -1.f;
    DevBuf<int> pc_err_;
    int pc_same_simd_ = 0;
    Plan last_plan_;
    DevBuf<float> split_part_;
    DevBuf<float> split_out_;
    DevBuf<float> rowff_;
    DevBuf<float> gscratch_;        // launch_gram_scratch: one slot per row of the call + one per heavy row
    DevBuf<float> scratch_;         // the fused kernels: one slot per heavy (pairs: and deferred) row
    // fold_in's own state: nothing here is read or written by a training call, nothing of the training state above is written by fold_in
    struct FoldState {
        DevBuf<float> ff[2];              // the fold-in Gramians: [0] Q^T Q (axis 0), [1] P^T P (axis 1) ...
        uint64_t ff_ver[2] = {0, 0};      // ... and the fver_ of that factor they were formed at
        DevBuf<double> ff64;              // fp64 accumulator of gramian_into
        DevBuf<float> out;                // [rows, vdim]: device buffer "fold"
        int rows = 0;
        DevBuf<int32_t> keys;
        DevBuf<float> vals;
        DevBuf<AlsWork> work;
        DevBuf<AlsHeavy> solve;
        DevBuf<float> slots;              // one sub-batch's slots, at most fold_slot_bytes_ (or one row's)
        DevBuf<int> ticket;
        EventTimer t_solve;
    };
    FoldState fold_;
    bool fold_solve_ = true;
    int64_t fold_slot_bytes_ = int64_t(512) << 20;
    Comm* comm_ = nullptr;   // not owned
};

}  // namespace bfh
