// CFR (CoFactor) on gfx950 -- handle + the small kernels that are not shared with ALS.
//
// Reference semantics: CCFR (/root/reference/lib/algo_impl/cfr/cfr.cc:29-313) behind CyCFR's surface
// (/root/reference/buffalo/algo/_cfr.pyx:25-71); SURVEY.md section 8(f) rank 4: "CFR calls the same
// _leastsquare".  The three row updates are instances of the ALS dense path (als_gram_kernel ->
// scratch slot -> als_solve_kernel / als_dense_solve):
//   user     A = l (FF_I + sum alpha v i i^T) + reg_u I,                         y = l sum (1 + alpha v) i
//   item     A = l (FF_U + sum alpha v u u^T) + sum c c^T + reg_i I,             y = l sum (1 + alpha v) u + sum (v - Ib_x - Cb_c) c
//   context  A = sum i i^T + reg_c I,                                            y = sum (v - Cb_x - Ib_i) i
// -- the item system is built by two Gramian passes adding into one slot (p.accumulate, p.out_scale,
// p.ctx) -- followed by the bias refresh from the UPDATED row (cfr.cc:244-250, 303-309).
// Host arrays are [rows, d] unpadded (the reference's CPU layout); the device copies are padded to vdim.
// CfrHandle derives from AlsCore (als_core.hpp): options, Gramian and the slot path come from there, the rest is its own.
#pragma once
#include "als_core.hpp"
#include "cfr_fold_kernels.hpp"

namespace bfh {

// b[x] = sum_k (v_k - F[x].G[key_k] - bias_other[key_k]) / (n + 1e-10) over the row's entries; one wave per row.
// `indptr_also`: rows that were solved because of entries in a second matrix get 0 / 1e-10 = 0 when they have none here
// (cfr.cc:244-250 runs for every item that was not skipped at :177-180).
__global__ __launch_bounds__(256) void cfr_bias_kernel(const float* __restrict__ F, const float* __restrict__ G, int vdim, const int64_t* __restrict__ indptr,
                                                       int64_t shift, int start_x, int next_x, const int32_t* __restrict__ keys,
                                                       const float* __restrict__ vals, const float* __restrict__ bias_other, float* __restrict__ bias_self,
                                                       const int64_t* __restrict__ indptr_also) {
    const int lane = threadIdx.x & 63;
    const int x = start_x + static_cast<int>((static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6);
    if (x >= next_x) return;
    const int64_t beg = row_begin(indptr, x) - shift, end = indptr[x] - shift;
    if (end == beg) {
        if (indptr_also && lane == 0 && indptr_also[x] - row_begin(indptr_also, x) > 0) bias_self[x] = 0.f;
        return;
    }
    const float* fx = F + static_cast<size_t>(x) * vdim;
    float b = 0.f;
    for (int64_t k = beg; k < end; ++k) {
        const int c = keys[k];
        b += vals[k] - wave_dot(fx, G + static_cast<size_t>(c) * vdim, vdim, lane) - bias_other[c];
    }
    if (lane == 0) bias_self[x] = b / (static_cast<float>(end - beg) + 1e-10f);
}

// out += scale * sum_x |F[x]|^2 over rows of [start_x, next_x) that have entries in `indptr` (or in `indptr2`)
__global__ __launch_bounds__(256) void cfr_sqnorm_kernel(const float* __restrict__ F, int vdim, const int64_t* __restrict__ indptr,
                                                         const int64_t* __restrict__ indptr2, int start_x, int next_x, double scale, double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int x = start_x + static_cast<int>((static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6);
    if (x >= next_x) return;
    const bool has = indptr[x] - row_begin(indptr, x) > 0 || (indptr2 && indptr2[x] - row_begin(indptr2, x) > 0);
    if (!has) return;
    const float* fx = F + static_cast<size_t>(x) * vdim;
    const float part = wave_dot(fx, fx, vdim, lane);
    if (lane == 0) atomicAdd(out, scale * static_cast<double>(part));
}

// item loss terms of cfr.cc:176-190, 212-228 on the row BEFORE its update; one wave per row
__global__ __launch_bounds__(256) void cfr_item_loss_kernel(const float* __restrict__ I, const float* __restrict__ U, const float* __restrict__ C,
                                                            const float* __restrict__ FF, int d, int vdim, const int64_t* __restrict__ ip_u,
                                                            int64_t shift_u, const int32_t* __restrict__ keys_u, const float* __restrict__ vals_u,
                                                            const int64_t* __restrict__ ip_c, int64_t shift_c, const int32_t* __restrict__ keys_c,
                                                            const float* __restrict__ vals_c, const float* __restrict__ Ib, const float* __restrict__ Cb,
                                                            int start_x, int next_x, float alpha, float l, float reg_i, double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int x = start_x + static_cast<int>((static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6);
    if (x >= next_x) return;
    const int64_t bu = row_begin(ip_u, x) - shift_u, eu = ip_u[x] - shift_u;
    const int64_t bc = row_begin(ip_c, x) - shift_c, ec = ip_c[x] - shift_c;
    if (eu == bu && ec == bc) return;
    const float* ix = I + static_cast<size_t>(x) * vdim;
    auto dot = [&](const float* a, const float* b) { return wave_dot(a, b, vdim, lane); };
    float loss = 0.f;
    {   // (I_x FF) . I_x
        float part = 0.f;
        for (int i = lane; i < d; i += 64) {
            float t = 0.f;
            for (int j = 0; j < d; ++j) t += ix[j] * FF[static_cast<size_t>(j) * vdim + i];
            part += t * ix[i];
        }
        loss += wave_sum(part);
    }
    for (int64_t k = bu; k < eu; ++k) {
        const float w = vals_u[k] * alpha;
        const float dt = dot(ix, U + static_cast<size_t>(keys_u[k]) * vdim);
        loss += (-dt * dt + (1 + w) * (dt - 1) * (dt - 1));
    }
    double total = static_cast<double>(loss * l);
    loss = 0.f;
    for (int64_t k = bc; k < ec; ++k) {
        const int c = keys_c[k];
        const float err = vals_c[k] - dot(ix, C + static_cast<size_t>(c) * vdim) - Ib[x] - Cb[c];
        loss += err * err;
    }
    total += static_cast<double>(loss) + static_cast<double>(reg_i * dot(ix, ix));
    if (lane == 0) atomicAdd(out, total);
}

class CfrHandle : public AlsCore {
 public:   // the entry points of als.hip
    bool init(const char* opt_path) {
        if (!init_common(opt_path, 128, 2)) return false;
        l_ = static_cast<float>(opt_.num("l"));
        reg_c_ = static_cast<float>(opt_.num("reg_c"));
        eps_ = static_cast<float>(opt_.num_or("eps", 1e-10));
        cg_tol_ = static_cast<float>(opt_.num_or("cg_tolerance_", 0.0));   // sic (cfr.cc:38): the key nobody sets
        num_cg_max_iters_ = static_cast<int>(opt_.num_or("num_cg_max_iters", 3));
        cfr_loss_ = opt_.boolean_or("compute_loss", false);                // cfr.cc:44
        const std::string optimizer = opt_.str("optimizer");
        if (optimizer == "llt") code_ = 0;
        else if (optimizer == "ldlt") code_ = 1;
        else if (optimizer == "manual_cg") code_ = 2;
        else throw Error(BFH_ERR_UNSUPPORTED, "optimizer '" + optimizer + "' is not implemented on gfx950 (supported: llt, ldlt, manual_cg)");
        work_cache_.clear();   // init on a used handle: nothing of the previous model's matrices survives
        inited_ = true;
        return true;
    }

    // cfr.cc:70-82: binds the caller's array; the device copy is padded to vdim
    void set_embedding(float* data, int size, const std::string& t) {
        BFH_REQUIRE(inited_, "set_embedding called before init");
        BFH_REQUIRE(data && size > 0, "set_embedding: null array or empty shape");
        Emb& e = emb(t);
        const bool bias = t == "item_bias" || t == "context_bias";
        e.host = data; e.rows = size; e.cols = bias ? 1 : d_;
        const int ld = e.ld = bias ? 1 : vdim_;
        e.dev.resize(static_cast<size_t>(size) * ld, true, stream);
        stats.h2d_bytes += rows_to_device(e.dev.get(), ld, data, e.cols, 0, size, stream);
        BFH_HIP(hipStreamSynchronize(stream));
        ++e.ver;
        fold_.rows = fold_.bias_rows = 0;   // the rows of an earlier fold_in belong to the arrays they were folded against
    }
    // cfr.cc:85-90
    void precompute(const std::string& t) {
        BFH_REQUIRE(t == "user" || t == "item", "precompute: obj_type must be user or item");
        Emb& e = emb(t);
        BFH_REQUIRE(e.host, "precompute before set_embedding");
        gramian_of(e.dev.get(), e.rows);
    }

    // cfr.cc:92-146
    double partial_update_user(int start_x, int next_x, const int64_t* indptr, const int32_t* keys, const float* vals) {
        BFH_REQUIRE(U_.host && I_.host, "partial_update_user before set_embedding(user / item)");
        BFH_REQUIRE(0 <= start_x && start_x <= next_x && next_x <= U_.rows, "partial_update_user: bad row range");
        if (next_x == start_x) return 0.0;
        upload(cu_, start_x, next_x, indptr, keys, vals);
        const int slot = t_main_.begin(stream);
        AlsParams p = base_params(U_, I_, cu_, start_x, next_x, reg_u_);
        p.out_scale = l_; p.ff_scale = l_;
        zero_slots(next_x - start_x);
        p.accumulate = 1;
        gram_pass(p, WorkId::CfrUser, cu_, start_x, next_x);
        solve_rows(p, start_x, next_x, indptr, nullptr);
        BFH_HIP(hipMemsetAsync(loss_.get(), 0, 2 * sizeof(double), stream));
        if (cfr_loss_)   // reg_u * |U_x|^2 of the UPDATED rows (cfr.cc:139-140)
            hipLaunchKernelGGL(cfr_sqnorm_kernel, dim3(wave_blocks(next_x - start_x)), dim3(256), 0, stream, U_.dev.get(), vdim_, cu_.indptr.get(), nullptr,
                               start_x, next_x, static_cast<double>(reg_u_), loss_.get());
        t_main_.end(slot, stream);
        write_back(U_, start_x, next_x);
        const double loss = read_loss();
        stats.kernel_ms += t_main_.drain();
        stats.samples += cu_.nnz;
        ++U_.ver;   // fold_in's U^T U is stale
        return loss;
    }
    // cfr.cc:148-255
    double partial_update_item(int start_x, int next_x, const int64_t* ip_u, const int32_t* keys_u, const float* vals_u, const int64_t* ip_c,
                               const int32_t* keys_c, const float* vals_c) {
        BFH_REQUIRE(U_.host && I_.host && C_.host && Ib_.host && Cb_.host, "partial_update_item before set_embedding of all five arrays");
        BFH_REQUIRE(0 <= start_x && start_x <= next_x && next_x <= I_.rows, "partial_update_item: bad row range");
        if (next_x == start_x) return 0.0;
        upload(ciu_, start_x, next_x, ip_u, keys_u, vals_u);
        upload(cic_, start_x, next_x, ip_c, keys_c, vals_c);
        const int slot = t_main_.begin(stream);
        BFH_HIP(hipMemsetAsync(loss_.get(), 0, 2 * sizeof(double), stream));
        if (cfr_loss_)
            hipLaunchKernelGGL(cfr_item_loss_kernel, dim3(wave_blocks(next_x - start_x)), dim3(256), 0, stream, I_.dev.get(), U_.dev.get(), C_.dev.get(),
                               FF_.get(), d_, vdim_, ciu_.indptr.get(), ciu_.shift, ciu_.keys.get(), ciu_.vals.get(), cic_.indptr.get(), cic_.shift,
                               cic_.keys.get(), cic_.vals.get(), Ib_.dev.get(), Cb_.dev.get(), start_x, next_x, alpha_, l_, reg_i_, loss_.get());
        zero_slots(next_x - start_x);
        AlsParams pu = base_params(I_, U_, ciu_, start_x, next_x, reg_i_);   // user-item part, weighted by l
        pu.out_scale = l_; pu.ff_scale = l_; pu.accumulate = 1;
        gram_pass(pu, WorkId::CfrItemUsers, ciu_, start_x, next_x);
        AlsParams pc = base_params(I_, C_, cic_, start_x, next_x, reg_i_);   // item-context part
        pc.ctx = 1; pc.bias_self = Ib_.dev.get(); pc.bias_other = Cb_.dev.get(); pc.accumulate = 1; pc.ff_scale = l_;
        gram_pass(pc, WorkId::CfrItemContexts, cic_, start_x, next_x);
        solve_rows(pc, start_x, next_x, ip_u, ip_c);
        hipLaunchKernelGGL(cfr_bias_kernel, dim3(wave_blocks(next_x - start_x)), dim3(256), 0, stream, I_.dev.get(), C_.dev.get(), vdim_, cic_.indptr.get(),
                           cic_.shift, start_x, next_x, cic_.keys.get(), cic_.vals.get(), Cb_.dev.get(), Ib_.dev.get(), ciu_.indptr.get());
        BFH_HIP(hipGetLastError());
        t_main_.end(slot, stream);
        write_back(I_, start_x, next_x);
        write_back(Ib_, start_x, next_x);
        const double loss = read_loss();
        stats.kernel_ms += t_main_.drain();
        stats.samples += ciu_.nnz + cic_.nnz;
        ++I_.ver;   // fold_in's I^T I is stale
        return loss;
    }
    // cfr.cc:257-313
    double partial_update_context(int start_x, int next_x, const int64_t* indptr, const int32_t* keys, const float* vals) {
        BFH_REQUIRE(I_.host && C_.host && Ib_.host && Cb_.host, "partial_update_context before set_embedding(item, context, biases)");
        BFH_REQUIRE(0 <= start_x && start_x <= next_x && next_x <= C_.rows, "partial_update_context: bad row range");
        if (next_x == start_x) return 0.0;
        upload(cc_, start_x, next_x, indptr, keys, vals);
        const int slot = t_main_.begin(stream);
        BFH_HIP(hipMemsetAsync(loss_.get(), 0, 2 * sizeof(double), stream));
        if (cfr_loss_)   // reg_c * |C_x|^2 of the rows BEFORE the update (cfr.cc:297-298)
            hipLaunchKernelGGL(cfr_sqnorm_kernel, dim3(wave_blocks(next_x - start_x)), dim3(256), 0, stream, C_.dev.get(), vdim_, cc_.indptr.get(), nullptr,
                               start_x, next_x, static_cast<double>(reg_c_), loss_.get());
        zero_slots(next_x - start_x);
        AlsParams p = base_params(C_, I_, cc_, start_x, next_x, reg_c_);
        p.ctx = 1; p.bias_self = Cb_.dev.get(); p.bias_other = Ib_.dev.get(); p.accumulate = 1; p.ff_scale = 0.0f;
        gram_pass(p, WorkId::CfrContext, cc_, start_x, next_x);
        solve_rows(p, start_x, next_x, indptr, nullptr);
        hipLaunchKernelGGL(cfr_bias_kernel, dim3(wave_blocks(next_x - start_x)), dim3(256), 0, stream, C_.dev.get(), I_.dev.get(), vdim_, cc_.indptr.get(),
                           cc_.shift, start_x, next_x, cc_.keys.get(), cc_.vals.get(), Ib_.dev.get(), Cb_.dev.get(), nullptr);
        BFH_HIP(hipGetLastError());
        t_main_.end(slot, stream);
        write_back(C_, start_x, next_x);
        write_back(Cb_, start_x, next_x);
        const double loss = read_loss();
        stats.kernel_ms += t_main_.drain();
        stats.samples += cc_.nnz;
        return loss;
    }

    // ---- fold-in: rows and biases for users, items and contexts that are not in the model (bfh_cfr_fold_in; the rule is stated in
    // include/buffalo_hip.h and at the head of cfr_fold_kernels.hpp) ---------------------------------------------------------------------
    // Steps: refuse bad input on the host -> the fold-in Gramian of the factor part a gathers (kept per kind while that factor does not
    // change) -> upload -> the non-empty rows, longest first -> ONE launch of cfr_fold_kernel -> copy out, or leave the rows in "fold" /
    // "fold_bias".  Everything it writes is its own (FoldState); of the model it reads the device copies of the arrays the kind gathers.
    void fold_in(const std::string& t, int n_rows, const int64_t* ip_a, const int32_t* keys_a, const float* vals_a, int64_t nnz_a, const int64_t* ip_c,
                 const int32_t* keys_c, const float* vals_c, int64_t nnz_c, int iters, const float* init_bias, float* out, float* out_bias) {
        BFH_REQUIRE(inited_, "fold_in before init");
        const int kind = t == "user" ? 0 : t == "item" ? 1 : t == "context" ? 2 : -1;
        BFH_REQUIRE(kind >= 0, "fold_in: unknown obj_type '" + t + "' (user, item, context)");
        const Emb* Ya = kind == 0 ? &I_ : kind == 1 ? &U_ : nullptr;   // part a gathers it (and needs its Gramian)
        const Emb* Gc = kind == 1 ? &C_ : kind == 2 ? &I_ : nullptr;   // part c gathers it ...
        const Emb* Bc = kind == 1 ? &Cb_ : kind == 2 ? &Ib_ : nullptr; // ... and this bias beside it
        fold_check(t, n_rows, Ya, ip_a, keys_a, vals_a, nnz_a, Gc, Bc, ip_c, keys_c, vals_c, nnz_c, iters, init_bias, out_bias);
        FoldState& f = fold_;
        f.rows = n_rows;
        f.bias_rows = kind == 0 ? 0 : n_rows;
        if (n_rows == 0) return;
        if (Ya) fold_gramian(kind, *Ya);
        // out: zero (the empty rows and the padding columns stay so); bias: init_bias (an empty row keeps it), or zero
        const size_t nout = static_cast<size_t>(n_rows) * vdim_;
        grow(f.out, nout);
        grow(f.bias, static_cast<size_t>(n_rows));
        BFH_HIP(hipMemsetAsync(f.out.get(), 0, nout * sizeof(float), stream));
        if (init_bias) {
            BFH_HIP(hipMemcpyAsync(f.bias.get(), init_bias, n_rows * sizeof(float), hipMemcpyHostToDevice, stream));
            stats.h2d_bytes += 4.0 * n_rows;
        } else BFH_HIP(hipMemsetAsync(f.bias.get(), 0, n_rows * sizeof(float), stream));
        fold_upload(f.keys_a, f.vals_a, keys_a, vals_a, nnz_a);
        fold_upload(f.keys_c, f.vals_c, keys_c, vals_c, nnz_c);
        const int n_list = fold_list(n_rows, nnz_a ? ip_a : nullptr, nnz_c ? ip_c : nullptr);
        if (n_list) {
            CfrFoldParams p{};
            if (Ya) { p.Ya = Ya->dev.get(); p.FF = f.ff[kind].get(); }
            if (Gc) { p.Gc = Gc->dev.get(); p.Bc = Bc->dev.get(); }
            p.keys_a = f.keys_a.get(); p.vals_a = f.vals_a.get(); p.keys_c = f.keys_c.get(); p.vals_c = f.vals_c.get();
            p.out = f.out.get();
            p.bias = kind == 0 ? nullptr : f.bias.get();
            p.d = d_; p.iters = iters; p.alpha = alpha_; p.l = l_;
            p.reg = kind == 0 ? reg_u_ : kind == 1 ? reg_i_ : reg_c_;
            const int slot = t_main_.begin(stream);
            dispatch_int<1, 4>(vdim_ / 32, [&](auto tt) {
                constexpr int TT = decltype(tt)::value;
                const size_t lds = cfr_fold_lds_bytes(TT);
                BFH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(cfr_fold_kernel<TT>), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
                hipLaunchKernelGGL(cfr_fold_kernel<TT>, dim3(std::min(n_list, num_cus_ * cfr_fold_blocks_per_cu(TT))), dim3(256), lds, stream, p, f.list.get(), n_list);
            });
            BFH_HIP(hipGetLastError());
            t_main_.end(slot, stream);
        }
        if (out) stats.d2h_bytes += rows_to_host(out, d_, f.out.get(), vdim_, 0, n_rows, stream);
        if (out_bias) stats.d2h_bytes += rows_to_host(out_bias, 1, f.bias.get(), 1, 0, n_rows, stream);
        BFH_HIP(hipStreamSynchronize(stream));
        drain_aux();
        stats.kernel_ms += t_main_.drain();
        stats.samples += nnz_a + nnz_c;
        stats.launches += 1;
    }

    int vdim() const { return vdim_; }
    int dim() const { return d_; }
    void device_buffer(const std::string& name, void** p, size_t* bytes) {
        BFH_REQUIRE(p && bytes, "device_buffer: null output");
        if (name == "fold") {   // the rows of the last fold_in (which returned with the stream drained)
            *p = fold_.rows ? fold_.out.get() : nullptr;
            *bytes = static_cast<size_t>(fold_.rows) * vdim_ * sizeof(float);
        } else if (name == "fold_bias") {   // ... and their biases (none after a fold_in of users)
            *p = fold_.bias_rows ? fold_.bias.get() : nullptr;
            *bytes = static_cast<size_t>(fold_.bias_rows) * sizeof(float);
        } else {
            Emb& e = emb(name);   // (an unknown name is refused there)
            BFH_REQUIRE(e.host, "device_buffer before set_embedding(" + name + ")");
            BFH_HIP(hipStreamSynchronize(stream));   // whoever takes the pointer reads it on another stream
            *p = e.dev.get();
            *bytes = e.dev.bytes();
        }
    }

 private:
    struct Emb {
        float* host = nullptr;
        int rows = 0, cols = 0;   // cols: d for factor matrices, 1 for biases
        int ld = 1;               // row pitch of the device copy: vdim for factor matrices (d = 1 included), 1 for biases
        uint64_t ver = 0;         // moves whenever the device copy changes (set_embedding, the matching partial_update_*): fold_in's Gramians follow it
        DevBuf<float> dev;
    };
    Emb& emb(const std::string& t) {
        if (t == "user") return U_;
        if (t == "item") return I_;
        if (t == "context") return C_;
        if (t == "item_bias") return Ib_;
        if (t == "context_bias") return Cb_;
        throw Error(BFH_ERR_INVALID, "unknown embedding '" + t + "' (user, item, context, item_bias, context_bias)");
    }
    void write_back(Emb& e, int start_x, int next_x) {   // rows [start_x, next_x) -> the caller's array
        stats.d2h_bytes += rows_to_host(e.host, e.cols, e.dev.get(), e.ld, start_x, next_x, stream);
    }
    struct Csr {   // one chunk on the device
        DevBuf<int64_t> indptr;
        DevBuf<int32_t> keys;
        DevBuf<float> vals;
        int64_t shift = 0, nnz = 0;
        const int64_t* host_ip = nullptr;
    };
    void upload(Csr& c, int start_x, int next_x, const int64_t* indptr, const int32_t* keys, const float* vals) {
        // the reference hands the FULL indptr (end offsets) + the chunk's keys/vals (buffered_data.py:99-118)
        const int64_t beg = start_x == 0 ? 0 : indptr[start_x - 1];
        const int64_t end = next_x == 0 ? 0 : indptr[next_x - 1];
        c.shift = beg; c.nnz = end - beg; c.host_ip = indptr;
        c.indptr.resize(std::max<size_t>(c.indptr.size(), next_x));
        BFH_HIP(hipMemcpyAsync(c.indptr.get(), indptr, sizeof(int64_t) * next_x, hipMemcpyHostToDevice, stream));
        c.keys.resize(std::max<size_t>(c.keys.size(), std::max<int64_t>(c.nnz, 1)));
        c.vals.resize(std::max<size_t>(c.vals.size(), std::max<int64_t>(c.nnz, 1)));
        if (c.nnz) {
            BFH_HIP(hipMemcpyAsync(c.keys.get(), keys, sizeof(int32_t) * c.nnz, hipMemcpyHostToDevice, stream));
            BFH_HIP(hipMemcpyAsync(c.vals.get(), vals, sizeof(float) * c.nnz, hipMemcpyHostToDevice, stream));
        }
        stats.h2d_bytes += 8.0 * next_x + 8.0 * c.nnz;
    }

    AlsParams base_params(Emb& self, Emb& other, Csr& c, int start_x, int next_x, float reg) {
        AlsParams p{};
        p.P = self.dev.get(); p.Q = other.dev.get(); p.FF = FF_.get();
        p.indptr = c.indptr.get(); p.keys = c.keys.get(); p.vals = c.vals.get(); p.shift = c.shift;
        p.start_x = start_x; p.next_x = next_x; p.d = d_; p.vdim = vdim_; p.op_rows = other.rows; p.block_size = 32;
        p.alpha = alpha_; p.reg = reg; p.eps = eps_; p.cg_tol = cg_tol_; p.num_cg_max_iters = num_cg_max_iters_;
        p.loss = loss_.get(); p.ticket = ticket_.get(); p.solver = static_cast<int>(code_);
        p.out_scale = 1.0f; p.ff_scale = 1.0f;
        return p;
    }
    // one Gramian pass of the chunk's rows into the slots (row - start_x)
    void gram_pass(const AlsParams& p0, WorkId id, const Csr& c, int start_x, int next_x) {
        const WorkList& wl = work_list(id, start_x, next_x, c.host_ip, c.shift, true);   // the caller's indptr: another matrix may come with any call
        if (wl.n_work == 0) return;
        BFH_HIP(hipMemsetAsync(ticket_.get(), 0, sizeof(int), stream));
        launch_gram_to_slots(p0, wl.work.get(), wl.n_work, slots_.get(), next_x - start_x, false);
    }
    void zero_slots(int nrows) {
        const size_t need = static_cast<size_t>(nrows) * als_slot_floats(vdim_);
        if (slots_.size() < need) slots_.resize(need);
        BFH_HIP(hipMemsetAsync(slots_.get(), 0, need * sizeof(float), stream));
    }
    // solves every row of [start_x, next_x) that has entries in ip_a (or ip_b) from its slot
    void solve_rows(const AlsParams& p0, int start_x, int next_x, const int64_t* ip_a, const int64_t* ip_b) {
        std::vector<AlsHeavy> sv;
        for (int x = start_x; x < next_x; ++x) {
            const int64_t na = ip_a[x] - (x == 0 ? 0 : ip_a[x - 1]);
            const int64_t nb = ip_b ? ip_b[x] - (x == 0 ? 0 : ip_b[x - 1]) : 0;
            if (na + nb > 0) sv.push_back({x, x - start_x, na + nb});
        }
        if (sv.empty()) return;
        solve_list_.resize(std::max(solve_list_.size(), sv.size()));
        BFH_HIP(hipMemcpyAsync(solve_list_.get(), sv.data(), sv.size() * sizeof(AlsHeavy), hipMemcpyHostToDevice, stream));
        BFH_HIP(hipStreamSynchronize(stream));   // sv is a local
        launch_solve(p0, solve_list_.get(), static_cast<int>(sv.size()), slots_.get(), true);
    }
    double read_loss() {
        double v = 0.0;
        BFH_HIP(hipMemcpyAsync(&v, loss_.get(), sizeof(double), hipMemcpyDeviceToHost, stream));
        BFH_HIP(hipStreamSynchronize(stream));
        drain_aux();   // the stream is idle: book the Gramian queued by precompute (its events go back to the pool)
        return v;
    }
    static unsigned wave_blocks(int nrows) { return static_cast<unsigned>((nrows + 3) / 4); }

    // ---- fold-in ----
    // Everything bfh_cfr_fold_in refuses, before anything is uploaded or launched.  The key check is a host scan of all keys of both parts.
    // A part is absent when all four of its arguments are NULL / 0: every row is then empty in it.
    void fold_check(const std::string& t, int n_rows, const Emb* Ya, const int64_t* ip_a, const int32_t* keys_a, const float* vals_a, int64_t nnz_a,
                    const Emb* Gc, const Emb* Bc, const int64_t* ip_c, const int32_t* keys_c, const float* vals_c, int64_t nnz_c, int iters,
                    const float* init_bias, const float* out_bias) const {
        BFH_REQUIRE((!Ya || Ya->host) && (!Gc || (Gc->host && Bc->host)),
                    "fold_in(" + t + ") before set_embedding of the arrays it reads (user: item; item: user, context, context_bias; context: item, item_bias)");
        BFH_REQUIRE(!Gc || Gc->rows == Bc->rows, "fold_in(" + t + "): the factor of part c and its bias differ in rows");
        BFH_REQUIRE(n_rows >= 0, "fold_in: n_rows is negative");
        BFH_REQUIRE(iters >= 1, "fold_in: iters must be at least 1");
        BFH_REQUIRE(Gc || (!init_bias && !out_bias), "fold_in(user): a user has no bias (init_bias and out_bias must be NULL)");
        auto part = [&](const char* name, const Emb* F, const int64_t* ip, const int32_t* keys, const float* vals, int64_t nnz) {
            const std::string w = std::string("fold_in(") + t + "): part " + name;
            const bool absent = !ip && !keys && !vals && nnz == 0;
            BFH_REQUIRE(F || absent, w + " given, but this obj_type has none");
            if (absent) {
                BFH_REQUIRE(!F || n_rows == 0 || (Ya && Gc), w + " is missing");   // only an item may come with one part alone
                return;
            }
            BFH_REQUIRE(nnz >= 0, w + ": nnz is negative");
            BFH_REQUIRE(nnz < (int64_t(1) << 31) - 64, w + ": 2^31 entries or more in one call");
            BFH_REQUIRE(n_rows == 0 || ip, w + ": null indptr");
            BFH_REQUIRE(nnz == 0 || (keys && vals), w + ": null keys / vals with nnz > 0");
            int64_t prev = 0;
            for (int b = 0; b < n_rows; ++b) {
                BFH_REQUIRE(ip[b] >= prev, w + ": indptr decreases at row " + std::to_string(b));
                prev = ip[b];
            }
            BFH_REQUIRE(prev == nnz, w + ": indptr[n_rows - 1] != nnz");
            for (int64_t i = 0; i < nnz; ++i)
                if (keys[i] < 0 || keys[i] >= F->rows)
                    throw Error(BFH_ERR_INVALID, w + ": key " + std::to_string(keys[i]) + " at position " + std::to_string(i) + " is outside [0, " +
                                                     std::to_string(F->rows) + ")");
        };
        part("a", Ya, ip_a, keys_a, vals_a, nnz_a);
        part("c", Gc, ip_c, keys_c, vals_c, nnz_c);
    }
    // The fold-in Gramian of the factor part a gathers (kind 0: I^T I, kind 1: U^T U), recomputed only when that factor has changed; booked under aux_ms
    void fold_gramian(int kind, const Emb& Y) {
        FoldState& f = fold_;
        const size_t nff = static_cast<size_t>(vdim_) * vdim_;
        if (f.ff[kind].size() == nff && f.ff_ver[kind] == Y.ver) return;
        f.ff[kind].resize(nff);
        f.ff64.resize(nff);
        gramian_into(Y.dev.get(), Y.rows, f.ff64, f.ff[kind]);
        f.ff_ver[kind] = Y.ver;
    }
    void fold_upload(DevBuf<int32_t>& dk, DevBuf<float>& dv, const int32_t* keys, const float* vals, int64_t nnz) {
        grow(dk, static_cast<size_t>(std::max<int64_t>(nnz, 1)));
        grow(dv, static_cast<size_t>(std::max<int64_t>(nnz, 1)));
        if (!nnz) return;
        BFH_HIP(hipMemcpyAsync(dk.get(), keys, nnz * sizeof(int32_t), hipMemcpyHostToDevice, stream));
        BFH_HIP(hipMemcpyAsync(dv.get(), vals, nnz * sizeof(float), hipMemcpyHostToDevice, stream));
        stats.h2d_bytes += 8.0 * nnz;
    }
    // The rows with entries in either part (NULL: that part is empty throughout), longest first by n_a + n_c; a row's item does not depend on
    // the batch.  -> the length of the list, now in FoldState::list
    int fold_list(int n_rows, const int64_t* ip_a, const int64_t* ip_c) {
        FoldState& f = fold_;
        std::vector<CfrFoldItem> items;
        for (int x = 0; x < n_rows; ++x) {
            const int64_t ab = ip_a ? row_begin(ip_a, x) : 0, ae = ip_a ? ip_a[x] : 0;
            const int64_t cb = ip_c ? row_begin(ip_c, x) : 0, ce = ip_c ? ip_c[x] : 0;
            if (ae - ab + ce - cb > 0)   // (an empty row: the zero row, its init_bias kept)
                items.push_back({x, static_cast<int>(ab), static_cast<int>(ae), static_cast<int>(cb), static_cast<int>(ce)});
        }
        std::stable_sort(items.begin(), items.end(), [](const CfrFoldItem& a, const CfrFoldItem& b) {
            return (a.aend - a.abeg) + (a.cend - a.cbeg) > (b.aend - b.abeg) + (b.cend - b.cbeg);
        });
        grow(f.list, std::max<size_t>(1, items.size()));
        if (!items.empty()) BFH_HIP(hipMemcpyAsync(f.list.get(), items.data(), items.size() * sizeof(CfrFoldItem), hipMemcpyHostToDevice, stream));
        BFH_HIP(hipStreamSynchronize(stream));   // the vector ends with this function
        stats.h2d_bytes += static_cast<double>(items.size() * sizeof(CfrFoldItem));
        return static_cast<int>(items.size());
    }
    // fold_in's own state: nothing here is read or written by a training call, nothing of the training state is written by fold_in
    struct FoldState {
        int rows = 0, bias_rows = 0;           // rows of the last call ("fold") and how many of them have a bias ("fold_bias")
        DevBuf<float> ff[2];                   // the fold-in Gramians: [0] I^T I (user), [1] U^T U (item)
        uint64_t ff_ver[2] = {0, 0};
        DevBuf<double> ff64;
        DevBuf<float> out, bias;               // [rows, vdim], [rows]
        DevBuf<int32_t> keys_a, keys_c;
        DevBuf<float> vals_a, vals_c;
        DevBuf<CfrFoldItem> list;
    };
    FoldState fold_;

    float l_ = 1.f, reg_c_ = 0.f;
    bool cfr_loss_ = false;
    Emb U_, I_, C_, Ib_, Cb_;
    Csr cu_, ciu_, cic_, cc_;
    DevBuf<AlsHeavy> solve_list_;
    DevBuf<float> slots_;   // one slot per row of the call: both Gramian passes of the item update add into it
};

}  // namespace bfh
