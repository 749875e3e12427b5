// eALS handle (gfx950): the host side of the kernels in eals_kernels.hpp.  precompute_cache binds one orientation (structure, row
// classes, the index map into the other orientation by a device radix sort, vhat); update launches the three row classes side by side.
// EalsHandle derives from AlsCore (als_core.hpp) for the options, the stream, the Gramian and the timers; the factors are its own.
#pragma once
#include <algorithm>

#include "als_core.hpp"
#include "eals_kernels.hpp"

namespace bfh {

class EalsHandle : public AlsCore {
 public:   // the entry points of als.hip
    ~EalsHandle() override {
        for (int k = 0; k < 2; ++k) {
            if (side_done_[k]) (void)hipEventDestroy(side_done_[k]);
            if (side_stream_[k]) (void)hipStreamDestroy(side_stream_[k]);
        }
        if (side_go_) (void)hipEventDestroy(side_go_);
    }
    bool init(const char* opt_path) {   // eals.cc:19-31
        if (!init_common(opt_path, 1024, 4)) return false;
        S2_.resize(static_cast<size_t>(vdim_) * vdim_, true, stream);   // (stream order is enough: estimate_loss fills it on the same stream)
        inited_ = true;
        return true;
    }
    // eals.cc:33-47
    void initialize_model(float* P, float* Q, float* Cw, int P_rows, int Q_rows) {
        BFH_REQUIRE(inited_, "initialize_model called before init");
        BFH_REQUIRE(P && Q && Cw && P_rows > 0 && Q_rows > 0, "initialize_model: null arrays or empty shapes");
        hostP_ = P; hostQ_ = Q; P_rows_ = P_rows; Q_rows_ = Q_rows;
        P_.resize(static_cast<size_t>(P_rows) * vdim_, true, stream);
        Q_.resize(static_cast<size_t>(Q_rows) * vdim_, true, stream);
        Cw_.resize(Q_rows);
        stats.h2d_bytes += rows_to_device(P_.get(), vdim_, P, d_, 0, P_rows, stream);
        stats.h2d_bytes += rows_to_device(Q_.get(), vdim_, Q, d_, 0, Q_rows, stream);
        BFH_HIP(hipMemcpyAsync(Cw_.get(), Cw, sizeof(float) * Q_rows, hipMemcpyHostToDevice, stream));
        BFH_HIP(hipStreamSynchronize(stream));
        cached_[0] = cached_[1] = false;
        model_ = true;
    }

    // eals.cc:49-100: the orientation's structure stays resident; the index map by a device sort; vhat from the current factors
    void precompute_cache(int nnz, const int64_t* indptr, const int32_t* keys, int axis) {
        BFH_REQUIRE(model_, "precompute_cache before initialize_model");
        BFH_REQUIRE(axis == 0 || axis == 1, "axis must be 0 or 1");
        if (cached_[axis]) return;   // eals.cc:54-56
        const int rows = rows_of(axis);
        BFH_REQUIRE(indptr && keys && nnz >= 0 && (rows == 0 || indptr[rows - 1] == nnz), "precompute_cache: indptr does not end at nnz");
        Side& s = side_[axis];
        bind_structure(s, rows, nnz, indptr, keys);
        classify_rows(s, rows, indptr);
        const int slot = t_aux_.begin(stream);
        if (nnz) build_index_map(s, rows, rows_of(1 - axis));
        fill_cache(s, axis, rows);
        t_aux_.end(slot, stream);
        BFH_HIP(hipStreamSynchronize(stream));
        stats.h2d_bytes += 8.0 * rows + 4.0 * nnz;
        stats.aux_ms += t_aux_.drain();
        cached_[axis] = true;
    }

    // eals.cc:102-115: false until both caches exist
    bool update(const int64_t* indptr, const int32_t* keys, const float* vals, int axis) {
        BFH_REQUIRE(model_, "update before initialize_model");
        BFH_REQUIRE(axis == 0 || axis == 1, "axis must be 0 or 1");
        if (!(cached_[0] && cached_[1])) return false;
        (void)indptr; (void)keys;   // the structure was bound by precompute_cache
        Side& s = side_[axis];
        upload_vals(s, vals);
        stats.h2d_bytes += 4.0 * s.nnz;
        gram_for(axis);
        const EalsParams p = make_eals_params(axis);
        // three launches over disjoint rows (heavy / mid / light), each with its own ticket, side by side on three streams: the few
        // blocks of the longest rows would otherwise leave most of the chip idle while they crawl through their 128 steps
        ensure_side_streams();
        const int g_heavy = std::min(s.n_heavy, num_cus_ * 2), g_mid = std::min(s.n_mid, num_cus_ * 16), g_light = std::min((s.n_light + 3) / 4, num_cus_ * 4);
        // mid slot = the longest mid row (the list is sorted longest first) rounded up to a wave, not the class bound EALS_HEAVY: mid rows
        // may be as short as EALS_LIGHT + 1 entries, and 4,096 groups x 17 x EALS_HEAVY floats were 1.1 GB whatever the rows' lengths
        const int64_t cap = std::min<int64_t>(EALS_HEAVY, round64(s.mid_longest));
        const RowClass classes[3] = {
            {Rows::Heavy, s.heavy.get(), s.n_heavy, 0, -1, g_heavy, &scratch_h_, static_cast<size_t>(s.heavy_entries) * (1 + EALS_DB), 0},
            {Rows::Mid, s.mid.get(), s.n_mid, 1, 0, g_mid, &scratch_m_, static_cast<size_t>(g_mid) * (1 + EALS_DB) * cap, cap},
            {Rows::Light, s.light.get(), s.n_light, 2, 1, g_light, nullptr, 0, 0},
        };
        BFH_HIP(hipMemsetAsync(tickets3_.get(), 0, 3 * sizeof(int), stream));
        const int slot = t_main_.begin(stream);
        BFH_HIP(hipEventRecord(side_go_, stream));
        for (const RowClass& c : classes) launch_class(p, s, c);
        t_main_.end(slot, stream);
        stats.d2h_bytes += rows_to_host(axis == 0 ? hostP_ : hostQ_, d_, axis == 0 ? P_.get() : Q_.get(), vdim_, 0, rows_of(axis), stream);   // the updated side -> the caller's array
        BFH_HIP(hipStreamSynchronize(stream));
        drain_aux();   // the stream is idle: book gram_for's Gramian (its events go back to the pool)
        stats.kernel_ms += t_main_.drain();
        stats.samples += s.nnz;
        stats.launches += 1;
        return true;
    }

    // eals.cc:117-174 -> (rmse, loss); accumulated in double (the reference sums tens of millions of floats in a float)
    void estimate_loss(int nnz, const int64_t* indptr, const int32_t* keys, const float* vals, int axis, float* rmse, float* loss) {
        (void)indptr; (void)keys;
        *rmse = *loss = 0.f;
        if (!(cached_[0] && cached_[1])) return;
        Side& s = side_[axis];
        BFH_REQUIRE(nnz == s.nnz, "estimate_loss: nnz differs from the cached structure");
        upload_vals(s, vals);
        launch_loss_terms(s, axis);
        double acc[4];
        const double ip = gram_inner_product(acc);
        const double reg = static_cast<double>(reg_u_) * acc[2] + static_cast<double>(reg_i_) * acc[3];
        *rmse = static_cast<float>(std::sqrt(acc[1] / std::max(nnz, 1)));
        *loss = static_cast<float>(acc[0] + ip + reg);
    }

 private:
    int rows_of(int axis) const { return axis == 0 ? P_rows_ : Q_rows_; }
    static int64_t round64(int64_t n) { return ((n + 63) / 64) * 64; }

    struct Side {
        DevBuf<int64_t> indptr, map;
        DevBuf<int32_t> keys;
        DevBuf<float> vals, vhat;
        DevBuf<int32_t> light, mid, heavy;   // row ids with <= EALS_LIGHT / <= EALS_HEAVY / more entries, the long ones longest first (empty rows are light: the regulariser still moves them)
        int n_light = 0, n_mid = 0, n_heavy = 0;
        int64_t mid_longest = 0;
        int64_t heavy_entries = 0;                // sum of the heavy rows' lengths, each rounded up to 64
        DevBuf<int64_t> heavy_off;                // [n_heavy] scratch offset (entries) of every heavy row, in list order
        int64_t nnz = 0;
    };

    void bind_structure(Side& s, int rows, int nnz, const int64_t* indptr, const int32_t* keys) {
        s.nnz = nnz;
        s.indptr.resize(rows);
        s.keys.resize(std::max(nnz, 1));
        s.vals.resize(std::max(nnz, 1));
        s.vhat.resize(std::max(nnz, 1));
        s.map.resize(std::max(nnz, 1));
        BFH_HIP(hipMemcpyAsync(s.indptr.get(), indptr, sizeof(int64_t) * rows, hipMemcpyHostToDevice, stream));
        if (nnz) BFH_HIP(hipMemcpyAsync(s.keys.get(), keys, sizeof(int32_t) * nnz, hipMemcpyHostToDevice, stream));
    }
    // one host pass: every row into its class, the long classes longest first (ticket order), every heavy row's scratch offset
    void classify_rows(Side& s, int rows, const int64_t* indptr) {
        auto len = [&](int x) { return indptr[x] - row_begin(indptr, x); };
        std::vector<int32_t> li, md, hv;
        for (int x = 0; x < rows; ++x) (len(x) > EALS_HEAVY ? hv : (len(x) > EALS_LIGHT ? md : li)).push_back(x);
        auto longer = [&](int a, int b) { return len(a) > len(b); };
        std::stable_sort(hv.begin(), hv.end(), longer);
        std::stable_sort(md.begin(), md.end(), longer);
        std::vector<int64_t> off(hv.size());
        s.heavy_entries = 0;
        for (size_t k = 0; k < hv.size(); ++k) { off[k] = s.heavy_entries; s.heavy_entries += round64(len(hv[k])); }
        s.mid_longest = md.empty() ? 0 : len(md[0]);
        auto upload = [&](auto& dev, const auto& host) {   // -> the list's length
            dev.resize(std::max<size_t>(1, host.size()));
            if (!host.empty()) BFH_HIP(hipMemcpyAsync(dev.get(), host.data(), host.size() * sizeof(host[0]), hipMemcpyHostToDevice, stream));
            return static_cast<int>(host.size());
        };
        s.n_light = upload(s.light, li);
        s.n_mid = upload(s.mid, md);
        s.n_heavy = upload(s.heavy, hv);
        upload(s.heavy_off, off);
        BFH_HIP(hipStreamSynchronize(stream));   // the lists are locals
    }
    // rank of every entry in (other id, own id) order = its position in the other orientation (eals.cc:81-99): one
    // radix sort of (other id << 32 | own id) with the entry's position as payload, then map[payload[r]] = r
    void build_index_map(Side& s, int rows, int other_rows) {
        const int64_t nnz = s.nnz;
        DevBuf<uint64_t> ka, kb;   // 32 bytes per entry in all: they live for this step only
        DevBuf<int64_t> va, vb;
        DevBuf<char> tmp;
        ka.resize(nnz); kb.resize(nnz); va.resize(nnz); vb.resize(nnz);
        const unsigned blocks = static_cast<unsigned>((nnz + 255) / 256);
        hipLaunchKernelGGL(eals_coord_kernel, dim3(blocks), dim3(256), 0, stream, s.indptr.get(), s.keys.get(), rows, nnz, ka.get(), va.get());
        BFH_HIP(hipGetLastError());
        int bits = 33;
        while (bits < 64 && (uint64_t(1) << (bits - 32)) < static_cast<uint64_t>(other_rows)) ++bits;
        device_sort_pairs_u64(ka.get(), kb.get(), va.get(), vb.get(), nnz, bits, tmp, stream);
        hipLaunchKernelGGL(eals_rank_kernel, dim3(blocks), dim3(256), 0, stream, vb.get(), nnz, s.map.get());
        BFH_HIP(hipGetLastError());
        BFH_HIP(hipStreamSynchronize(stream));   // the sort buffers are locals
    }
    void fill_cache(Side& s, int axis, int rows) {
        hipLaunchKernelGGL(eals_cache_kernel, dim3(static_cast<unsigned>((rows + 3) / 4)), dim3(256), 0, stream, axis == 0 ? P_.get() : Q_.get(),
                           axis == 0 ? Q_.get() : P_.get(), vdim_, rows, s.indptr.get(), s.keys.get(), s.vhat.get());
        BFH_HIP(hipGetLastError());
    }

    // S for the update of `axis`: axis 0 -> sum_i C_i q q^T (eals.cc:179-191), axis 1 -> P^T P (:234-235); lands in FF_
    void gram_for(int axis) {
        if (axis == 0) {
            CQ_.resize(static_cast<size_t>(Q_rows_) * vdim_);
            const int64_t n = static_cast<int64_t>(Q_rows_) * vdim_;
            hipLaunchKernelGGL(eals_scale_rows_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, stream, Q_.get(), Cw_.get(), Q_rows_, vdim_,
                               CQ_.get());
            BFH_HIP(hipGetLastError());
            gramian_of(CQ_.get(), Q_rows_);
        } else {
            gramian_of(P_.get(), P_rows_);
        }
    }
    void upload_vals(Side& s, const float* vals) {   // the structure was bound by precompute_cache; the values come with every call
        if (s.nnz) BFH_HIP(hipMemcpyAsync(s.vals.get(), vals, sizeof(float) * s.nnz, hipMemcpyHostToDevice, stream));
    }

    // One launch of update(): a class of rows, where it runs and over how much scratch.
    enum class Rows { Heavy, Mid, Light };
    struct RowClass {
        Rows kind;
        const int32_t* list;       // the class's rows ...
        int n;                     // ... and how many
        int ticket;                // index into tickets3_
        int side;                  // -1: the main stream; 0 / 1: side_stream_[side], forked from side_go_ and joined back
        int groups;                // thread groups launched (blocks; the mid class: one-wave blocks)
        DevBuf<float>* scratch;    // grown to `floats` before the launch
        size_t floats;
        int64_t cap;               // mid: entries per scratch slot, one slot per group
    };
    void fork_side(int k) { BFH_HIP(hipStreamWaitEvent(side_stream_[k], side_go_, 0)); }
    void join_side(int k) {
        BFH_HIP(hipEventRecord(side_done_[k], side_stream_[k]));
        BFH_HIP(hipStreamWaitEvent(stream, side_done_[k], 0));
    }
    void launch_class(EalsParams p, const Side& s, const RowClass& c) {
        if (!c.n) return;
        p.row_list = c.list; p.n_list = c.n; p.ticket = tickets3_.get() + c.ticket;
        if (c.scratch && c.scratch->size() < c.floats) c.scratch->resize(c.floats);
        const hipStream_t st = c.side < 0 ? stream : side_stream_[c.side];
        if (c.side >= 0) fork_side(c.side);
        const size_t lds_long = (static_cast<size_t>(vdim_) + 48) * sizeof(float);   // x | red[3][16]
        switch (c.kind) {
            case Rows::Heavy:   // one 1024-thread block per row, every row over its own slot (heavy_off)
                hipLaunchKernelGGL(eals_update_long_kernel<1024>, dim3(c.groups), dim3(1024), lds_long, st, p, c.scratch->get(), int64_t(0),
                                   static_cast<const int64_t*>(s.heavy_off.get()));
                break;
            case Rows::Mid:     // one wave per row over its group's slot
                hipLaunchKernelGGL(eals_update_long_kernel<64>, dim3(c.groups), dim3(64), lds_long, st, p, c.scratch->get(), c.cap,
                                   static_cast<const int64_t*>(nullptr));
                break;
            case Rows::Light:   // four waves per block, a row each, in registers
                hipLaunchKernelGGL(eals_update_kernel, dim3(c.groups), dim3(256), static_cast<size_t>(4) * vdim_ * sizeof(float), st, p);
                break;
        }
        BFH_HIP(hipGetLastError());
        if (c.side >= 0) join_side(c.side);
    }
    void ensure_side_streams() {
        if (tickets3_.size() < 3) tickets3_.resize(3);
        if (side_stream_[0]) return;
        for (int k = 0; k < 2; ++k) {
            BFH_HIP(hipStreamCreateWithFlags(&side_stream_[k], hipStreamNonBlocking));
            BFH_HIP(hipEventCreateWithFlags(&side_done_[k], hipEventDisableTiming));
        }
        BFH_HIP(hipEventCreateWithFlags(&side_go_, hipEventDisableTiming));
    }
    EalsParams make_eals_params(int axis) {
        const Side& s = side_[axis];
        EalsParams p{};
        p.X = axis == 0 ? P_.get() : Q_.get();
        p.Y = axis == 0 ? Q_.get() : P_.get();
        p.Cw = Cw_.get(); p.S = FF_.get();
        p.indptr = s.indptr.get(); p.keys = s.keys.get(); p.vals = s.vals.get();
        p.own = s.vhat.get(); p.other = side_[1 - axis].vhat.get(); p.map = s.map.get();
        p.d = d_; p.vdim = vdim_; p.axis = axis; p.alpha = alpha_; p.reg = axis == 0 ? reg_u_ : reg_i_;
        return p;
    }
    // loss_[0] feedbacks, [1] squared error over the entries; [2] |P|^2, [3] |Q|^2
    void launch_loss_terms(const Side& s, int axis) {
        BFH_HIP(hipMemsetAsync(loss_.get(), 0, 4 * sizeof(double), stream));
        const int rows = rows_of(axis);
        hipLaunchKernelGGL(eals_loss_kernel, dim3(static_cast<unsigned>((rows + 3) / 4)), dim3(256), 0, stream, s.indptr.get(), s.keys.get(), s.vals.get(),
                           s.vhat.get(), Cw_.get(), rows, axis, alpha_, loss_.get());
        hipLaunchKernelGGL(eals_sqsum_kernel, dim3(num_cus_ * 4), dim3(256), 0, stream, P_.get(), static_cast<int64_t>(P_rows_) * vdim_, loss_.get() + 2);
        hipLaunchKernelGGL(eals_sqsum_kernel, dim3(num_cus_ * 4), dim3(256), 0, stream, Q_.get(), static_cast<int64_t>(Q_rows_) * vdim_, loss_.get() + 3);
        BFH_HIP(hipGetLastError());
    }
    // <S^p, S^q> over the full symmetric matrices (misc/blas.hpp:49-63 mirrors the computed triangle); loss_ -> acc[4] under the same synchronisation
    double gram_inner_product(double* acc) {
        const size_t nn = static_cast<size_t>(vdim_) * vdim_;
        gram_for(1);
        BFH_HIP(hipMemcpyAsync(S2_.get(), FF_.get(), nn * sizeof(float), hipMemcpyDeviceToDevice, stream));
        gram_for(0);
        std::vector<float> sp(nn), sq(nn);
        BFH_HIP(hipMemcpyAsync(sp.data(), S2_.get(), nn * sizeof(float), hipMemcpyDeviceToHost, stream));
        BFH_HIP(hipMemcpyAsync(sq.data(), FF_.get(), nn * sizeof(float), hipMemcpyDeviceToHost, stream));
        BFH_HIP(hipMemcpyAsync(acc, loss_.get(), 4 * sizeof(double), hipMemcpyDeviceToHost, stream));
        BFH_HIP(hipStreamSynchronize(stream));
        double ip = 0.0;
        for (size_t k = 0; k < nn; ++k) ip += static_cast<double>(sp[k]) * static_cast<double>(sq[k]);
        return ip;
    }

    bool model_ = false;
    float *hostP_ = nullptr, *hostQ_ = nullptr;   // the caller's arrays [rows, d]
    int P_rows_ = 0, Q_rows_ = 0;
    DevBuf<float> P_, Q_;                         // [rows, vdim], pad columns zero
    bool cached_[2] = {false, false};
    Side side_[2];
    DevBuf<float> Cw_, CQ_, S2_;
    DevBuf<float> scratch_m_, scratch_h_;   // per thread group (1 + EALS_DB) * cap floats (eals_update_long_kernel)
    DevBuf<int> tickets3_;
    hipStream_t side_stream_[2] = {nullptr, nullptr};
    hipEvent_t side_done_[2] = {nullptr, nullptr}, side_go_ = nullptr;
};

}  // namespace bfh
