// What the ALS, CFR and eALS handles share (gfx950): the options every one of them reads, the stream, the Gramian, the loss words and the
// ticket, the two timers, and the slot path of als_kernels.hpp that ALS and CFR both run -- work list -> als_gram_kernel into one HBM slot
// per row -> als_solve_kernel.  AlsHandle (als_handle.hpp), CfrHandle (cfr_impl.hpp) and EalsHandle (eals_handle.hpp) derive from it and
// own everything else themselves; none of them sees another's state.
#pragma once
#include <algorithm>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <tuple>
#include <type_traits>
#include <utility>
#include <vector>

#include "als_kernels.hpp"

namespace bfh {

// A run-time value in a closed range -> a template argument: f is called with std::integral_constant<int, Lo .. Hi> (values
// outside the range take the nearest end) or with std::true_type / std::false_type.  Every kernel instantiation of the
// library's ALS paths is named inside such a lambda; a combination that must not exist is excluded there with if constexpr.
template <int Lo, int Hi, class F>
void dispatch_int(int v, F&& f) {
    if constexpr (Lo == Hi) f(std::integral_constant<int, Lo>{});
    else if (v <= Lo) f(std::integral_constant<int, Lo>{});
    else dispatch_int<Lo + 1, Hi>(v, f);
}
template <class F>
void dispatch_bool(bool b, F&& f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}

class AlsCore : public HandleBase {
 public:
    ~AlsCore() override {
        if (stream) (void)hipStreamDestroy(stream);
    }
    // bfh_*_get_stats: everything queued so far is part of the numbers
    void refresh_stats() override {
        if (stream) BFH_HIP(hipStreamSynchronize(stream));
        drain_aux();
    }

 protected:
    // What the three init functions share: the option file, device, stream, CU count, d / vdim (refused above max_vdim), alpha and the two
    // regularisers, the Gramian buffers, `loss_words` doubles of loss and the ticket, all zeroed.
    // False with last_error set on a bad option file.  The caller reads its own options and sets inited_ last.
    bool init_common(const char* opt_path, int max_vdim, size_t loss_words) {
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
        BFH_REQUIRE(vdim_ <= max_vdim, "d > " + std::to_string(max_vdim) + " is not supported by the gfx950 kernels yet");
        alpha_ = static_cast<float>(opt_.num("alpha"));
        reg_u_ = static_cast<float>(opt_.num("reg_u"));
        reg_i_ = static_cast<float>(opt_.num("reg_i"));
        FF_.resize(static_cast<size_t>(vdim_) * vdim_, true, stream);
        FF64_.resize(static_cast<size_t>(vdim_) * vdim_, true, stream);
        loss_.resize(loss_words, true, stream);
        ticket_.resize(1, true, stream);
        BFH_HIP(hipStreamSynchronize(stream));
        return true;
    }

    // FF = F^T F for a device matrix [rows, vdim]
    void gramian_of(const float* F, int rows) { gramian_into(F, rows, FF64_, FF_); }
    // ... into a pair of buffers [vdim, vdim]: the fp64 accumulator of the slices and its float rounding
    void gramian_into(const float* F, int rows, DevBuf<double>& acc, DevBuf<float>& ff) {
        BFH_HIP(hipMemsetAsync(acc.get(), 0, acc.bytes(), stream));
        const int T = vdim_ / 32;
        constexpr int NT = 4;
        const int TG = (T + NT - 1) / NT;
        // Waves per CU: 4 at vdim 128 (configs[2]: 0.157 instead of 0.229 ms per epoch, every d = 128 parity case unchanged), 8 elsewhere.
        // Measured on ML-20M at d = 128 (profiles/r06_als_gramian.txt, ms for the items / the users): 4 waves per CU 0.048 / 0.109, 8: 0.086 / 0.143,
        // 12: 0.118 / 0.163 -- every slice ends in 64 fp64 atomics per lane on the same 16 K addresses, so fewer, longer slices are faster.  Outside vdim 128 it STAYS at 8:
        // the slice boundaries decide FF's last bits, and with 4 the one matrix-free tiny case at d = 160 / block_size 64 -- three CG steps on systems conditioned
        // beyond fp32 -- lands at 20x the oracle's distance from float64 instead of 0.2x (deterministically; every other case unchanged: GPU call 14).  A re-roll of
        // the rounding, not an error of either FF (both 7e-8 from float64) -- but the parity suite is held as it is.
        const int wpc = vdim_ == 128 ? 4 : 8;
        int slices = (num_cus_ * wpc) / (T * TG);
        if (slices < 1) slices = 1;
        int rps = (rows + slices - 1) / slices;
        rps = (rps + 1) & ~1;  // even: row pairs never straddle slices
        if (rps < 2) rps = 2;
        slices = (rows + rps - 1) / rps;
        const int slot = t_aux_.begin(stream);
        hipLaunchKernelGGL(als_gramian_kernel<NT>, dim3(slices, T, TG), dim3(64), 0, stream, F, rows, vdim_, rps, acc.get());
        BFH_HIP(hipGetLastError());
        const int nff = vdim_ * vdim_;
        hipLaunchKernelGGL(als_gramian_round_kernel, dim3((nff + 255) / 256), dim3(256), 0, stream, acc.get(), ff.get(), nff);
        BFH_HIP(hipGetLastError());
        t_aux_.end(slot, stream);
        // (no synchronisation here since round 6: nothing of the Gramian is read by the host, the next call on the stream waits for it anyway, and a
        //  blocking call per precompute was ~30 us of the epoch; the timer is drained where the stream is idle next -- a row update, get_stats)
    }
    // stream idle: account what the aux timer holds
    void drain_aux() { stats.aux_ms += t_aux_.drain(); }

    // ---- the slot path: work list -> als_gram_kernel on the fp32 instruction, tiles to HBM slots -> als_solve_kernel -----------------
    static bool big_gather(const AlsParams& p) { return static_cast<uint64_t>(p.op_rows) * p.vdim * 4 >= (1ull << 32); }

    // slot (row - start_x) below slot_base = the call's rows, slot_base + wk.slot for the chunks of a heavy (or deferred) row;
    // slot_base 0: only the latter exist
    void launch_gram_to_slots(const AlsParams& p, const AlsWork* work, int n, float* scratch, int slot_base, bool ials) {
        const int blocks = std::min((n + 3) / 4, num_cus_ * 4);   // 4 independent waves per block, one work item each; persistent: residency is set by the kernel's VGPR count
        dispatch_int<1, 4>(vdim_ / 32, [&](auto tt) { dispatch_bool(ials, [&](auto il) { dispatch_bool(big_gather(p), [&](auto bg) {
            constexpr int TT = decltype(tt)::value;
            constexpr bool IALS = decltype(il)::value, BG = decltype(bg)::value;
            hipLaunchKernelGGL((als_gram_kernel<TT, IALS, false, BG>), dim3(blocks), dim3(256), 0, stream, p, work, n, scratch, slot_base);
        }); }); });
        BFH_HIP(hipGetLastError());
    }
    // als_solve_kernel over the n slots of a list: a block per slot, or (persistent) as many blocks as the CUs' LDS holds, walking the list
    void launch_solve(const AlsParams& p, const AlsHeavy* list, int n, const float* scratch, bool persistent) { launch_solve(p, list, n, scratch, persistent, code_); }
    // ... with the solver named by the caller (fold_in: 0, whatever the option file says)
    void launch_solve(const AlsParams& p, const AlsHeavy* list, int n, const float* scratch, bool persistent, int mode) {
        const size_t lds = als_gs_lds_bytes(vdim_);
        BFH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(als_solve_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
        const int blocks = persistent ? std::min(n, persistent_solve_blocks(lds)) : n;
        hipLaunchKernelGGL(als_solve_kernel, dim3(blocks), dim3(256), lds, stream, p, list, n, scratch, mode);
        BFH_HIP(hipGetLastError());
    }
    // as many blocks as the CUs' LDS holds (at most 8 per CU)
    int persistent_solve_blocks(size_t lds) const { return num_cus_ * static_cast<int>(std::max<size_t>(1, std::min<size_t>(8, (160 * 1024) / lds))); }

    struct WorkList {
        DevBuf<AlsWork> work;
        DevBuf<AlsHeavy> heavy;   // fused kernels: heavy rows only (slot = scratch slot)
        DevBuf<AlsHeavy> solve;   // split design: every non-empty row, longest first (slot = row - start_x)
        DevBuf<AlsWork> heavy_work;   // wide kernel's finalize launch: one item per heavy row (kend - kbeg = its nnz)
        int n_work = 0, n_heavy = 0, n_solve = 0;
        // als_pc_kernel: items whose weights need the fp32 instruction (AlsHandle::scan_deferred)
        DevBuf<int> defer;             // per work item
        DevBuf<AlsWork> dlist;         // the flagged items (whole rows with their scratch slot = n_heavy + j)
        DevBuf<AlsHeavy> dsolve;       // the flagged whole rows, for als_solve_kernel
        DevBuf<int> dcount;
        int n_def = 0, n_def_rows = 0;
        uint64_t scan_ver = ~uint64_t(0);
        float scan_wcut = -1.f;
        const float* scan_vals = nullptr;
        std::vector<int64_t> bounds;   // check_bounds: the host copy of ip[start_x - 1 .. next_x) the list was built from
    };
    // The work items of one row of n > 0 entries at chunk-local position kb: the whole row (slot -1: its result is complete), or, above HEAVY
    // entries, chunks of equal, even length that are summed into the zeroed scratch slot `heavy_slot`.  The one statement of the rule, for
    // work_list and AlsHandle::fold_plan.
    static constexpr int64_t HEAVY = 4096;
    static void push_row_items(std::vector<AlsWork>& w, int row, int64_t kb, int64_t n, int heavy_slot) {
        if (n <= HEAVY) {
            w.push_back({row, static_cast<int>(kb), static_cast<int>(kb + n), -1});
            return;
        }
        const int64_t nch = (n + HEAVY - 1) / HEAVY, per = ((n + nch - 1) / nch + 1) & ~int64_t(1);
        for (int64_t c0 = 0; c0 < n; c0 += per)
            w.push_back({row, static_cast<int>(kb + c0), static_cast<int>(kb + std::min(n, c0 + per)), heavy_slot});
    }
    // Whose rows a cached work list cuts: the two sides of ALS, the four matrices of CFR
    enum class WorkId { AlsUsers, AlsItems, CfrUser, CfrItemUsers, CfrItemContexts, CfrContext };
    // Work items of one row-update call: one per non-empty row, rows above HEAVY nnz cut into
    // chunks; longest first (dynamic ticket order) so the tail is short.  Cached per (matrix, range): ALS replaces its matrix only
    // through set_placeholder / set_resident_csr, which clear the cache.  `check_bounds`: the caller may hand another matrix to
    // any call (CFR: cfr.py:68 set_data on a model in use; CCFR keeps no data state), so a hit also needs the row bounds
    // ip[start_x - 1 .. next_x) the list was built from -- 8 bytes per row beside an indptr upload of the same size.
    WorkList& work_list(WorkId id, int start_x, int next_x, const int64_t* ip, int64_t shift, bool check_bounds = false) {
        const auto key = std::make_tuple(id, start_x, next_x);
        const int64_t* bfirst = ip + (start_x == 0 ? 0 : start_x - 1);
        const int64_t* blast = ip + next_x;
        auto it = work_cache_.find(key);
        if (it != work_cache_.end() && (!check_bounds || (it->second->bounds.size() == static_cast<size_t>(blast - bfirst) &&
                                                          std::equal(bfirst, blast, it->second->bounds.begin()))))
            return *it->second;
        std::vector<AlsWork> w;
        std::vector<AlsHeavy> h, sv;
        w.reserve(next_x - start_x);
        sv.reserve(next_x - start_x);
        int64_t prev = start_x == 0 ? 0 : ip[start_x - 1];
        for (int x = start_x; x < next_x; ++x) {
            const int64_t e = ip[x], n = e - prev;
            if (n > 0) {  // Q-16: empty rows are left untouched
                const int64_t kb = prev - shift;
                if (n <= HEAVY) {
                    push_row_items(w, x, kb, n, -1);
                    sv.push_back({x, x - start_x, n});
                } else {
                    const int slot = static_cast<int>(h.size());
                    sv.push_back({x, (next_x - start_x) + slot, n});   // split design: heavy slots follow the per-row slots
                    h.push_back({x, slot, n});
                    push_row_items(w, x, kb, n, slot);
                }
            }
            prev = e;
        }
        std::stable_sort(w.begin(), w.end(), [](const AlsWork& a, const AlsWork& b) { return (a.kend - a.kbeg) > (b.kend - b.kbeg); });
        std::stable_sort(sv.begin(), sv.end(), [](const AlsHeavy& a, const AlsHeavy& b) { return a.n > b.n; });
        auto wl = std::make_unique<WorkList>();
        if (check_bounds) wl->bounds.assign(bfirst, blast);
        wl->n_work = static_cast<int>(w.size());
        wl->n_heavy = static_cast<int>(h.size());
        wl->n_solve = static_cast<int>(sv.size());
        wl->solve.resize(std::max<size_t>(1, sv.size()));
        if (!sv.empty()) BFH_HIP(hipMemcpyAsync(wl->solve.get(), sv.data(), sv.size() * sizeof(AlsHeavy), hipMemcpyHostToDevice, stream));
        wl->work.resize(std::max<size_t>(1, w.size()));
        wl->heavy.resize(std::max<size_t>(1, h.size()));
        {
            std::vector<AlsWork> hw;
            for (const auto& hh : h) hw.push_back({hh.row, 0, static_cast<int>(hh.n), hh.slot});
            wl->heavy_work.resize(std::max<size_t>(1, hw.size()));
            if (!hw.empty()) BFH_HIP(hipMemcpyAsync(wl->heavy_work.get(), hw.data(), hw.size() * sizeof(AlsWork), hipMemcpyHostToDevice, stream));
        }
        if (!w.empty()) BFH_HIP(hipMemcpyAsync(wl->work.get(), w.data(), w.size() * sizeof(AlsWork), hipMemcpyHostToDevice, stream));
        if (!h.empty()) BFH_HIP(hipMemcpyAsync(wl->heavy.get(), h.data(), h.size() * sizeof(AlsHeavy), hipMemcpyHostToDevice, stream));
        BFH_HIP(hipStreamSynchronize(stream));
        if (work_cache_.size() > 64) work_cache_.clear();
        return *(work_cache_[key] = std::move(wl));
    }

    Options opt_;
    bool inited_ = false;
    int d_ = 0, vdim_ = 0, code_ = 2, num_cg_max_iters_ = 3, num_cus_ = 256;
    float alpha_ = 0, reg_u_ = 0, reg_i_ = 0, eps_ = 1e-10f, cg_tol_ = 1e-10f;
    DevBuf<float> FF_;
    DevBuf<double> FF64_;   // fp64 accumulator of the Gramian slices (see als_gramian_kernel)
    DevBuf<double> loss_;
    DevBuf<int> ticket_;
    std::map<std::tuple<WorkId, int, int>, std::unique_ptr<WorkList>> work_cache_;
    EventTimer t_main_, t_aux_;
};

}  // namespace bfh
