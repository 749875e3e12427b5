// SPPMI matrix of a stream on the device (the context input of CoFactor / CFR) -- host steps + C ABI; the kernels are in sppmi_kernels.hpp.
//
// Reference semantics, three steps of buffalo's data creation:
//   * pair lines, /root/reference/buffalo/data/stream.py:257-267: for every user's sequence, each item and the `windows`
//     items after it are written as the two text lines "w c" and "c w"; sppmi_total_lines (D) counts the lines;
//   * _parallel_build_sppmi, /root/reference/buffalo/data/fileio.hpp:109-254, over the lines sorted by their first id:
//     appearances[id] = lines starting with id; for every distinct pair (probe, c), c <= probe, with cnt lines:
//     pmi = log(cnt) + log(D) - log(app[probe]) - log(app[c]) (double, left to right), sppmi = pmi - log(k); when
//     sppmi > 0 the lines "probe c sppmi" and "c probe sppmi" are written -- as text with six significant digits
//     (`fout << double`), which the next step parses with "%f" (fileio.hpp:84);
//   * the output is sorted by (row, col) and compressed into (indptr, key, val) like any matrix (stream.py:181-195).
//
// Device formulation -- no text, no files, one pass each:
//   1. pairs per user in closed form, exclusive scan -> where each user's lines start;
//   2. one thread per event writes its <= 2 * windows lines as keys  first * num_items + second  (32-bit while num_items^2 fits,
//      which halves the bytes of steps 2-3; 64-bit beyond 65,536 items);
//   3. radix sort of the keys over the bits they use (device_sort_keys), run-length encode (distinct pairs + cnt);
//   4. appearances by two binary searches per item in the sorted keys (no atomics on popular items);
//   5. one thread per distinct pair: the reference's double arithmetic, the six-digit decimal rounding of the text
//      round trip restated in exact double steps (powers of ten up to 1e22 are exact), emit count 0 / 1 / 2;
//   6. exclusive scan of the emit counts, scatter.  The distinct pairs are already in (row, col) order and the lines
//      are symmetric (cnt(a, b) == cnt(b, a)), so entry (a, b) is produced from its own run with probe = max(a, b) --
//      the output needs no second sort; indptr comes from the row changes.
// HBM-bound integer work: 8 (16) B per line and radix pass; the log / rounding step touches only the distinct pairs.
#include <cmath>
#include <cstring>

#include "abi.hpp"
#include "builder_base.hpp"
#include "sppmi_kernels.hpp"

namespace bfh {

// The scratch of ONE build, freed when build_with returns: a 200 M-line build must not leave ~2 GB parked in the handle.
template <typename KeyT>
struct SppmiWork {
    DevBuf<int64_t> indptr, pairs, off, app, emit, emit_off, n_runs;
    DevBuf<int32_t> items, rows;
    DevBuf<KeyT> keys, sorted, uniq;
    DevBuf<unsigned int> cnt;
    DevBuf<float> val;
    DevBuf<char> tmp;
};

class SppmiHandle : public BuilderHandle {
 public:
    SppmiHandle() : BuilderHandle("sppmi") {}

    void build(const int64_t* indptr, const int32_t* items, int num_users, int num_items, int windows, int k, int64_t* nnz_out, int64_t* lines_out) {
        if (static_cast<uint64_t>(num_items) * static_cast<uint64_t>(num_items) <= (uint64_t(1) << 32))
            build_with<uint32_t>(indptr, items, num_users, num_items, windows, k, nnz_out, lines_out);
        else
            build_with<uint64_t>(indptr, items, num_users, num_items, windows, k, nnz_out, lines_out);
    }

    void fetch(int64_t* indptr_out, int32_t* keys_out, float* vals_out) {
        BFH_REQUIRE(num_items_ > 0, "sppmi: fetch before build");
        ensure();
        BFH_HIP(hipMemcpyAsync(indptr_out, d_indptr_out_.get(), sizeof(int64_t) * num_items_, hipMemcpyDeviceToHost, stream));
        BFH_HIP(hipStreamSynchronize(stream));
        stats.d2h_bytes += 8.0 * num_items_;
        // keys and values through the library's pinned ring: a plain hipMemcpy into pageable numpy memory costs several times the build's device time
        to_host(keys_out, d_key_out_.get(), sizeof(int32_t) * nnz_);
        to_host(vals_out, d_val_out_.get(), sizeof(float) * nnz_);
    }

 private:
    template <typename KeyT>
    void build_with(const int64_t* indptr, const int32_t* items, int num_users, int num_items, int windows, int k, int64_t* nnz_out, int64_t* lines_out) {
        BFH_REQUIRE(num_users > 0 && num_items > 0 && windows > 0 && k > 0, "sppmi: num_users, num_items, windows and k must be positive");
        ensure();
        const int64_t events = indptr[num_users - 1];
        int64_t prev = 0;
        for (int u = 0; u < num_users; ++u) {
            BFH_REQUIRE(indptr[u] >= prev, "sppmi: indptr must be non-decreasing END offsets");
            prev = indptr[u];
        }
        for (int64_t e = 0; e < events; ++e)
            if (items[e] < 0 || items[e] >= num_items) throw Error(BFH_ERR_INVALID, "sppmi: item id outside [0, num_items) at event " + std::to_string(e));
        num_items_ = num_items;
        nnz_ = 0;
        d_indptr_out_.resize(static_cast<size_t>(num_items));
        BFH_HIP(hipMemsetAsync(d_indptr_out_.get(), 0, d_indptr_out_.bytes(), stream));
        stats = bfh_stats{};
        int64_t total_pairs = 0;
        for (int u = 0; u < num_users; ++u) total_pairs += sppmi_pairs_of(indptr[u] - (u ? indptr[u - 1] : 0), windows);
        const int64_t lines = 2 * total_pairs;
        if (lines_out) *lines_out = lines;
        if (lines == 0) {
            BFH_HIP(hipStreamSynchronize(stream));
            if (nnz_out) *nnz_out = 0;
            return;
        }
        SppmiWork<KeyT> W;
        W.indptr.resize(num_users); W.pairs.resize(num_users); W.off.resize(num_users); W.items.resize(static_cast<size_t>(events));
        W.keys.resize(static_cast<size_t>(lines)); W.sorted.resize(static_cast<size_t>(lines)); W.app.resize(num_items);
        BFH_HIP(hipMemcpyAsync(W.indptr.get(), indptr, sizeof(int64_t) * num_users, hipMemcpyHostToDevice, stream));
        BFH_HIP(hipMemcpyAsync(W.items.get(), items, sizeof(int32_t) * events, hipMemcpyHostToDevice, stream));
        const int slot = t_main_.begin(stream);
        lines_per_user(W, num_users, windows);
        write_keys(W, num_users, events, windows);
        sort_and_runs(W, lines);
        appearances(W, lines);
        int64_t runs = 0;                                            // first wait: the number of distinct pairs
        BFH_HIP(hipMemcpyAsync(&runs, W.n_runs.get(), sizeof(int64_t), hipMemcpyDeviceToHost, stream));
        BFH_HIP(hipStreamSynchronize(stream));
        values_and_emits(W, runs, lines, k);
        nnz_ = scan_emits(W, runs);                                  // second wait
        scatter(W, runs);
        t_main_.end(slot, stream);
        BFH_HIP(hipStreamSynchronize(stream));   // W is freed on return
        stats.samples = lines;
        stats.launches = runs;                   // distinct pairs
        stats.kernel_ms = t_main_.drain();
        stats.h2d_bytes = 8.0 * num_users + 4.0 * events;
        if (nnz_out) *nnz_out = nnz_;
    }

    // step 1: pairs per user in closed form, exclusive scan -> where each user's lines start
    template <typename KeyT>
    void lines_per_user(SppmiWork<KeyT>& W, int num_users, int windows) {
        hipLaunchKernelGGL(sppmi_count_kernel, dim3(blocks_of(num_users)), dim3(256), 0, stream, W.indptr.get(), num_users, windows, W.pairs.get());
        BFH_HIP(hipGetLastError());
        exclusive_scan_i64(W.pairs.get(), W.off.get(), num_users, W.tmp, stream);
    }

    // step 2: one thread per event writes its lines as keys
    template <typename KeyT>
    void write_keys(SppmiWork<KeyT>& W, int num_users, int64_t events, int windows) {
        hipLaunchKernelGGL((sppmi_lines_kernel<KeyT>), dim3(blocks_of(events)), dim3(256), 0, stream, W.indptr.get(), W.items.get(), num_users, events, windows,
                           static_cast<uint64_t>(num_items_), W.off.get(), W.keys.get());
        BFH_HIP(hipGetLastError());
    }

    // step 3: sort over the bits the keys use; distinct pairs (at most `lines`) with their counts, the number of runs left on the device
    template <typename KeyT>
    void sort_and_runs(SppmiWork<KeyT>& W, int64_t lines) {
        const size_t n = static_cast<size_t>(lines);
        int bits = 1;
        while (bits < static_cast<int>(sizeof(KeyT)) * 8 && (uint64_t(1) << bits) < static_cast<uint64_t>(num_items_) * static_cast<uint64_t>(num_items_)) ++bits;
        device_sort_keys(W.keys.get(), W.sorted.get(), lines, bits, W.tmp, stream);
        W.uniq.resize(n); W.cnt.resize(n); W.n_runs.resize(1);
        device_run_length_encode(W.sorted.get(), lines, W.uniq.get(), W.cnt.get(), W.n_runs.get(), W.tmp, stream);
    }

    // step 4: appearances[id] = lines starting with id, by two binary searches per item in the sorted keys
    template <typename KeyT>
    void appearances(SppmiWork<KeyT>& W, int64_t lines) {
        hipLaunchKernelGGL((sppmi_appear_kernel<KeyT>), dim3(blocks_of(num_items_)), dim3(256), 0, stream, W.sorted.get(), lines, num_items_, W.app.get());
        BFH_HIP(hipGetLastError());
    }

    // step 5: one thread per distinct pair: value and emit count 0 / 1 / 2
    template <typename KeyT>
    void values_and_emits(SppmiWork<KeyT>& W, int64_t runs, int64_t lines, int k) {
        const size_t n = static_cast<size_t>(runs);
        W.val.resize(n); W.emit.resize(n); W.emit_off.resize(n);
        hipLaunchKernelGGL((sppmi_value_kernel<KeyT>), dim3(blocks_of(runs)), dim3(256), 0, stream, W.uniq.get(), W.cnt.get(), runs,
                           static_cast<uint64_t>(num_items_), W.app.get(), std::log(static_cast<double>(lines)), std::log(static_cast<double>(k)), W.val.get(),
                           W.emit.get());
        BFH_HIP(hipGetLastError());
    }

    // step 6, first half: where each pair's entries go; returns the number of entries
    template <typename KeyT>
    int64_t scan_emits(SppmiWork<KeyT>& W, int64_t runs) {
        exclusive_scan_i64(W.emit.get(), W.emit_off.get(), runs, W.tmp, stream);
        int64_t last_off = 0, last_emit = 0;
        BFH_HIP(hipMemcpyAsync(&last_off, W.emit_off.get() + (runs - 1), sizeof(int64_t), hipMemcpyDeviceToHost, stream));
        BFH_HIP(hipMemcpyAsync(&last_emit, W.emit.get() + (runs - 1), sizeof(int64_t), hipMemcpyDeviceToHost, stream));
        BFH_HIP(hipStreamSynchronize(stream));
        return last_off + last_emit;
    }

    // step 6, second half: the entries in (row, col) order and the END offsets from the row changes (all zero already when there is no entry)
    template <typename KeyT>
    void scatter(SppmiWork<KeyT>& W, int64_t runs) {
        if (nnz_ == 0) return;
        W.rows.resize(static_cast<size_t>(nnz_)); d_key_out_.resize(static_cast<size_t>(nnz_)); d_val_out_.resize(static_cast<size_t>(nnz_));
        hipLaunchKernelGGL((sppmi_scatter_kernel<KeyT>), dim3(blocks_of(runs)), dim3(256), 0, stream, W.uniq.get(), W.val.get(), W.emit_off.get(), runs, nnz_,
                           static_cast<uint64_t>(num_items_), W.rows.get(), d_key_out_.get(), d_val_out_.get());
        hipLaunchKernelGGL(csr_ends_kernel, dim3(blocks_of(nnz_)), dim3(256), 0, stream, W.rows.get(), nnz_, num_items_, d_indptr_out_.get());
        BFH_HIP(hipGetLastError());
    }

    int num_items_ = 0;
    int64_t nnz_ = 0;
    DevBuf<int64_t> d_indptr_out_;
    DevBuf<int32_t> d_key_out_;
    DevBuf<float> d_val_out_;
    EventTimer t_main_;
};

}  // namespace bfh

using bfh::guarded;
using bfh::SppmiHandle;

extern "C" {

BFH_ABI_CREATE_DESTROY_STATS(sppmi, SppmiHandle)

int bfh_sppmi_build(void* h, const int64_t* indptr, const int32_t* items, int num_users, int num_items, int windows, int k, int64_t* nnz,
                    int64_t* total_lines) {
    return guarded<SppmiHandle>(h, [&](SppmiHandle& s) { s.build(indptr, items, num_users, num_items, windows, k, nnz, total_lines); });
}
int bfh_sppmi_fetch(void* h, int64_t* indptr_out, int32_t* keys_out, float* vals_out) {
    return guarded<SppmiHandle>(h, [&](SppmiHandle& s) { s.fetch(indptr_out, keys_out, vals_out); });
}

}  // extern "C"
