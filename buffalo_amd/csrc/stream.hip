// Stream databases on the device (the Stream half) -- host steps + C ABI; the kernels are in stream_kernels.hpp, text_tiles.hpp (the marks)
// and csr_kernels.hpp (pair keys, END offsets).
//
// Reference semantics: Stream._create + Stream._create_working_data (/root/reference/buffalo/data/stream.py:81-158, 197-271): every line of
// the main file is a user, `line.strip().split()` are its events, every token is looked up in the dict the item-id file gives
// (:120-122), the validation events are split off (`newest`: the last n of a user, :224-231; `sample`: drawn global positions, :232-245),
// and the rest is written as the working file -- one line per event ("stream"), or one per distinct item with its count in order of first
// appearance (`Counter`, "matrix", :253-256).  W2V.build_vocab (buffalo/algo/w2v.py:91-100) then walks all events once more for the counts.
//
// Device formulation:
//   1. line ends and token starts by the count / scan / scatter over 4 KB tiles of text_tiles.hpp (two passes over the text);
//   2. one thread per token hashes its bytes (a third, partial pass: token bytes only) and looks the name up in an open-addressing table
//      built by compare-and-swap; its user is the number of line ends before it, which pass 1's scan already holds;
//   3. keep flags per event, an exclusive scan, a scatter: train events and held-out events, both in file order;
//   4. distinct (user, item) of a list in order of first appearance: stable radix sort by (user, item) with the position as payload, run
//      heads = first position + count, compacted, sorted by first position (global positions are monotone in the user: that IS the file
//      order) -- used for the records and for the held-out triples;
//   5. item counts by an LDS histogram per block, or global atomics beyond kStreamLdsBins items.
// The host waits three times per build: for the two mark counts, for (first unknown token, train events), for (records, held-out triples).
#include <climits>

#include "abi.hpp"
#include "builder_base.hpp"
#include "stream_kernels.hpp"

namespace bfh {

// d_flags_: word 0 = duplicate name (set_vocabulary) / first unknown token (build); from word kStreamProbeStride on, the probe counter's slots
constexpr size_t kFlagWords = static_cast<size_t>(kStreamProbeSlots + 1) * kStreamProbeStride;

// distinct (user, item) pairs of a device list, see step 4
struct DistinctPairs {
    DevBuf<uint64_t> keys, keys_sorted, run_key, run_first, run_first_sorted;
    DevBuf<int64_t> pos, pos_sorted, head, hidx, run_start, run_id, order;
    DevBuf<int32_t> rows, cols;
    DevBuf<float> vals;
    int64_t n = 0, runs = 0;
};

class StreamHandle : public BuilderHandle {
 public:
    StreamHandle() : BuilderHandle("stream") {}

    // ---------------------------------------------------------------- vocabulary ----------------------------------------------------------------
    void set_vocabulary(const char* names, int64_t bytes, int* num_items_out) {
        BFH_REQUIRE(bytes >= 0 && (names || bytes == 0), "stream: the item-id bytes are missing");
        ensure();
        built_ = false;
        have_vocab_ = false;
        t_aux_.timed(stream, [&] {
            upload_text(names, bytes, d_names_);
            const int64_t n_eol = index_text(d_names_, bytes, false, nullptr);
            const int64_t lines = n_eol + (ends_open(names, bytes) ? 1 : 0);
            BFH_REQUIRE(lines < INT_MAX, "stream: more than 2^31 - 1 item ids");
            num_items_ = static_cast<int>(lines);
            table_mask_ = 15;
            while (table_mask_ + 1 < 2 * static_cast<uint64_t>(num_items_)) table_mask_ = 2 * table_mask_ + 1;
            d_table_.resize(table_mask_ + 1, true, stream);
            d_flags_.resize(kFlagWords);
            const int no_dup = INT_MAX;
            BFH_HIP(hipMemcpyAsync(d_flags_.get(), &no_dup, sizeof(int), hipMemcpyHostToDevice, stream));
            if (num_items_ > 0) {
                d_name_beg_.resize(num_items_); d_name_len_.resize(num_items_); d_name_head_.resize(num_items_);
                hipLaunchKernelGGL(stream_names_kernel, dim3(blocks_of(num_items_)), dim3(256), 0, stream, d_names_.get(), bytes, d_eol_.get(), n_eol, num_items_,
                                   d_name_beg_.get(), d_name_len_.get(), d_name_head_.get());
                hipLaunchKernelGGL(stream_insert_kernel, dim3(blocks_of(num_items_)), dim3(256), 0, stream, d_names_.get(), d_name_beg_.get(), d_name_len_.get(),
                                   num_items_, d_table_.get(), table_mask_, reinterpret_cast<int*>(d_flags_.get()));
                BFH_HIP(hipGetLastError());
            }
        });
        int dup = INT_MAX;
        BFH_HIP(hipMemcpyAsync(&dup, d_flags_.get(), sizeof(int), hipMemcpyDeviceToHost, stream));
        BFH_HIP(hipStreamSynchronize(stream));
        stats.aux_ms += t_aux_.drain();
        stats.h2d_bytes += static_cast<double>(bytes);
        BFH_REQUIRE(dup == INT_MAX, "stream: the item-id file holds a name twice (line " + std::to_string(dup + 1) +
                                        " repeats an earlier one); the reference's dict would drop one id (stream.py:120-122)");
        have_vocab_ = true;
        if (num_items_out) *num_items_out = num_items_;
    }

    // ---------------------------------------------------------------- build ----------------------------------------------------------------
    void build(const char* text, int64_t bytes, int vali_n, const int64_t* sample_pos, int64_t n_sample, int64_t out_counts[5]) {
        built_ = false;
        BFH_REQUIRE(have_vocab_, "stream: build before set_vocabulary");
        BFH_REQUIRE(bytes >= 0 && (text || bytes == 0), "stream: the text bytes are missing");
        BFH_REQUIRE(vali_n >= 0 && n_sample >= 0, "stream: vali_n and n_sample must not be negative");
        BFH_REQUIRE(!(vali_n > 0 && sample_pos), "stream: `newest` (vali_n > 0) and `sample` (positions) exclude each other (stream.py:199-204)");
        ensure();
        try {
            tokenise(text, bytes);
            check_positions(sample_pos, n_sample);
            lookup(text, bytes);
            split(vali_n, sample_pos, n_sample);
            finish_split(text, bytes);
            count_items();
            distinct_begin(d_train_user_.get(), d_train_item_.get(), num_train_, records_);
            distinct_begin(d_held_user_.get(), d_held_item_.get(), num_events_ - num_train_, vali_);
            read_runs();
            distinct_end(records_, false);
            distinct_end(vali_, sample_pos == nullptr);   // `newest`: the held list is the user's distinct items, each once (:229-231)
            BFH_HIP(hipStreamSynchronize(stream));
        } catch (...) {
            (void)hipStreamSynchronize(stream);
            (void)t_kernel_.drain();
            (void)t_aux_.drain();
            throw;
        }
        stats.kernel_ms += t_kernel_.drain();
        stats.aux_ms += t_aux_.drain();
        stats.samples += num_events_;
        stats.accepted += num_train_;
        stats.merges += records_.runs;
        stats.h2d_bytes += static_cast<double>(bytes) + 8.0 * n_sample;
        built_ = true;
        if (out_counts) {
            out_counts[0] = num_users_;
            out_counts[1] = num_events_;
            out_counts[2] = num_train_;
            out_counts[3] = records_.runs;
            out_counts[4] = vali_.runs;
        }
    }

    // ---------------------------------------------------------------- fetches ----------------------------------------------------------------
    void fetch_events(int64_t* indptr, int32_t* items) {
        need_build();
        to_host(indptr, d_train_ends_.get(), 8 * static_cast<size_t>(num_users_));
        to_host(items, d_train_item_.get(), 4 * static_cast<size_t>(num_train_));
    }
    void fetch_records(int32_t* rows, int32_t* cols, float* vals) {
        need_build();
        fetch_triples(records_, rows, cols, vals);
    }
    void fetch_vali(int32_t* rows, int32_t* cols, float* vals) {
        need_build();
        fetch_triples(vali_, rows, cols, vals);
    }
    void fetch_counts(int64_t* counts) {
        need_build();
        to_host(counts, d_counts_.get(), 8 * static_cast<size_t>(num_items_));
    }
    void fetch_group(int sort_key, int64_t max_records, int64_t* indptr, int32_t* keys, float* vals) {
        need_build();
        BFH_REQUIRE(sort_key == 1 || sort_key == 2, "stream: sort_key is 1 (rowwise) or 2 (colwise)");
        const int64_t cut = max_records < 0 ? records_.runs : std::min(max_records, records_.runs);
        const int num_major = sort_key == 1 ? static_cast<int>(num_users_) : num_items_;
        if (num_major == 0) return;
        if (cut == 0) {   // no record: every END offset is zero
            grow(group_.indptr, static_cast<size_t>(num_major));
            BFH_HIP(hipMemsetAsync(group_.indptr.get(), 0, 8 * static_cast<size_t>(num_major), stream));
            to_host(indptr, group_.indptr.get(), 8 * static_cast<size_t>(num_major));
            return;
        }
        const int32_t* major = sort_key == 1 ? records_.rows.get() : records_.cols.get();
        const int32_t* minor = sort_key == 1 ? records_.cols.get() : records_.rows.get();
        group_.fetch(*this, t_aux_, d_tmp_, major, minor, records_.vals.get(), cut, num_major, indptr, keys, vals);
        stats.aux_ms += t_aux_.drain();
    }

 private:
    // a last line without a terminator counts as a line (Python's file iteration)
    static bool ends_open(const char* text, int64_t bytes) { return bytes > 0 && text[bytes - 1] != '\n' && text[bytes - 1] != '\r'; }

    // count / scan / scatter: d_eol_ = line ends, d_tok_ = token starts (when asked for).  Waits for the two totals; returns the line ends.
    int64_t index_text(const DevBuf<char>& d, int64_t bytes, bool with_tokens, int64_t* n_tok_out) {
        const int64_t tiles = text_tiles_of(bytes);
        int64_t totals[2] = {0, 0};
        if (tiles > 0) {
            grow(d_tile_tok_, static_cast<size_t>(tiles + 1)); grow(d_tile_eol_, static_cast<size_t>(tiles + 1));
            grow(d_base_tok_, static_cast<size_t>(tiles + 1)); grow(d_base_eol_, static_cast<size_t>(tiles + 1));
            BFH_HIP(hipMemsetAsync(d_tile_tok_.get() + tiles, 0, sizeof(int64_t), stream));
            BFH_HIP(hipMemsetAsync(d_tile_eol_.get() + tiles, 0, sizeof(int64_t), stream));
            hipLaunchKernelGGL((text_count_marks_kernel<true>), dim3(static_cast<unsigned>(tiles)), dim3(256), 0, stream, d.get(), bytes, d_tile_tok_.get(), d_tile_eol_.get());
            BFH_HIP(hipGetLastError());
            exclusive_scan_i64(d_tile_tok_.get(), d_base_tok_.get(), tiles + 1, d_tmp_, stream);
            exclusive_scan_i64(d_tile_eol_.get(), d_base_eol_.get(), tiles + 1, d_tmp_, stream);
            BFH_HIP(hipMemcpyAsync(&totals[0], d_base_tok_.get() + tiles, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
            BFH_HIP(hipMemcpyAsync(&totals[1], d_base_eol_.get() + tiles, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
            BFH_HIP(hipStreamSynchronize(stream));
            stats.d2h_bytes += 16.0;
            grow(d_eol_, static_cast<size_t>(std::max<int64_t>(1, totals[1])));
            if (with_tokens) {
                grow(d_tok_, static_cast<size_t>(std::max<int64_t>(1, totals[0])));
                grow(d_user_, static_cast<size_t>(std::max<int64_t>(1, totals[0])));
            }
            hipLaunchKernelGGL((text_write_marks_kernel<true>), dim3(static_cast<unsigned>(tiles)), dim3(256), 0, stream, d.get(), bytes, d_base_tok_.get(),
                               d_base_eol_.get(), totals[0], totals[1], with_tokens ? d_tok_.get() : nullptr, d_user_.get(), d_eol_.get());
            BFH_HIP(hipGetLastError());
        }
        if (n_tok_out) *n_tok_out = totals[0];
        return totals[1];
    }

    void tokenise(const char* text, int64_t bytes) {
        t_aux_.timed(stream, [&] { upload_text(text, bytes, d_text_); });
        t_kernel_.timed(stream, [&] { n_eol_ = index_text(d_text_, bytes, true, &num_events_); });
        num_users_ = n_eol_ + (ends_open(text, bytes) ? 1 : 0);
        BFH_REQUIRE(num_users_ < INT_MAX && num_events_ < INT_MAX, "stream: more than 2^31 - 1 users or events");
    }

    void check_positions(const int64_t* pos, int64_t n) const {
        if (!pos) return;
        for (int64_t j = 0; j < n; ++j) {
            BFH_REQUIRE(pos[j] >= 0 && pos[j] < num_events_, "stream: sample position " + std::to_string(pos[j]) + " is outside the " +
                                                                 std::to_string(num_events_) + " events");
            BFH_REQUIRE(j == 0 || pos[j] > pos[j - 1], "stream: sample positions must be ascending (position " + std::to_string(j) + " is not)");
        }
    }

    void lookup(const char* text, int64_t bytes) {
        const int64_t n = num_events_;
        d_flags_.resize(kFlagWords, true, stream);           // the probe slots start at zero
        BFH_HIP(hipMemsetAsync(d_flags_.get(), 0xff, sizeof(unsigned long long), stream));   // first unknown token: none
        if (n == 0) return;
        grow(d_item_, static_cast<size_t>(n));
        t_kernel_.timed(stream, [&] {
            hipLaunchKernelGGL(stream_lookup_kernel, dim3(blocks_of(n)), dim3(256), 0, stream, d_text_.get(), bytes, d_tok_.get(), n, d_names_.get(),
                               d_name_beg_.get(), d_name_len_.get(), d_name_head_.get(), d_table_.get(), table_mask_, d_item_.get(), d_flags_.get(),
                               d_flags_.get() + kStreamProbeStride);
            BFH_HIP(hipGetLastError());
        });
    }

    // keep flags -> train / held lists in file order, END offsets of the train events per user
    void split(int vali_n, const int64_t* sample_pos, int64_t n_sample) {
        const int64_t n = num_events_;
        grow(d_keep_, static_cast<size_t>(n + 1)); grow(d_kept_, static_cast<size_t>(n + 1));
        grow(d_train_ends_, static_cast<size_t>(std::max<int64_t>(1, num_users_)));
        if (n == 0) {
            BFH_HIP(hipMemsetAsync(d_train_ends_.get(), 0, d_train_ends_.bytes(), stream));
            BFH_HIP(hipMemsetAsync(d_kept_.get(), 0, sizeof(int64_t), stream));
            return;
        }
        grow(d_train_user_, static_cast<size_t>(n)); grow(d_train_item_, static_cast<size_t>(n));
        grow(d_held_user_, static_cast<size_t>(n)); grow(d_held_item_, static_cast<size_t>(n));
        t_aux_.timed(stream, [&] {
            if (vali_n > 0) {
                grow(d_ends_, static_cast<size_t>(num_users_));
                hipLaunchKernelGGL(csr_ends_kernel, dim3(blocks_of(n)), dim3(256), 0, stream, d_user_.get(), n, static_cast<int>(num_users_), d_ends_.get());
                hipLaunchKernelGGL(stream_hold_newest_kernel, dim3(blocks_of(n)), dim3(256), 0, stream, d_user_.get(), d_ends_.get(), n, vali_n, d_keep_.get());
            } else {
                hipLaunchKernelGGL(stream_fill_kernel, dim3(blocks_of(n)), dim3(256), 0, stream, d_keep_.get(), n, int64_t(1));
                if (sample_pos && n_sample > 0) {
                    grow(d_sample_, static_cast<size_t>(n_sample));
                    BFH_HIP(hipMemcpyAsync(d_sample_.get(), sample_pos, 8 * static_cast<size_t>(n_sample), hipMemcpyHostToDevice, stream));
                    hipLaunchKernelGGL(stream_hold_sample_kernel, dim3(blocks_of(n_sample)), dim3(256), 0, stream, d_sample_.get(), n_sample, d_keep_.get());
                }
            }
            BFH_HIP(hipGetLastError());
            BFH_HIP(hipMemsetAsync(d_keep_.get() + n, 0, sizeof(int64_t), stream));
            exclusive_scan_i64(d_keep_.get(), d_kept_.get(), n + 1, d_tmp_, stream);
            hipLaunchKernelGGL(stream_split_kernel, dim3(blocks_of(n)), dim3(256), 0, stream, d_user_.get(), d_item_.get(), d_keep_.get(), d_kept_.get(), n,
                               d_train_user_.get(), d_train_item_.get(), d_held_user_.get(), d_held_item_.get());
            BFH_HIP(hipGetLastError());
        });
    }

    // second wait: the first unknown token (the reference's KeyError, stream.py:230, 234, 241) and the number of train events
    void finish_split(const char* text, int64_t bytes) {
        std::vector<unsigned long long> flags(kFlagWords, 0ull);
        BFH_HIP(hipMemcpyAsync(flags.data(), d_flags_.get(), kFlagWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
        BFH_HIP(hipMemcpyAsync(&num_train_, d_kept_.get() + num_events_, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
        BFH_HIP(hipStreamSynchronize(stream));
        stats.d2h_bytes += 8.0 * kFlagWords + 8.0;
        for (int s = 0; s < kStreamProbeSlots; ++s) stats.loaded_rows += static_cast<int64_t>(flags[static_cast<size_t>(s + 1) * kStreamProbeStride]);
        if (flags[0] != ~0ull) {
            int64_t pos = 0;
            int32_t user = 0;
            BFH_HIP(hipMemcpyAsync(&pos, d_tok_.get() + flags[0], sizeof(pos), hipMemcpyDeviceToHost, stream));
            BFH_HIP(hipMemcpyAsync(&user, d_user_.get() + flags[0], sizeof(user), hipMemcpyDeviceToHost, stream));
            BFH_HIP(hipStreamSynchronize(stream));
            int64_t end = pos;
            while (end < bytes && !stream_space(static_cast<unsigned char>(text[end])) && end - pos < 64) ++end;
            throw Error(BFH_ERR_INVALID, "stream: line " + std::to_string(user + 1) + ": '" + std::string(text + pos, text + end) +
                                             "' is not in the item-id file (the reference's KeyError, stream.py:230-241)");
        }
        if (num_events_ > 0 && num_users_ > 0) {
            t_aux_.timed(stream, [&] {
                if (num_train_ > 0) {
                    hipLaunchKernelGGL(csr_ends_kernel, dim3(blocks_of(num_train_)), dim3(256), 0, stream, d_train_user_.get(), num_train_,
                                       static_cast<int>(num_users_), d_train_ends_.get());
                    BFH_HIP(hipGetLastError());
                } else {
                    BFH_HIP(hipMemsetAsync(d_train_ends_.get(), 0, 8 * static_cast<size_t>(num_users_), stream));
                }
            });
        }
    }

    void count_items() {
        grow(d_counts_, static_cast<size_t>(std::max(1, num_items_)));
        BFH_HIP(hipMemsetAsync(d_counts_.get(), 0, d_counts_.bytes(), stream));
        const int64_t n = num_train_;
        if (n == 0) return;
        t_aux_.timed(stream, [&] {
            if (num_items_ <= kStreamLdsBins) {
                // a small histogram leaves room for several blocks per CU; a large one takes the CU's LDS: one block per CU, 256 CUs
                const unsigned blocks = static_cast<unsigned>(std::min<int64_t>(blocks_of(n), num_items_ <= kStreamSmallBins ? 1024 : 256));
                const int lds = 4 * num_items_;
                BFH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(stream_counts_lds_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 4 * kStreamLdsBins));
                hipLaunchKernelGGL(stream_counts_lds_kernel, dim3(blocks), dim3(256), lds, stream, d_train_item_.get(), n, num_items_, d_counts_.get());
            } else {
                hipLaunchKernelGGL(stream_counts_global_kernel, dim3(blocks_of(n)), dim3(256), 0, stream, d_train_item_.get(), n, d_counts_.get());
            }
            BFH_HIP(hipGetLastError());
        });
    }

    // step 4 up to the number of runs (left on the device in hidx[n])
    void distinct_begin(const int32_t* user, const int32_t* item, int64_t n, DistinctPairs& D) {
        D.n = n;
        D.runs = 0;
        if (n == 0) return;
        const size_t sz = static_cast<size_t>(n);
        grow(D.keys, sz); grow(D.keys_sorted, sz); grow(D.pos, sz); grow(D.pos_sorted, sz); grow(D.head, sz + 1); grow(D.hidx, sz + 1);
        t_aux_.timed(stream, [&] {
            hipLaunchKernelGGL(csr_pack_kernel, dim3(blocks_of(n)), dim3(256), 0, stream, user, item, n, D.keys.get(), D.pos.get());
            BFH_HIP(hipGetLastError());
            device_sort_pairs_u64(D.keys.get(), D.keys_sorted.get(), D.pos.get(), D.pos_sorted.get(), n, 32 + bits_for(num_users_), d_tmp_, stream);
            hipLaunchKernelGGL(stream_heads_kernel, dim3(blocks_of(n + 1)), dim3(256), 0, stream, D.keys_sorted.get(), n, D.head.get());
            BFH_HIP(hipGetLastError());
            exclusive_scan_i64(D.head.get(), D.hidx.get(), n + 1, d_tmp_, stream);
        });
    }

    // third wait: the numbers of records and of held-out triples
    void read_runs() {
        if (records_.n > 0) BFH_HIP(hipMemcpyAsync(&records_.runs, records_.hidx.get() + records_.n, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
        if (vali_.n > 0) BFH_HIP(hipMemcpyAsync(&vali_.runs, vali_.hidx.get() + vali_.n, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
        BFH_HIP(hipStreamSynchronize(stream));
        stats.d2h_bytes += 16.0;
    }

    void distinct_end(DistinctPairs& D, bool unit_vals) {
        const int64_t n = D.n, m = D.runs;
        if (m == 0) return;
        const size_t sz = static_cast<size_t>(m);
        grow(D.run_key, sz); grow(D.run_first, sz); grow(D.run_first_sorted, sz); grow(D.run_start, sz + 1); grow(D.run_id, sz); grow(D.order, sz);
        grow(D.rows, sz); grow(D.cols, sz); grow(D.vals, sz);
        t_aux_.timed(stream, [&] {
            hipLaunchKernelGGL(stream_runs_kernel, dim3(blocks_of(n)), dim3(256), 0, stream, D.keys_sorted.get(), D.pos_sorted.get(), D.head.get(), D.hidx.get(), n, m,
                               D.run_key.get(), D.run_first.get(), D.run_start.get(), D.run_id.get());
            BFH_HIP(hipGetLastError());
            device_sort_pairs_u64(D.run_first.get(), D.run_first_sorted.get(), D.run_id.get(), D.order.get(), m, bits_for(n), d_tmp_, stream);
            hipLaunchKernelGGL(stream_emit_kernel, dim3(blocks_of(m)), dim3(256), 0, stream, D.order.get(), D.run_key.get(), D.run_start.get(), m, unit_vals ? 1 : 0,
                               D.rows.get(), D.cols.get(), D.vals.get());
            BFH_HIP(hipGetLastError());
        });
    }

    void fetch_triples(const DistinctPairs& D, int32_t* rows, int32_t* cols, float* vals) {
        const size_t b = 4 * static_cast<size_t>(D.runs);
        to_host(rows, D.rows.get(), b);
        to_host(cols, D.cols.get(), b);
        to_host(vals, D.vals.get(), b);
    }

    bool have_vocab_ = false;
    int num_items_ = 0;
    uint64_t table_mask_ = 0;
    int64_t num_users_ = 0, num_events_ = 0, num_train_ = 0, n_eol_ = 0;
    DevBuf<char> d_names_, d_text_, d_tmp_;
    DevBuf<int64_t> d_name_beg_, d_tile_tok_, d_tile_eol_, d_base_tok_, d_base_eol_, d_tok_, d_eol_, d_ends_, d_train_ends_, d_keep_, d_kept_, d_sample_;
    DevBuf<int32_t> d_name_len_, d_user_, d_item_, d_train_user_, d_train_item_, d_held_user_, d_held_item_;
    DevBuf<unsigned long long> d_table_, d_flags_, d_counts_;
    DevBuf<uint64_t> d_name_head_;
    DistinctPairs records_, vali_;
    GroupFetch group_;
    EventTimer t_kernel_, t_aux_;
};

}  // namespace bfh

using bfh::guarded;
using bfh::StreamHandle;

extern "C" {

BFH_ABI_LIFECYCLE(stream, StreamHandle)

int bfh_stream_set_vocabulary(void* h, const char* names, int64_t bytes, int* num_items) {
    return guarded<StreamHandle>(h, [&](StreamHandle& s) { s.set_vocabulary(names, bytes, num_items); });
}
int bfh_stream_build(void* h, const char* text, int64_t bytes, int vali_n, const int64_t* sample_pos, int64_t n_sample, int64_t out_counts[5]) {
    return guarded<StreamHandle>(h, [&](StreamHandle& s) { s.build(text, bytes, vali_n, sample_pos, n_sample, out_counts); });
}
int bfh_stream_fetch_events(void* h, int64_t* indptr, int32_t* items) {
    return guarded<StreamHandle>(h, [&](StreamHandle& s) { s.fetch_events(indptr, items); });
}
int bfh_stream_fetch_records(void* h, int32_t* rows, int32_t* cols, float* vals) {
    return guarded<StreamHandle>(h, [&](StreamHandle& s) { s.fetch_records(rows, cols, vals); });
}
int bfh_stream_fetch_group(void* h, int sort_key, int64_t max_records, int64_t* indptr, int32_t* keys, float* vals) {
    return guarded<StreamHandle>(h, [&](StreamHandle& s) { s.fetch_group(sort_key, max_records, indptr, keys, vals); });
}
int bfh_stream_fetch_vali(void* h, int32_t* rows, int32_t* cols, float* vals) {
    return guarded<StreamHandle>(h, [&](StreamHandle& s) { s.fetch_vali(rows, cols, vals); });
}
int bfh_stream_fetch_counts(void* h, int64_t* counts) {
    return guarded<StreamHandle>(h, [&](StreamHandle& s) { s.fetch_counts(counts); });
}

}  // extern "C"
