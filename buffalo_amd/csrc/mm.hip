// MatrixMarket databases on the device (the MatrixMarket half) -- host steps + C ABI; the kernels are in
// mm_kernels.hpp, text_tiles.hpp (line ends) and csr_kernels.hpp (pair keys), the text parser is ingest.hip's (parse_lines_on_device).
//
// Reference semantics: MatrixMarket.create (/root/reference/buffalo/data/mm.py:236-279): the leading "%" lines are skipped (:154-159,
// :248-251), the next line is "num_users num_items num_nnz", the first num_nnz body lines are the entries; the `sample` split takes the
// lines at the drawn positions out in ascending order (base.py:210-238, mm.py:167-234), the rest is the working file, which
// _build_data (base.py:399-451) sorts and compresses once per orientation (fileio.hpp:263-420); one value_prepro object
// (buffalo/data/prepro.py) sees the rowwise values, the held-out values and the colwise values in this order, and the held-out values
// pass through csr_matrix((val, (row, col))).data, which lists them by (row, col) (base.py:240-253).
//
// Device formulation:
//   1. line ends by the count / scan / scatter over 4 KB tiles of text_tiles.hpp, with the Stream builder's rule ("\n", "\r\n", lone "\r");
//   2. the device parser over the body lines [0, header_nnz), once (lines it cannot guarantee: the host's sscanf, scattered back);
//   3. every body line to its train or held-out slot, ids 0-based and checked against the matrix.  The held positions arrive sorted, so the
//      held lines before a line are a binary search: no flag array, no scan;
//   4. value_prepro: min / max of the train values and of the held-out values by integer atomics on the ordered bit pattern, then the
//      scale kernel (four separately rounded binary32 operations) once per group -- the colwise group with the range the held-out values
//      widened --, or the ImplicitALS kernel, or the fill with 1;
//   5. held-out triples: stable radix sort by (row, col) with the position as payload, neighbours compared for a pair listed twice, the
//      values permuted into that order and transformed;
//   6. a group = the train triples through csr_from_device_coo, made when it is fetched.
// The held-out values are parsed like all others (strtof).  The reference reads them with Python's float() and narrows to binary32; the
// two differ only for a decimal string within 2^-53 (relative) of the midpoint of two neighbouring binary32 values.
// The host waits four times per build: for the number of line ends, for the parser's list of lines to re-parse, for (ids outside the
// matrix, the two value ranges, a repeated held-out pair), and at the end.
#include <climits>
#include <limits>

#include "abi.hpp"
#include "builder_base.hpp"
#include "mm_kernels.hpp"

namespace bfh {

enum class Prepro { kNone, kOneBased, kMinMaxScalar, kImplicitALS };

// d_flags_ words: the parser's re-parse count, ids outside the matrix, the first repeated held-out pair, {min, max} of the train values,
// {min, max} of the held-out values (two 32-bit words in each of the last two)
enum { kRedo = 0, kBad = 1, kDup = 2, kTrainRange = 3, kHeldRange = 4, kFlagWords = 5 };

class MMHandle : public BuilderHandle {
 public:
    MMHandle() : BuilderHandle("mm") {}

    void set_value_prepro(const char* name, double a, double b) {
        const std::string n = name ? name : "";
        if (n.empty()) {
            prepro_ = Prepro::kNone;
        } else if (n == "OneBased") {
            prepro_ = Prepro::kOneBased;
        } else if (n == "MinMaxScalar") {
            BFH_REQUIRE(std::isfinite(a) && std::isfinite(b), "mm: MinMaxScalar needs finite min and max");
            prepro_ = Prepro::kMinMaxScalar;
        } else if (n == "ImplicitALS") {
            BFH_REQUIRE(a > 0.0 && static_cast<float>(a) > 0.f && std::isfinite(static_cast<float>(a)), "mm: ImplicitALS needs epsilon > 0");
            prepro_ = Prepro::kImplicitALS;
        } else {
            throw Error(BFH_ERR_UNSUPPORTED, n == "SPPMI" ? "mm: SPPMI does not support MatrixMarket (mm.py:104-106)"
                                                          : "mm: unknown value_prepro '" + n + "' (OneBased, MinMaxScalar, ImplicitALS)");
        }
        opt_a_ = a;
        opt_b_ = b;
    }

    void set_mode(const char* name, int64_t value) {
        BFH_REQUIRE(name && std::string(name) == "vali_file_order", std::string("mm: unknown mode '") + (name ? name : "") + "'");
        BFH_REQUIRE(value == 0 || value == 1, "mm: vali_file_order is 0 or 1");
        vali_file_order_ = value != 0;
    }

    // ---------------------------------------------------------------- build ----------------------------------------------------------------
    void build(const char* text, int64_t bytes, const int64_t* sample_pos, int64_t n_sample, int64_t out_counts[6]) {
        built_ = false;
        BFH_REQUIRE(text && bytes > 0, "mm: the text bytes are missing");
        BFH_REQUIRE(n_sample >= 0 && (sample_pos || n_sample == 0), "mm: the sample positions are missing");
        ensure();
        read_header(text, bytes);
        check_positions(sample_pos, n_sample);
        num_vali_ = n_sample;
        num_train_ = header_nnz_ - n_sample;
        int64_t reparsed = 0;
        try {
            line_ends(text, bytes);
            reparsed = parse(text, bytes);
            split(sample_pos);
            measure_values();
            sort_held();
            read_flags(sample_pos);
            transform_values();
            BFH_HIP(hipStreamSynchronize(stream));
        } catch (...) {
            (void)hipStreamSynchronize(stream);
            (void)t_kernel_.drain();
            (void)t_aux_.drain();
            (void)hipGetLastError();   // a pair of events the failure left half recorded: not the next call's error
            throw;
        }
        stats.kernel_ms += t_kernel_.drain();
        stats.aux_ms += t_aux_.drain();
        stats.samples += header_nnz_;
        stats.accepted += num_train_;
        stats.merges += reparsed;
        stats.h2d_bytes += static_cast<double>(bytes) + 8.0 * n_sample;
        built_ = true;
        if (out_counts) {
            out_counts[0] = num_users_;
            out_counts[1] = num_items_;
            out_counts[2] = header_nnz_;
            out_counts[3] = header_lines_;
            out_counts[4] = num_train_;
            out_counts[5] = num_vali_;
        }
    }

    // ---------------------------------------------------------------- fetches ----------------------------------------------------------------
    void fetch_group(int sort_key, int64_t* indptr, int32_t* keys, float* vals) {
        need_build();
        BFH_REQUIRE(sort_key == 1 || sort_key == 2, "mm: sort_key is 1 (rowwise) or 2 (colwise)");
        const int num_major = sort_key == 1 ? num_users_ : num_items_;
        const int32_t* major = sort_key == 1 ? d_train_row_.get() : d_train_col_.get();
        const int32_t* minor = sort_key == 1 ? d_train_col_.get() : d_train_row_.get();
        const float* v = sort_key == 2 && built_prepro_ == Prepro::kMinMaxScalar ? d_vals_col_.get() : d_vals_row_.get();
        group_.fetch(*this, t_aux_, d_tmp_, major, minor, v, num_train_, num_major, indptr, keys, vals);   // num_train_ > 0: the last line is never held out
        stats.aux_ms += t_aux_.drain();
    }
    void fetch_vali(int32_t* rows, int32_t* cols, float* vals) {
        need_build();
        const size_t b = 4 * static_cast<size_t>(num_vali_);
        to_host(rows, d_held_row_.get(), b);
        to_host(cols, d_held_col_.get(), b);
        to_host(vals, d_vali_val_.get(), b);
    }
    void fetch_value_range(float out[4]) {
        need_build();
        BFH_REQUIRE(built_prepro_ == Prepro::kMinMaxScalar, "mm: a value range exists only with MinMaxScalar");
        BFH_REQUIRE(out != nullptr, "mm: an output array is missing");
        std::memcpy(out, range_, sizeof(range_));
    }

 private:
    // One line as Python's text mode hands it out: [beg, end) without the terminator, `next` = where the following line begins.
    static bool next_line(const char* text, int64_t bytes, int64_t beg, int64_t& end, int64_t& next) {
        if (beg >= bytes) return false;
        int64_t e = beg;
        while (e < bytes && text[e] != '\n' && text[e] != '\r') ++e;
        end = e;
        next = e < bytes ? e + ((text[e] == '\r' && e + 1 < bytes && text[e + 1] == '\n') ? 2 : 1) : e;
        return true;
    }

    // mm.py:154-159 counts the leading lines whose STRIPPED form starts with "%", mm.py:248-251 takes the first line that does not start
    // with "%" as it stands for the size line.  Both must name the same line.
    void read_header(const char* text, int64_t bytes) {
        int64_t beg = 0, end = 0, next = 0, line = 0;
        for (;; beg = next, ++line) {
            BFH_REQUIRE(next_line(text, bytes, beg, end, next), "mm: the file ends after " + std::to_string(line) + " comment lines: no size line");
            int64_t b = beg;
            while (b < end && stream_space(static_cast<unsigned char>(text[b]))) ++b;
            if (!(b < end && text[b] == '%')) break;
            BFH_REQUIRE(b == beg, "mm: line " + std::to_string(line + 1) + " has white space in front of its '%': mm.py:156 skips it as a comment, " +
                                      "mm.py:250 reads it as the size line");
        }
        // map(int, H.split()) (mm.py:119): exactly three integers
        int64_t v[3] = {0, 0, 0};
        int n = 0;
        bool ok = true;
        for (int64_t i = beg; i < end && ok;) {
            if (stream_space(static_cast<unsigned char>(text[i]))) { ++i; continue; }
            if (n == 3) { ok = false; break; }
            if (text[i] == '+') ++i;
            int digits = 0;
            int64_t x = 0;
            for (; i < end && text[i] >= '0' && text[i] <= '9'; ++i, ++digits) {
                ok = ok && x < (int64_t(1) << 56);
                x = x * 10 + (text[i] - '0');
            }
            ok = ok && digits > 0 && (i == end || stream_space(static_cast<unsigned char>(text[i])));
            v[n++] = x;
        }
        BFH_REQUIRE(ok && n == 3, "mm: line " + std::to_string(line + 1) + " is not the size line 'num_users num_items num_nnz'");
        BFH_REQUIRE(v[0] > 0 && v[1] > 0 && v[2] > 0 && v[0] < INT_MAX && v[1] < INT_MAX,
                    "mm: line " + std::to_string(line + 1) + ": an empty matrix, or more than 2^31 - 1 users or items");
        num_users_ = static_cast<int>(v[0]);
        num_items_ = static_cast<int>(v[1]);
        header_nnz_ = v[2];
        header_lines_ = line + 1;
    }

    void check_positions(const int64_t* pos, int64_t n) const {
        for (int64_t j = 0; j < n; ++j) {
            BFH_REQUIRE(pos[j] >= 0 && pos[j] < header_nnz_ - 1, "mm: sample position " + std::to_string(pos[j]) + " is outside [0, num_nnz - 1) = [0, " +
                                                                     std::to_string(header_nnz_ - 1) + "): the last line is never held out (base.py:224-226)");
            BFH_REQUIRE(j == 0 || pos[j] > pos[j - 1], "mm: sample positions must be strictly ascending (position " + std::to_string(j) + " is not)");
        }
    }

    // step 1.  First wait: the number of line ends
    void line_ends(const char* text, int64_t bytes) {
        const int64_t tiles = text_tiles_of(bytes);
        t_aux_.timed(stream, [&] { upload_text(text, bytes, d_text_); });
        int64_t n_eol = 0;
        t_kernel_.timed(stream, [&] {
            grow(d_tile_eol_, static_cast<size_t>(tiles + 1)); grow(d_base_eol_, static_cast<size_t>(tiles + 1));
            BFH_HIP(hipMemsetAsync(d_tile_eol_.get() + tiles, 0, sizeof(int64_t), stream));
            hipLaunchKernelGGL((text_count_marks_kernel<false>), dim3(static_cast<unsigned>(tiles)), dim3(256), 0, stream, d_text_.get(), bytes,
                               static_cast<int64_t*>(nullptr), d_tile_eol_.get());   // no tokens here
            BFH_HIP(hipGetLastError());
            exclusive_scan_i64(d_tile_eol_.get(), d_base_eol_.get(), tiles + 1, d_tmp_, stream);
        });
        BFH_HIP(hipMemcpyAsync(&n_eol, d_base_eol_.get() + tiles, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
        BFH_HIP(hipStreamSynchronize(stream));
        stats.d2h_bytes += 8.0;
        const int64_t lines_in_file = n_eol + ((text[bytes - 1] != '\n' && text[bytes - 1] != '\r') ? 1 : 0);
        BFH_REQUIRE(lines_in_file - header_lines_ >= header_nnz_,
                    "mm: the file ends with line " + std::to_string(lines_in_file) + ", that is " + std::to_string(lines_in_file - header_lines_) +
                        " body lines; the size line (line " + std::to_string(header_lines_) + ") says " + std::to_string(header_nnz_) +
                        " (the reference aborts in fileio.hpp:325)");
        n_ends_ = std::min(n_eol, header_lines_ + header_nnz_);   // only the first num_nnz body lines count
        t_kernel_.timed(stream, [&] {
            grow(d_eol_, static_cast<size_t>(n_ends_));
            hipLaunchKernelGGL((text_write_marks_kernel<false>), dim3(static_cast<unsigned>(tiles)), dim3(256), 0, stream, d_text_.get(), bytes,
                               static_cast<const int64_t*>(nullptr), d_base_eol_.get(), int64_t(0), n_ends_, static_cast<int64_t*>(nullptr),
                               static_cast<int32_t*>(nullptr), d_eol_.get());
            BFH_HIP(hipGetLastError());
        });
    }

    // step 2.  Second wait (inside the parser): the lines to re-parse on the host
    int64_t parse(const char* text, int64_t bytes) {
        const size_t n = static_cast<size_t>(header_nnz_);
        grow(d_r_, n); grow(d_c_, n); grow(d_v_, n);
        d_flags_.resize(kFlagWords, true, stream);
        ParsedLines p;
        t_kernel_.timed(stream, [&] {
            p = parse_lines_on_device(text, d_text_.get(), bytes, d_eol_.get(), n_ends_, header_lines_, header_nnz_, d_r_.get(), d_c_.get(), d_v_.get(), d_redo_,
                                      d_flags_.get() + kRedo, stream);
        });
        stats.d2h_bytes += 8.0;
        BFH_REQUIRE(p.first_malformed < 0, "mm: line " + std::to_string(header_lines_ + p.first_malformed + 1) + " is not 'row col value' (int int float)");
        return p.reparsed;
    }

    // step 3
    void split(const int64_t* sample_pos) {
        const size_t nt = static_cast<size_t>(num_train_), nv = static_cast<size_t>(std::max<int64_t>(1, num_vali_));
        grow(d_train_row_, nt); grow(d_train_col_, nt); grow(d_vals_row_, nt);
        grow(d_held_row_, nv); grow(d_held_col_, nv); grow(d_held_val_, nv); grow(d_vali_val_, nv); grow(d_sample_, nv);
        t_aux_.timed(stream, [&] {
            if (num_vali_ > 0)
                BFH_HIP(hipMemcpyAsync(d_sample_.get(), sample_pos, 8 * static_cast<size_t>(num_vali_), hipMemcpyHostToDevice, stream));
            hipLaunchKernelGGL(mm_split_kernel, dim3(blocks_of(header_nnz_)), dim3(256), 0, stream, d_r_.get(), d_c_.get(), d_v_.get(), header_nnz_,
                               d_sample_.get(), num_vali_, num_users_, num_items_, d_train_row_.get(), d_train_col_.get(), d_vals_row_.get(),
                               d_held_row_.get(), d_held_col_.get(), d_held_val_.get(), d_flags_.get() + kBad);
            BFH_HIP(hipGetLastError());
        });
    }

    // step 4, first half: {min, max} of the train values and of the held-out values
    void measure_values() {
        if (prepro_ != Prepro::kMinMaxScalar) return;
        const unsigned start[4] = {0xffffffffu, 0u, 0xffffffffu, 0u};
        t_aux_.timed(stream, [&] {
            BFH_HIP(hipMemcpyAsync(d_flags_.get() + kTrainRange, start, sizeof(start), hipMemcpyHostToDevice, stream));
            unsigned* range = reinterpret_cast<unsigned*>(d_flags_.get() + kTrainRange);
            hipLaunchKernelGGL(mm_minmax_kernel, dim3(std::min(blocks_of(num_train_), 2048u)), dim3(256), 0, stream, d_vals_row_.get(), num_train_, range);
            if (num_vali_ > 0)
                hipLaunchKernelGGL(mm_minmax_kernel, dim3(std::min(blocks_of(num_vali_), 2048u)), dim3(256), 0, stream, d_held_val_.get(), num_vali_, range + 2);
            BFH_HIP(hipGetLastError());
        });
    }

    // step 5, first half: the held-out triples in (row, col) order, a pair listed twice
    void sort_held() {
        const unsigned long long none = ~0ull;
        BFH_HIP(hipMemcpyAsync(d_flags_.get() + kDup, &none, sizeof(none), hipMemcpyHostToDevice, stream));
        const int64_t n = num_vali_;
        if (n == 0) return;
        const size_t sz = static_cast<size_t>(n);
        grow(d_keys_, sz); grow(d_keys_sorted_, sz); grow(d_pos_, sz); grow(d_pos_sorted_, sz);
        t_aux_.timed(stream, [&] {
            hipLaunchKernelGGL(csr_pack_kernel, dim3(blocks_of(n)), dim3(256), 0, stream, d_held_row_.get(), d_held_col_.get(), n, d_keys_.get(), d_pos_.get());
            BFH_HIP(hipGetLastError());
            device_sort_pairs_u64(d_keys_.get(), d_keys_sorted_.get(), d_pos_.get(), d_pos_sorted_.get(), n, 32 + bits_for(num_users_), d_tmp_, stream);
            hipLaunchKernelGGL(mm_dup_kernel, dim3(blocks_of(n)), dim3(256), 0, stream, d_keys_sorted_.get(), n, d_flags_.get() + kDup);
            BFH_HIP(hipGetLastError());
        });
    }

    // Third wait: ids outside the matrix, the value ranges, a repeated held-out pair
    void read_flags(const int64_t* sample_pos) {
        unsigned long long flags[kFlagWords];
        BFH_HIP(hipMemcpyAsync(flags, d_flags_.get(), sizeof(flags), hipMemcpyDeviceToHost, stream));
        BFH_HIP(hipStreamSynchronize(stream));
        stats.d2h_bytes += sizeof(flags);
        BFH_REQUIRE(flags[kBad] == 0, "mm: " + std::to_string(flags[kBad]) + " records with an id outside the matrix");
        if (flags[kDup] != ~0ull) {
            int64_t at[2] = {0, 0};
            BFH_HIP(hipMemcpy(at, d_pos_sorted_.get() + flags[kDup] - 1, sizeof(at), hipMemcpyDeviceToHost));
            const int64_t a = header_lines_ + sample_pos[at[0]] + 1, b = header_lines_ + sample_pos[at[1]] + 1;
            throw Error(BFH_ERR_INVALID, "mm: the held-out lines " + std::to_string(a) + " and " + std::to_string(b) +
                                             " list the same (row, col): scipy sums them into one entry and the reference cannot fill vali/val (base.py:250-253)");
        }
        if (prepro_ != Prepro::kMinMaxScalar) return;
        unsigned w[4];
        std::memcpy(w, flags + kTrainRange, sizeof(w));
        float f[4];
        for (int k = 0; k < 4; ++k) {
            const unsigned bits = mm_float_bits(w[k]);
            std::memcpy(&f[k], &bits, 4);
        }
        BFH_REQUIRE(std::isfinite(f[0]) && std::isfinite(f[1]) && (num_vali_ == 0 || (std::isfinite(f[2]) && std::isfinite(f[3]))),
                    "mm: a value that is not finite: MinMaxScalar has no range for it");
        // prepro.py:36-45: value_min starts at +inf, value_max at 0.0; every call widens them
        float lo = std::numeric_limits<float>::infinity(), hi = 0.f;
        lo = f[0] < lo ? f[0] : lo;
        hi = f[1] > hi ? f[1] : hi;
        range_[0] = lo; range_[1] = hi;
        if (num_vali_ > 0) {
            lo = f[2] < lo ? f[2] : lo;
            hi = f[3] > hi ? f[3] : hi;
        }
        range_[2] = lo; range_[3] = hi;
    }

    // MinMaxScalar.post of one group (prepro.py:47-58)
    void scale(const float* in, float* out, float lo, float hi) {
        const float width = hi - lo;   // binary32, as numpy subtracts two float32 scalars
        if (width < 0.00000001f) {     // ... and compares with the Python float
            hipLaunchKernelGGL(mm_fill_kernel, dim3(blocks_of(num_train_)), dim3(256), 0, stream, out, num_train_, static_cast<float>(opt_b_));
        } else {
            hipLaunchKernelGGL(mm_scale_kernel, dim3(blocks_of(num_train_)), dim3(256), 0, stream, in, num_train_, lo, width, static_cast<float>(opt_b_ - opt_a_),
                               static_cast<float>(opt_a_), out);
        }
        BFH_HIP(hipGetLastError());
    }

    // steps 4 and 5, second halves
    void transform_values() {
        built_prepro_ = prepro_;
        t_aux_.timed(stream, [&] {
            if (num_vali_ > 0) {
                hipLaunchKernelGGL(mm_vali_vals_kernel, dim3(blocks_of(num_vali_)), dim3(256), 0, stream, d_held_val_.get(), d_pos_sorted_.get(), num_vali_,
                                   vali_file_order_ ? 1 : 0, d_vali_val_.get());
                BFH_HIP(hipGetLastError());
            }
            switch (prepro_) {
            case Prepro::kNone:
                break;
            case Prepro::kOneBased:
                hipLaunchKernelGGL(mm_fill_kernel, dim3(blocks_of(num_train_)), dim3(256), 0, stream, d_vals_row_.get(), num_train_, 1.0f);
                if (num_vali_ > 0) hipLaunchKernelGGL(mm_fill_kernel, dim3(blocks_of(num_vali_)), dim3(256), 0, stream, d_vali_val_.get(), num_vali_, 1.0f);
                break;
            case Prepro::kImplicitALS:
                hipLaunchKernelGGL(mm_ials_kernel, dim3(blocks_of(num_train_)), dim3(256), 0, stream, d_vals_row_.get(), num_train_, static_cast<float>(opt_a_),
                                   d_vals_row_.get());
                if (num_vali_ > 0)
                    hipLaunchKernelGGL(mm_ials_kernel, dim3(blocks_of(num_vali_)), dim3(256), 0, stream, d_vali_val_.get(), num_vali_, static_cast<float>(opt_a_),
                                       d_vali_val_.get());
                break;
            case Prepro::kMinMaxScalar:   // the held-out values widen the range and stay as they are; the colwise group is scaled after them
                grow(d_vals_col_, static_cast<size_t>(num_train_));
                scale(d_vals_row_.get(), d_vals_col_.get(), range_[2], range_[3]);
                scale(d_vals_row_.get(), d_vals_row_.get(), range_[0], range_[1]);
                break;
            }
            BFH_HIP(hipGetLastError());
        });
    }

    Prepro prepro_ = Prepro::kNone, built_prepro_ = Prepro::kNone;   // as set / as the last build used it
    double opt_a_ = 0.0, opt_b_ = 0.0;
    bool vali_file_order_ = false;
    int num_users_ = 0, num_items_ = 0;
    int64_t header_nnz_ = 0, header_lines_ = 0, num_train_ = 0, num_vali_ = 0, n_ends_ = 0;
    float range_[4] = {0.f, 0.f, 0.f, 0.f};
    DevBuf<char> d_text_, d_tmp_;
    DevBuf<int64_t> d_tile_eol_, d_base_eol_, d_eol_, d_redo_, d_sample_, d_pos_, d_pos_sorted_;
    DevBuf<int32_t> d_r_, d_c_, d_train_row_, d_train_col_, d_held_row_, d_held_col_;
    DevBuf<float> d_v_, d_vals_row_, d_vals_col_, d_held_val_, d_vali_val_;
    DevBuf<unsigned long long> d_flags_;
    DevBuf<uint64_t> d_keys_, d_keys_sorted_;
    GroupFetch group_;
    EventTimer t_kernel_, t_aux_;
};

}  // namespace bfh

using bfh::guarded;
using bfh::MMHandle;

extern "C" {

BFH_ABI_LIFECYCLE(mm, MMHandle)

int bfh_mm_set_value_prepro(void* h, const char* name, double a, double b) {
    return guarded<MMHandle>(h, [&](MMHandle& m) { m.set_value_prepro(name, a, b); });
}
int bfh_mm_set_mode(void* h, const char* name, int64_t value) {
    return guarded<MMHandle>(h, [&](MMHandle& m) { m.set_mode(name, value); });
}
int bfh_mm_build(void* h, const char* text, int64_t bytes, const int64_t* sample_pos, int64_t n_sample, int64_t out_counts[6]) {
    return guarded<MMHandle>(h, [&](MMHandle& m) { m.build(text, bytes, sample_pos, n_sample, out_counts); });
}
int bfh_mm_fetch_group(void* h, int sort_key, int64_t* indptr, int32_t* keys, float* vals) {
    return guarded<MMHandle>(h, [&](MMHandle& m) { m.fetch_group(sort_key, indptr, keys, vals); });
}
int bfh_mm_fetch_vali(void* h, int32_t* rows, int32_t* cols, float* vals) {
    return guarded<MMHandle>(h, [&](MMHandle& m) { m.fetch_vali(rows, cols, vals); });
}
int bfh_mm_fetch_value_range(void* h, float out[4]) {
    return guarded<MMHandle>(h, [&](MMHandle& m) { m.fetch_value_range(out); });
}

}  // extern "C"
