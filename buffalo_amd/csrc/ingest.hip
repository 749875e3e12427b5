// COO -> compressed rows on the device and the device text parser -- host steps + C ABI; the kernels are in
// ingest_kernels.hpp and csr_kernels.hpp.
//
// Reference semantics: _sort_and_compressed_binarization (/root/reference/buffalo/data/fileio.hpp:263-420):
// the (row, col, val) records are STABLE-sorted by (major, minor) (`__gnu_parallel::stable_sort`, :328-339;
// duplicates keep their input order and are all kept), `indptr[k]` = number of records whose major id is
// <= k (END offsets, no leading zero, :359-379) and the minor ids / values are written out in sorted order
// (:389-410).  The reference runs it once per orientation (sort_key 1: rowwise, 2: colwise) on 1-based ids
// parsed from text; here the ids are 0-based arrays already in memory.
//
// Device formulation: one 64-bit key (major << 32 | minor) per record, a stable LSD radix sort over only the
// bits the two id ranges need (device_sort_pairs_u64_f32 -- the one library primitive on this path, like
// rocBLAS would be for a plain GEMM), then two trivially parallel passes: split the sorted keys
// back into minor ids and fill indptr from the positions where the major id changes.  All HBM-bound integer
// work: 2 x (8 + 4) B per record and radix pass.
//
// The working TEXT file of buffalo's data creation parsed on the device (fileio.hpp:263-330).
//
// Reference semantics: the file holds one "row col val" line per entry (1-based ids; buffalo/data/mm.py:175-234 copies the MatrixMarket
// body lines into it), every line is parsed with sscanf(line, "%d %d %f") (:300-303) -- up to 64 OpenMP threads over 4 MB splits whose
// boundary lines are stitched so that the net effect is "all lines in file order" -- and only the first `total_lines` are kept (:312-320).
//
// Device formulation: newline positions, one thread per line, the lines it cannot guarantee re-parsed on the host with the reference's own
// sscanf call and scattered back (parse_lines_on_device below); what the kernels guarantee is described in ingest_kernels.hpp.
#include <cstdio>
#include <cstring>
#include <thread>

#include "abi.hpp"
#include "ingest_kernels.hpp"

namespace bfh {

// the sort + compress of device arrays (major / minor / vals 0-based and validated): results into out_* (device), indptr (device)
void csr_from_device_coo(const int32_t* d_major, int32_t* d_minor /* overwritten with the sorted minors */, const float* d_vin, float* d_vout, int64_t nnz,
                         int num_major, int64_t* d_indptr, DevBuf<uint64_t>& d_kin, DevBuf<uint64_t>& d_kout, DevBuf<char>& d_tmp, hipStream_t stream) {
    d_kin.resize(nnz); d_kout.resize(nnz);
    hipLaunchKernelGGL(csr_pack_kernel, dim3(blocks_of(nnz)), dim3(256), 0, stream, d_major, d_minor, nnz, d_kin.get(), static_cast<int64_t*>(nullptr));
    BFH_HIP(hipGetLastError());
    // the minor word is sorted over the bits it uses, the gap above it is all zero
    device_sort_pairs_u64_f32(d_kin.get(), d_kout.get(), d_vin, d_vout, nnz, 32 + bits_for(num_major), d_tmp, stream);
    hipLaunchKernelGGL(ingest_unpack_kernel, dim3(blocks_of(nnz)), dim3(256), 0, stream, d_kout.get(), nnz, num_major, d_minor, d_indptr);
    BFH_HIP(hipGetLastError());
}

// ---------------------------------------------------------------- the parser over a line list ----------------------------------------------------------------
namespace {

// One parse_lines_on_device call: its arguments, and what the host's share of the lines needs
struct LineParse {
    const char *text, *d_text;
    int64_t bytes;
    const int64_t* d_ends;
    int64_t n_ends, first, lines;
    int32_t *d_r, *d_c;
    float* d_v;
    hipStream_t stream;
    std::vector<int64_t> ends, idx;   // the line ends the wanted lines touch; the lines the host parses again: line idx[j] reads (r, c, v)[j]
    std::vector<int32_t> r, c;
    std::vector<float> v;
    std::vector<char> whole;          // sscanf converted all three fields

    // step 1: one thread per line; returns the number of lines the kernel flagged (the first wait)
    unsigned long long launch(DevBuf<int64_t>& d_redo, int64_t redo_cap, unsigned long long* d_n_redo) {
        grow(d_redo, static_cast<size_t>(redo_cap));
        hipLaunchKernelGGL(text_parse_kernel, dim3(blocks_of(lines)), dim3(256), 0, stream, d_text, bytes, d_ends, n_ends, first, lines, d_r, d_c, d_v,
                           d_redo.get(), redo_cap, d_n_redo);
        BFH_HIP(hipGetLastError());
        unsigned long long n_redo = 0;
        BFH_HIP(hipMemcpyAsync(&n_redo, d_n_redo, sizeof(n_redo), hipMemcpyDeviceToHost, stream));
        BFH_HIP(hipStreamSynchronize(stream));
        return n_redo;
    }

    // step 2: the line ends, and the flagged lines -- or every line, when there are more of them than the list holds (a file in a format the
    // kernel does not speak)
    void fetch_flagged(const DevBuf<int64_t>& d_redo, unsigned long long n_redo, int64_t redo_cap) {
        ends.resize(static_cast<size_t>(std::min(n_ends, first + lines)));
        if (!ends.empty()) BFH_HIP(hipMemcpy(ends.data(), d_ends, ends.size() * 8, hipMemcpyDeviceToHost));
        if (n_redo <= static_cast<unsigned long long>(redo_cap)) {
            idx.resize(n_redo);
            BFH_HIP(hipMemcpy(idx.data(), d_redo.get(), n_redo * 8, hipMemcpyDeviceToHost));
        } else {
            idx.resize(static_cast<size_t>(lines));
            for (int64_t k = 0; k < lines; ++k) idx[k] = k;
        }
    }

    // step 3: the reference's own call, line by line (fileio.hpp:300-303).  Every line is independent: above a few thousand of them the work
    // is cut over up to 8 threads (a file of 17-digit reprs hands MOST of its lines back; one thread's sscanf is ~5 M lines per second)
    void reparse_on_host() {
        const size_t m = idx.size();
        const int64_t cap = static_cast<int64_t>(ends.size());
        r.resize(m); c.resize(m); v.resize(m); whole.resize(m);
        auto reparse = [&](size_t j0, size_t j1) {
            std::string line;
            for (size_t j = j0; j < j1; ++j) {
                const int64_t g = first + idx[j];
                const int64_t beg = g == 0 ? 0 : ends[g - 1] + 1, end = g < cap ? ends[g] : bytes;
                line.assign(text + beg, text + end);
                int rr = 0, cc = 0;
                float vv = 0.f;
                whole[j] = sscanf(line.c_str(), "%d %d %f", &rr, &cc, &vv) == 3;
                r[j] = rr; c[j] = cc; v[j] = vv;
            }
        };
        const unsigned hw = std::thread::hardware_concurrency();
        const size_t parts = std::max<size_t>(1, std::min<size_t>({8, hw ? hw : 1, m / 4096}));
        std::vector<std::thread> th;
        th.reserve(parts);
        size_t started_to = 0;
        try {
            for (size_t t = 0; parts > 1 && t < parts; ++t) {   // one part: no thread is started
                const size_t a = m * t / parts, b = m * (t + 1) / parts;
                th.emplace_back(reparse, a, b);
                started_to = b;
            }
        } catch (...) {   // a thread could not be started: the calling thread takes what is left
        }
        if (started_to < m) reparse(started_to, m);
        for (auto& x : th) x.join();
    }

    // step 4: the list and the re-parsed values go up ONCE and a small kernel puts every line where it belongs -- one blocking copy per line
    // would be millions of them for a file of 17-digit values, and the list's order is the order of the flagging atomics, not of the file.
    // Waits for the stream: the staging buffers die with this frame.
    void scatter_back() {
        const size_t m = idx.size();
        DevBuf<int64_t> d_idx;
        DevBuf<int32_t> s_r, s_c;
        DevBuf<float> s_v;
        d_idx.resize(m); s_r.resize(m); s_c.resize(m); s_v.resize(m);
        BFH_HIP(hipMemcpyAsync(d_idx.get(), idx.data(), m * 8, hipMemcpyHostToDevice, stream));
        BFH_HIP(hipMemcpyAsync(s_r.get(), r.data(), m * 4, hipMemcpyHostToDevice, stream));
        BFH_HIP(hipMemcpyAsync(s_c.get(), c.data(), m * 4, hipMemcpyHostToDevice, stream));
        BFH_HIP(hipMemcpyAsync(s_v.get(), v.data(), m * 4, hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(text_scatter_kernel, dim3(blocks_of(static_cast<int64_t>(m))), dim3(256), 0, stream, d_idx.get(), s_r.get(), s_c.get(), s_v.get(),
                           static_cast<int64_t>(m), lines, d_r, d_c, d_v);
        BFH_HIP(hipGetLastError());
        BFH_HIP(hipStreamSynchronize(stream));
    }
};

}  // namespace

// `lines` lines of a text that lies on the device (d_text) and on the host (text), from line `first` of the line list d_ends[n_ends] (see
// text_parse_kernel) on: (r, c, v)[k] = line first + k as sscanf(line, "%d %d %f") reads it.  *d_n_redo must be zero.  Waits for the stream.
ParsedLines parse_lines_on_device(const char* text, const char* d_text, int64_t bytes, const int64_t* d_ends, int64_t n_ends, int64_t first, int64_t lines,
                                  int32_t* d_r, int32_t* d_c, float* d_v, DevBuf<int64_t>& d_redo, unsigned long long* d_n_redo, hipStream_t stream) {
    ParsedLines out;
    LineParse p{text, d_text, bytes, d_ends, n_ends, first, lines, d_r, d_c, d_v, stream};
    const int64_t redo_cap = std::min<int64_t>(lines, int64_t(1) << 22);
    const unsigned long long n_redo = p.launch(d_redo, redo_cap, d_n_redo);
    if (n_redo == 0) return out;
    p.fetch_flagged(d_redo, n_redo, redo_cap);
    p.reparse_on_host();
    p.scatter_back();
    out.reparsed = static_cast<int64_t>(p.idx.size());
    for (size_t j = 0; j < p.idx.size(); ++j)
        if (!p.whole[j] && (out.first_malformed < 0 || p.idx[j] < out.first_malformed)) out.first_malformed = p.idx[j];
    return out;
}

// ---------------------------------------------------------------- the one-shot calls ----------------------------------------------------------------
// what a stateless call owns: a stream and a stopwatch on it
struct OneShot {
    hipStream_t stream = nullptr;
    EventTimer timer;
    OneShot() { BFH_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking)); }
    ~OneShot() {
        if (stream) (void)hipStreamDestroy(stream);
    }

    // a group on the device -> the caller's arrays; waits for the stream
    void download_group(const int64_t* d_indptr, const int32_t* d_minor, const float* d_vals, int64_t nnz, int num_major, int64_t* indptr, int32_t* out_minor,
                        float* out_vals) {
        BFH_HIP(hipMemcpyAsync(out_minor, d_minor, nnz * 4, hipMemcpyDeviceToHost, stream));
        BFH_HIP(hipMemcpyAsync(out_vals, d_vals, nnz * 4, hipMemcpyDeviceToHost, stream));
        BFH_HIP(hipMemcpyAsync(indptr, d_indptr, static_cast<size_t>(num_major) * 8, hipMemcpyDeviceToHost, stream));
        BFH_HIP(hipStreamSynchronize(stream));
    }
    // call when the stream is idle; kernel_ms = what the stopwatch saw
    void fill_stats(bfh_stats* stats, int64_t samples, int64_t reparsed, double h2d_bytes, double d2h_bytes) {
        const double ms = timer.drain();
        if (!stats) return;
        *stats = bfh_stats{};
        stats->samples = samples;
        stats->kernel_ms = ms;
        stats->merges = reparsed;   // lines re-parsed on the host with sscanf
        stats->h2d_bytes = h2d_bytes;
        stats->d2h_bytes = d2h_bytes;
    }
};

static void coo_to_csr(const int32_t* major, const int32_t* minor, const float* vals, int64_t nnz, int num_major, int num_minor, int64_t* indptr,
                       int32_t* out_minor, float* out_vals, bfh_stats* stats) {
    BFH_REQUIRE(nnz >= 0 && num_major > 0 && num_minor > 0, "coo_to_csr: empty shape");
    for (int64_t i = 0; i < nnz; ++i)
        if (major[i] < 0 || major[i] >= num_major || minor[i] < 0 || minor[i] >= num_minor)
            throw Error(BFH_ERR_INVALID, "coo_to_csr: id outside the matrix at record " + std::to_string(i));
    if (nnz == 0) {
        std::fill(indptr, indptr + num_major, int64_t(0));
        return;
    }
    OneShot g;
    DevBuf<int32_t> d_major, d_minor;
    DevBuf<float> d_vin, d_vout;
    DevBuf<uint64_t> d_kin, d_kout;
    DevBuf<int64_t> d_indptr;
    DevBuf<char> d_tmp;
    d_major.resize(nnz); d_minor.resize(nnz); d_vin.resize(nnz); d_vout.resize(nnz);
    d_indptr.resize(num_major);
    BFH_HIP(hipMemcpyAsync(d_major.get(), major, nnz * 4, hipMemcpyHostToDevice, g.stream));
    BFH_HIP(hipMemcpyAsync(d_minor.get(), minor, nnz * 4, hipMemcpyHostToDevice, g.stream));
    BFH_HIP(hipMemcpyAsync(d_vin.get(), vals, nnz * 4, hipMemcpyHostToDevice, g.stream));
    g.timer.timed(g.stream, [&] {
        csr_from_device_coo(d_major.get(), d_minor.get(), d_vin.get(), d_vout.get(), nnz, num_major, d_indptr.get(), d_kin, d_kout, d_tmp, g.stream);
    });
    g.download_group(d_indptr.get(), d_minor.get(), d_vout.get(), nnz, num_major, indptr, out_minor, out_vals);
    g.fill_stats(stats, nnz, 0, 12.0 * nnz, 8.0 * nnz + 8.0 * num_major);
}

// text -> (r, c, v) on the device (1-based ids as sscanf reads them), the first `total_lines` lines
struct TextTriples {
    DevBuf<char> text;
    DevBuf<int64_t> tile_cnt, tile_base, nl, redo;
    DevBuf<int32_t> r, c;
    DevBuf<float> v;
    DevBuf<unsigned long long> counters;   // [0] lines to re-parse, [1] ids outside the matrix
    DevBuf<char> tmp;
    int64_t reparsed = 0;                  // lines the host re-parsed
};

static void parse_text_on_device(const char* text, int64_t bytes, int64_t total_lines, TextTriples& T, hipStream_t stream) {
    BFH_REQUIRE(text && bytes > 0 && total_lines > 0, "text parse: empty input");
    T.text.resize(static_cast<size_t>(bytes) + 16);
    BFH_HIP(hipMemcpyAsync(T.text.get(), text, static_cast<size_t>(bytes), hipMemcpyHostToDevice, stream));
    const int64_t tiles = text_tiles_of(bytes);
    T.tile_cnt.resize(tiles + 1); T.tile_base.resize(tiles + 1);
    T.counters.resize(2, true, stream);
    BFH_HIP(hipMemsetAsync(T.tile_cnt.get() + tiles, 0, sizeof(int64_t), stream));
    hipLaunchKernelGGL(text_count_newlines_kernel, dim3(static_cast<unsigned>(tiles)), dim3(256), 0, stream, T.text.get(), bytes, T.tile_cnt.get());
    BFH_HIP(hipGetLastError());
    exclusive_scan_i64(T.tile_cnt.get(), T.tile_base.get(), tiles + 1, T.tmp, stream);
    int64_t n_nl = 0;
    BFH_HIP(hipMemcpyAsync(&n_nl, T.tile_base.get() + tiles, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
    BFH_HIP(hipStreamSynchronize(stream));
    const int64_t lines_in_file = n_nl + (text[bytes - 1] != '\n' ? 1 : 0);   // getline also returns an unterminated last line
    BFH_REQUIRE(lines_in_file >= total_lines, "text parse: the file holds " + std::to_string(lines_in_file) + " lines, total_lines says " +
                                                  std::to_string(total_lines) + " (fileio.hpp:322 asserts the same)");
    const int64_t cap = std::min(n_nl, total_lines);
    T.nl.resize(std::max<int64_t>(1, cap));
    hipLaunchKernelGGL(text_write_newlines_kernel, dim3(static_cast<unsigned>(tiles)), dim3(256), 0, stream, T.text.get(), bytes, T.tile_base.get(), cap, T.nl.get());
    BFH_HIP(hipGetLastError());
    T.r.resize(total_lines); T.c.resize(total_lines); T.v.resize(total_lines);
    T.reparsed = parse_lines_on_device(text, T.text.get(), bytes, T.nl.get(), cap, 0, total_lines, T.r.get(), T.c.get(), T.v.get(), T.redo, T.counters.get(), stream).reparsed;
}

static void parse_triples(const char* text, int64_t bytes, int64_t total_lines, int32_t* rows, int32_t* cols, float* vals, bfh_stats* stats) {
    OneShot g;
    TextTriples T;
    // upload of the text + newline index + parse (+ the host's share, if any line was flagged)
    g.timer.timed(g.stream, [&] { parse_text_on_device(text, bytes, total_lines, T, g.stream); });
    BFH_HIP(hipMemcpyAsync(rows, T.r.get(), total_lines * 4, hipMemcpyDeviceToHost, g.stream));
    BFH_HIP(hipMemcpyAsync(cols, T.c.get(), total_lines * 4, hipMemcpyDeviceToHost, g.stream));
    BFH_HIP(hipMemcpyAsync(vals, T.v.get(), total_lines * 4, hipMemcpyDeviceToHost, g.stream));
    BFH_HIP(hipStreamSynchronize(g.stream));
    g.fill_stats(stats, total_lines, T.reparsed, static_cast<double>(bytes), 12.0 * total_lines);
}

static void text_to_csr(const char* text, int64_t bytes, int64_t total_lines, int num_major, int num_minor, int sort_key, int64_t* indptr,
                        int32_t* out_minor, float* out_vals, bfh_stats* stats) {
    BFH_REQUIRE(sort_key == 1 || sort_key == 2, "text_to_csr: sort_key is 1 (rowwise) or 2 (colwise)");
    BFH_REQUIRE(num_major > 0 && num_minor > 0, "text_to_csr: empty shape");
    OneShot g;
    hipStream_t stream = g.stream;
    TextTriples T;
    const int64_t nnz = total_lines;
    DevBuf<int32_t> d_major, d_minor;
    DevBuf<float> d_vout;
    DevBuf<uint64_t> d_kin, d_kout;
    DevBuf<int64_t> d_indptr;
    g.timer.timed(stream, [&] {
        parse_text_on_device(text, bytes, total_lines, T, stream);
        d_major.resize(nnz); d_minor.resize(nnz); d_vout.resize(nnz); d_indptr.resize(num_major);
        hipLaunchKernelGGL(text_orient_kernel, dim3(blocks_of(nnz)), dim3(256), 0, stream, T.r.get(), T.c.get(), nnz, sort_key, num_major, num_minor,
                           d_major.get(), d_minor.get(), T.counters.get() + 1);
        BFH_HIP(hipGetLastError());
        unsigned long long bad = 0;
        BFH_HIP(hipMemcpyAsync(&bad, T.counters.get() + 1, sizeof(bad), hipMemcpyDeviceToHost, stream));
        BFH_HIP(hipStreamSynchronize(stream));
        BFH_REQUIRE(bad == 0, "text_to_csr: " + std::to_string(bad) + " records with an id outside the matrix");
        T.text.release();   // the bytes are not needed any more: room for the sort
        csr_from_device_coo(d_major.get(), d_minor.get(), T.v.get(), d_vout.get(), nnz, num_major, d_indptr.get(), d_kin, d_kout, T.tmp, stream);
    });
    g.download_group(d_indptr.get(), d_minor.get(), d_vout.get(), nnz, num_major, indptr, out_minor, out_vals);
    g.fill_stats(stats, nnz, T.reparsed, static_cast<double>(bytes), 8.0 * nnz + 8.0 * num_major);
}

}  // namespace bfh

// the stateless calls have no handle to keep a message: it goes where bfh_*_create's goes (bfh_last_error(NULL))
template <typename F>
static int stateless_call(F&& fn) {
    try {
        (void)bfh::current_device();
        fn();
        return BFH_OK;
    } catch (const bfh::Error& e) {
        bfh::g_create_error = e.what();
        return e.code;
    } catch (const std::exception& e) {
        bfh::g_create_error = e.what();
        return BFH_ERR_HIP;
    }
}

extern "C" {

int bfh_coo_to_csr(const int32_t* major, const int32_t* minor, const float* vals, int64_t nnz, int num_major, int num_minor, int64_t* indptr,
                   int32_t* out_minor, float* out_vals, bfh_stats* stats) {
    return stateless_call([&] { bfh::coo_to_csr(major, minor, vals, nnz, num_major, num_minor, indptr, out_minor, out_vals, stats); });
}

int bfh_parse_triples(const char* text, int64_t bytes, int64_t total_lines, int32_t* rows, int32_t* cols, float* vals, bfh_stats* stats) {
    return stateless_call([&] { bfh::parse_triples(text, bytes, total_lines, rows, cols, vals, stats); });
}

int bfh_text_to_csr(const char* text, int64_t bytes, int64_t total_lines, int num_major, int num_minor, int sort_key, int64_t* indptr,
                    int32_t* out_minor, float* out_vals, bfh_stats* stats) {
    return stateless_call([&] { bfh::text_to_csr(text, bytes, total_lines, num_major, num_minor, sort_key, indptr, out_minor, out_vals, stats); });
}

}  // extern "C"
