// The library primitives of the host paths -- radix sorts, the exclusive scan, the run-length encode -- behind plain functions (declared in
// common.hpp).  rocPRIM is to these paths what rocBLAS would be to a plain GEMM; this is the only translation unit that includes it, so
// no other file pays for its headers.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_run_length_encode.hpp>
#include <rocprim/device/device_scan.hpp>

#include "common.hpp"

namespace bfh {

namespace {

// rocPRIM's calling convention: ask for the scratch size, grow `tmp` when it is smaller, run with all of `tmp`
template <typename Call>
void with_scratch(DevBuf<char>& tmp, Call&& call) {
    size_t bytes = 0;
    BFH_HIP(call(nullptr, bytes));
    if (tmp.size() < bytes) tmp.resize(bytes ? bytes : 1);
    bytes = tmp.size();
    BFH_HIP(call(tmp.get(), bytes));
}

template <typename K, typename V>
void sort_pairs(const K* keys_in, K* keys_out, const V* vals_in, V* vals_out, int64_t n, int bits, DevBuf<char>& tmp, hipStream_t s) {
    with_scratch(tmp, [&](void* t, size_t& b) {
        return rocprim::radix_sort_pairs(t, b, keys_in, keys_out, vals_in, vals_out, static_cast<size_t>(n), 0u, static_cast<unsigned>(bits), s);
    });
}

template <typename K>
void sort_keys(const K* keys_in, K* keys_out, int64_t n, int bits, DevBuf<char>& tmp, hipStream_t s) {
    with_scratch(tmp, [&](void* t, size_t& b) {
        return rocprim::radix_sort_keys(t, b, keys_in, keys_out, static_cast<size_t>(n), 0u, static_cast<unsigned>(bits), s);
    });
}

template <typename K>
void run_length_encode(const K* keys, int64_t n, K* uniq, unsigned int* counts, int64_t* d_runs, DevBuf<char>& tmp, hipStream_t s) {
    with_scratch(tmp, [&](void* t, size_t& b) { return rocprim::run_length_encode(t, b, keys, static_cast<size_t>(n), uniq, counts, d_runs, s); });
}

}  // namespace

void device_sort_pairs_u32(const uint32_t* keys_in, uint32_t* keys_out, const int32_t* vals_in, int32_t* vals_out, int64_t n, int bits, DevBuf<char>& tmp, hipStream_t s) {
    sort_pairs(keys_in, keys_out, vals_in, vals_out, n, bits, tmp, s);
}
void device_sort_pairs_u64(const uint64_t* keys_in, uint64_t* keys_out, const int64_t* vals_in, int64_t* vals_out, int64_t n, int bits, DevBuf<char>& tmp, hipStream_t s) {
    sort_pairs(keys_in, keys_out, vals_in, vals_out, n, bits, tmp, s);
}
void device_sort_pairs_u64_f32(const uint64_t* keys_in, uint64_t* keys_out, const float* vals_in, float* vals_out, int64_t n, int bits, DevBuf<char>& tmp, hipStream_t s) {
    sort_pairs(keys_in, keys_out, vals_in, vals_out, n, bits, tmp, s);
}

void device_sort_keys(const uint32_t* keys_in, uint32_t* keys_out, int64_t n, int bits, DevBuf<char>& tmp, hipStream_t s) {
    sort_keys(keys_in, keys_out, n, bits, tmp, s);
}
void device_sort_keys(const uint64_t* keys_in, uint64_t* keys_out, int64_t n, int bits, DevBuf<char>& tmp, hipStream_t s) {
    sort_keys(keys_in, keys_out, n, bits, tmp, s);
}

void exclusive_scan_i64(const int64_t* in, int64_t* out, int64_t n, DevBuf<char>& tmp, hipStream_t s) {
    with_scratch(tmp, [&](void* t, size_t& b) { return rocprim::exclusive_scan(t, b, in, out, int64_t(0), static_cast<size_t>(n), rocprim::plus<int64_t>(), s); });
}

void device_run_length_encode(const uint32_t* keys, int64_t n, uint32_t* uniq, unsigned int* counts, int64_t* d_runs, DevBuf<char>& tmp, hipStream_t s) {
    run_length_encode(keys, n, uniq, counts, d_runs, tmp, s);
}
void device_run_length_encode(const uint64_t* keys, int64_t n, uint64_t* uniq, unsigned int* counts, int64_t* d_runs, DevBuf<char>& tmp, hipStream_t s) {
    run_length_encode(keys, n, uniq, counts, d_runs, tmp, s);
}

}  // namespace bfh
