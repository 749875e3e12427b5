// Kernels of the SPPMI builder (sppmi.hip): the pair lines of a stream as sort keys, appearances per item, the reference's double
// arithmetic with the six-digit text round trip of its output, the scatter of the kept pairs.  The END offsets of the result are
// csr_kernels.hpp's.  No atomics, vector stores only.
#pragma once
#include "common.hpp"
#include "csr_kernels.hpp"

namespace bfh {

// lines of a sequence of L events: sum_i min(windows, L - 1 - i), times two
__host__ __device__ __forceinline__ int64_t sppmi_pairs_of(int64_t L, int64_t w) {
    if (L <= 1) return 0;
    return L <= w + 1 ? L * (L - 1) / 2 : (L - w) * w + w * (w - 1) / 2;
}
// pairs written by the events before position i of a sequence of L events
__host__ __device__ __forceinline__ int64_t sppmi_pairs_before(int64_t i, int64_t L, int64_t w) {
    // event t writes min(w, L-1-t) pairs: w of them while t <= L-1-w
    const int64_t full = L - w > 0 ? (i < L - w ? i : L - w) : 0;   // events before i that write w pairs
    const int64_t rest = i - full;                                    // they write L-1-t = (L-1-full), (L-2-full), ...
    const int64_t first = L - 1 - full;
    return full * w + rest * first - rest * (rest - 1) / 2;
}

__global__ __launch_bounds__(256) void sppmi_count_kernel(const int64_t* __restrict__ indptr, int num_users, int windows, int64_t* __restrict__ pairs) {
    const int u = blockIdx.x * 256 + threadIdx.x;
    if (u >= num_users) return;
    const int64_t beg = u ? indptr[u - 1] : 0;
    pairs[u] = sppmi_pairs_of(indptr[u] - beg, windows);
}

// one thread per event: its pairs with the `windows` events after it, both orientations
// KeyT: uint32_t when num_items^2 fits 32 bits (half the bytes through the sort), else uint64_t
template <typename KeyT>
__global__ __launch_bounds__(256) void sppmi_lines_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ items, int num_users,
                                                          int64_t num_events, int windows, uint64_t num_items, const int64_t* __restrict__ pair_off,
                                                          KeyT* __restrict__ keys) {
    const int64_t e = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= num_events) return;
    const int u = static_cast<int>(lower_bound_dev<int64_t>(indptr, num_users, e + 1));   // first user whose END offset is > e
    const int64_t beg = u ? indptr[u - 1] : 0, L = indptr[u] - beg, i = e - beg;
    int64_t at = 2 * (pair_off[u] + sppmi_pairs_before(i, L, windows));
    const uint64_t w = static_cast<uint32_t>(items[e]);
    for (int64_t j = i + 1; j < i + windows + 1 && j < L; ++j) {
        const uint64_t c = static_cast<uint32_t>(items[beg + j]);
        keys[at++] = static_cast<KeyT>(w * num_items + c);
        keys[at++] = static_cast<KeyT>(c * num_items + w);
    }
}

template <typename KeyT>
__global__ __launch_bounds__(256) void sppmi_appear_kernel(const KeyT* __restrict__ sorted, int64_t n, int num_items, int64_t* __restrict__ app) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= num_items) return;
    const uint64_t ni = static_cast<uint64_t>(num_items);
    // (x + 1) * ni can be one past the key type's range for the last item: its run ends at n
    const int64_t end = x + 1 < num_items ? lower_bound_dev<KeyT>(sorted, n, static_cast<KeyT>((static_cast<uint64_t>(x) + 1) * ni)) : n;
    app[x] = end - lower_bound_dev<KeyT>(sorted, n, static_cast<KeyT>(static_cast<uint64_t>(x) * ni));
}

__host__ __device__ __forceinline__ double sppmi_pow10(int m) {   // exact for 0 <= m <= 22
    double p = 1.0;
    for (int i = 0; i < m; ++i) p *= 10.0;
    return p;
}
// float("%g" % x) for finite x > 0: round to six significant decimal digits, then to the nearest float
__host__ __device__ __forceinline__ float sppmi_text_round_trip(double x) {
    int e = 0;   // 10^e <= x < 10^(e+1)
    if (x >= 1.0) {
        while (e < 22 && x >= sppmi_pow10(e + 1)) ++e;
    } else {
        int m = 1;
        while (m < 22 && x * sppmi_pow10(m) < 1.0) ++m;
        e = -m;
    }
    int m5 = 5 - e;   // x * 10^m5 in [1e5, 1e6)
    double r = rint(m5 >= 0 ? x * sppmi_pow10(m5) : x / sppmi_pow10(-m5));
    if (r >= 1e6) { r = 1e5; m5 -= 1; }
    if (r < 1e5) { r *= 10.0; m5 += 1; }   // x sat a hair below the power of ten the search placed it above
    return static_cast<float>(m5 >= 0 ? r / sppmi_pow10(m5) : r * sppmi_pow10(-m5));
}

// one thread per distinct (a, b): value + number of output entries (0: sppmi <= 0, 2: a == b -- the reference writes that line twice)
template <typename KeyT>
__global__ __launch_bounds__(256) void sppmi_value_kernel(const KeyT* __restrict__ uniq, const unsigned int* __restrict__ cnt, int64_t runs,
                                                          uint64_t num_items, const int64_t* __restrict__ app, double log_d, double log_k,
                                                          float* __restrict__ val, int64_t* __restrict__ emit) {
    const int64_t r = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (r >= runs) return;
    const uint64_t key = static_cast<uint64_t>(uniq[r]);
    const uint64_t a = key / num_items, b = key % num_items;
    const uint64_t probe = a > b ? a : b, c = a > b ? b : a;   // fileio.hpp:207-208: the group of the larger id does the pair
    // fileio.hpp:182-250 writes a group when the next id's first line arrives and never flushes at end of file: the group of the
    // largest id that has lines (the first id of the last sorted key) is never a probe, so its pairs are not in the reference's output
    const uint64_t eof_group = static_cast<uint64_t>(uniq[runs - 1]) / num_items;
    const double pmi = log(static_cast<double>(cnt[r])) + log_d - log(static_cast<double>(app[probe])) - log(static_cast<double>(app[c]));
    const double sppmi = pmi - log_k;
    const bool keep = sppmi > 0 && probe != eof_group;
    val[r] = keep ? sppmi_text_round_trip(sppmi) : 0.f;
    emit[r] = keep ? (a == b ? 2 : 1) : 0;
}

template <typename KeyT>
__global__ __launch_bounds__(256) void sppmi_scatter_kernel(const KeyT* __restrict__ uniq, const float* __restrict__ val,
                                                            const int64_t* __restrict__ emit_off, int64_t runs, int64_t nnz, uint64_t num_items,
                                                            int32_t* __restrict__ out_row, int32_t* __restrict__ out_key, float* __restrict__ out_val) {
    const int64_t r = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (r >= runs) return;
    const int64_t at = emit_off[r], end = r + 1 < runs ? emit_off[r + 1] : nnz;
    const uint64_t key = static_cast<uint64_t>(uniq[r]);
    for (int64_t p = at; p < end; ++p) {
        out_row[p] = static_cast<int32_t>(key / num_items);
        out_key[p] = static_cast<int32_t>(key % num_items);
        out_val[p] = val[r];
    }
}

}  // namespace bfh
