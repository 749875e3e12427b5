// Kernels of the MatrixMarket database builder (mm.hip): the split of the parsed body lines into train and held-out triples, the value
// transforms of buffalo/data/prepro.py, the (row, col) order of the held-out values.  The line ends of the file are text_tiles.hpp's
// kernels, the pair keys csr_kernels.hpp's.  Integer atomics only, vector stores only.
#pragma once
#include "common.hpp"
#include "csr_kernels.hpp"
#include "text_tiles.hpp"

namespace bfh {

// float -> unsigned whose order is the order of the floats (-nan < -inf < ... < -0 < +0 < ... < +inf < +nan), and back
__host__ __device__ __forceinline__ unsigned mm_ordered_bits(unsigned bits) { return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u); }
__host__ __device__ __forceinline__ unsigned mm_float_bits(unsigned ordered) { return (ordered & 0x80000000u) ? (ordered & 0x7fffffffu) : ~ordered; }

#if defined(__HIPCC__)

// ---- step 2: body line t -> train slot or held slot, ids 0-based ----
// held[] = the n_held ascending body-line indices that are held out.  The held lines before line t are a binary search in it, so line t goes to
// train slot t - before or, when it is held[before] itself, to held slot before: both lists stay in file order without a flag array or a scan.
// Ids outside the matrix are counted (the lists still take them: nothing here indexes by an id).
__global__ __launch_bounds__(256) void mm_split_kernel(const int32_t* __restrict__ r, const int32_t* __restrict__ c, const float* __restrict__ v, int64_t n,
                                                       const int64_t* __restrict__ held, int64_t n_held, int num_users, int num_items,
                                                       int32_t* __restrict__ train_row, int32_t* __restrict__ train_col, float* __restrict__ train_val,
                                                       int32_t* __restrict__ held_row, int32_t* __restrict__ held_col, float* __restrict__ held_val,
                                                       unsigned long long* __restrict__ n_bad) {
    const int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (t >= n) return;
    const int row = r[t] - 1, col = c[t] - 1;
    if (row < 0 || row >= num_users || col < 0 || col >= num_items) atomicAdd(n_bad, 1ull);
    const int64_t before = n_held ? lower_bound_dev(held, n_held, t) : 0;
    if (before < n_held && held[before] == t) {
        held_row[before] = row; held_col[before] = col; held_val[before] = v[t];
    } else {
        train_row[t - before] = row; train_col[t - before] = col; train_val[t - before] = v[t];
    }
}

// ---- step 4: the value transforms ----
// range[0] = min, range[1] = max over v[0, n) as ordered bit patterns (mm_ordered_bits): exact and independent of the order of the atomics.
// A NaN or an infinity among the values ends up in one of the two words, which is how the host sees it.
__global__ __launch_bounds__(256) void mm_minmax_kernel(const float* __restrict__ v, int64_t n, unsigned* __restrict__ range) {
    unsigned lo = 0xffffffffu, hi = 0u;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * 256) {
        const unsigned o = mm_ordered_bits(__float_as_uint(v[i]));
        lo = o < lo ? o : lo;
        hi = o > hi ? o : hi;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned l2 = __shfl_down(lo, off, 64), h2 = __shfl_down(hi, off, 64);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMin(range, lo);
        atomicMax(range + 1, hi);
    }
}

// MinMaxScalar.post (prepro.py:52-58): ((v - vmin) / width) * span + lo, every operation rounded to binary32 on its own.  Plain operators under
// `fp contract(off)`: the __fmul_rn / __fadd_rn of the HIP headers are inline functions compiled with contraction allowed, and inlined here they
// fuse into one v_fma_f32 (seen in the ISA) whatever this scope says.
__global__ __launch_bounds__(256) void mm_scale_kernel(const float* __restrict__ in, int64_t n, float vmin, float width, float span, float lo,
                                                       float* __restrict__ out) {
#pragma clang fp contract(off)
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    const float a = in[i] - vmin;
    const float b = a / width;
    const float m = b * span;
    out[i] = m + lo;
}

// ImplicitALS.__call__ (prepro.py:69): q = v / eps and s = 1 + q in binary32, then the correctly rounded binary32 of log(s) through binary64
__global__ __launch_bounds__(256) void mm_ials_kernel(const float* __restrict__ in, int64_t n, float eps, float* __restrict__ out) {
#pragma clang fp contract(off)
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    const float q = in[i] / eps;
    const float s = 1.0f + q;
    out[i] = static_cast<float>(log(static_cast<double>(s)));
}

__global__ __launch_bounds__(256) void mm_fill_kernel(float* __restrict__ out, int64_t n, float value) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i < n) out[i] = value;
}

// ---- step 5: the held-out triples by (row, col); the keys and positions are csr_pack_kernel's ----
// keys sorted: first_dup = the smallest i whose key equals its left neighbour's
__global__ __launch_bounds__(256) void mm_dup_kernel(const uint64_t* __restrict__ keys, int64_t n, unsigned long long* __restrict__ first_dup) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i > 0 && i < n && keys[i] == keys[i - 1]) atomicMin(first_dup, static_cast<unsigned long long>(i));
}

// base.py:249-253: value k is the k-th in (row, col) order (order[k] = its place in the file order); with `file_order` it stays triple k's
__global__ __launch_bounds__(256) void mm_vali_vals_kernel(const float* __restrict__ held_val, const int64_t* __restrict__ order, int64_t n, int file_order,
                                                           float* __restrict__ out) {
    const int64_t k = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (k < n) out[k] = held_val[file_order ? k : order[k]];
}

#endif  // __HIPCC__

}  // namespace bfh
