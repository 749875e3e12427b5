// The factor row of the wave-per-row SGD kernels (BPRMF, WARP): K = ceil(vdim / 64) dwords per lane, lane holds element k*64+lane,
// so one instruction per k covers the row in full cache lines; the lanes beyond vdim hold 0 and neither store nor add.
#pragma once
#include "common.hpp"

namespace bfh {

template <int K>
struct Row {
    float v[K];
};

template <int K>
__device__ __forceinline__ void load_row(Row<K>& r, const float* __restrict__ base, int lane, int vdim) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int e = k * 64 + lane;
        r.v[k] = (e < vdim) ? base[e] : 0.0f;
    }
}
// same map, every dword loaded past the CU's L1 (global_load_dword sc1): what another CU of this
// XCD stored is in the L2, not in this CU's L1
template <int K>
__device__ __forceinline__ void load_row_coh(Row<K>& r, const float* base, int lane, int vdim) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int e = k * 64 + lane;
        r.v[k] = (e < vdim) ? __hip_atomic_load(base + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0f;
    }
}
template <int K>
__device__ __forceinline__ void store_row(const Row<K>& r, float* __restrict__ base, int lane, int vdim) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int e = k * 64 + lane;
        if (e < vdim) base[e] = r.v[k];
    }
}
template <int K>
__device__ __forceinline__ void atomic_add_row(const Row<K>& r, float* __restrict__ base, int lane, int vdim) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int e = k * 64 + lane;
        if (e < vdim) atomic_add_f32(base + e, r.v[k]);
    }
}

}  // namespace bfh
