// What the SGD fold-in kernels share (bpr_fold_kernels.hpp, warp_fold_kernels.hpp): the lane group that holds one row -- G lanes, lane l the
// columns 4 l .. 4 l + 3 -- its sum with a fixed tree, and the membership test in a history's sorted keys.
#pragma once
#include "common.hpp"

namespace bfh {

static inline int fold_group_of(int vdim) { return vdim <= 64 ? 16 : vdim <= 128 ? 32 : 64; }

// sum over the G lanes of a group, every lane receiving the same bits: within a row of 16 lanes  v += ror 8;  += ror 4;  += ror 2;  += ror 1
// (every lane adds the lane 8, 4, 2, 1 above it, cyclically); G = 32: + the other row of 16; G = 64: (row0 + row1) + (row2 + row3)
template <int G>
__device__ __forceinline__ float fold_group_sum(float v) {
    if constexpr (G == 64) return wave_sum(v);
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xf, 0xf, false));  // row_ror:8
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x124, 0xf, 0xf, false));  // row_ror:4
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x122, 0xf, 0xf, false));  // row_ror:2
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x121, 0xf, 0xf, false));  // row_ror:1
    if constexpr (G == 32) v += __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), 0x401F));   // lane ^ 16
    return v;
}

// is v one of the row's n ascending keys?  The same search over the LDS copy or over global memory.
__device__ __forceinline__ bool fold_contains(const int32_t* lds_keys, const int32_t* glb_keys, bool in_lds, int n, int32_t v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int32_t k = in_lds ? lds_keys[mid] : glb_keys[mid];
        if (k < v) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && (in_lds ? lds_keys[lo] : glb_keys[lo]) == v;
}

}  // namespace bfh
