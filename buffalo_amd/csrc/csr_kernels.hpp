// The two kernels every COO -> compressed-rows path shares (ingest.hip, sppmi.hip, stream.hip, mm.hip): the packed (major, minor) sort key
// and the END offsets of a list whose major ids ascend.  Vector stores only.  The kernels are `static`: the header is
// included by several translation units, and each gets the copy it launches.
#pragma once
#include "common.hpp"

namespace bfh {

// keys[i] = major << 32 | minor: sorting the keys sorts the records by (major, minor).  pos[i] = i, the payload that carries the input
// order through a stable sort, is written when `pos` is not null.
static __global__ __launch_bounds__(256) void csr_pack_kernel(const int32_t* __restrict__ major, const int32_t* __restrict__ minor, int64_t n,
                                                       uint64_t* __restrict__ keys, int64_t* __restrict__ pos) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    keys[i] = (static_cast<uint64_t>(static_cast<uint32_t>(major[i])) << 32) | static_cast<uint32_t>(minor[i]);
    if (pos) pos[i] = i;
}

// The END-offset rule (no leading zero): entry i has major id m0, the next entry -- or the end of the list -- m1 >= m0, so every id in
// [m0, m1) ends behind entry i.  The ids in front of the first entry's are empty: entry 0 zeroes them.
__device__ __forceinline__ void csr_write_ends(int64_t i, int m0, int m1, int64_t* __restrict__ ends) {
    for (int m = m0; m < m1; ++m) ends[m] = i + 1;
    if (i == 0)
        for (int m = 0; m < m0; ++m) ends[m] = 0;
}

// major[0, n) ascending, n > 0: ends[m] = number of entries whose major id is <= m, for every m in [0, num_major)
static __global__ __launch_bounds__(256) void csr_ends_kernel(const int32_t* __restrict__ major, int64_t n, int num_major, int64_t* __restrict__ ends) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    csr_write_ends(i, major[i], i + 1 < n ? major[i + 1] : num_major, ends);
}

}  // namespace bfh
