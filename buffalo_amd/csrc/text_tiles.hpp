// The count / scan / scatter pattern over 4 KB text tiles that ingest.hip (newlines of the working file), stream.hip (line ends and token
// starts of a stream file) and mm.hip (line ends of a MatrixMarket file) share: every 256-thread block owns one tile, every thread 16 bytes of it.  Pass 1 counts the marked bytes per tile,
// an exclusive scan of the tile counts says where each tile's marks go, pass 2 writes their byte offsets in file order.
#pragma once
#include <rocprim/device/device_scan.hpp>

#include "common.hpp"

namespace bfh {

constexpr int kTextTile = 4096;   // bytes per 256-thread block: 16 per thread

static inline int64_t text_tiles_of(int64_t bytes) { return (bytes + kTextTile - 1) / kTextTile; }

// out[i] = in[0] + ... + in[i - 1] over n int64 (rocprim::exclusive_scan: the one library primitive of the pattern); `tmp` grows as needed
static inline void exclusive_scan_i64(const int64_t* in, int64_t* out, int64_t n, DevBuf<char>& tmp, hipStream_t s) {
    size_t tb = 0;
    BFH_HIP(rocprim::exclusive_scan(nullptr, tb, in, out, int64_t(0), static_cast<size_t>(n), rocprim::plus<int64_t>(), s));
    if (tmp.size() < tb) tmp.resize(tb ? tb : 1);
    tb = tmp.size();
    BFH_HIP(rocprim::exclusive_scan(tmp.get(), tb, in, out, int64_t(0), static_cast<size_t>(n), rocprim::plus<int64_t>(), s));
}

// Python's text rules, shared by the Stream and the MatrixMarket builder (stream.hip, mm.hip).
// White space of str.strip() / str.split() among the bytes below 0x80: \t \n \v \f \r (9..13), \x1c..\x1f and the space (28..32).
// Bytes >= 0x80 are never white space here: Unicode-only separators (U+0085, U+00A0, U+2028, ...) stay inside their tokens.
__host__ __device__ __forceinline__ bool stream_space(unsigned b) { return (b - 9u) <= 4u || (b - 28u) <= 4u; }

#if defined(__HIPCC__)

// The 16 bytes at `base` (the buffer is padded to whole tiles, so the load is always inside it): bit j of `tok` = a token starts at
// base + j (a byte that is not white space after one that is, or after the start of the text), bit j of `eol` = a line ends there
// ('\n', or a '\r' the next byte of which is not '\n': Python's universal newlines).  Needs the byte before and the byte after the 16.
__device__ __forceinline__ void stream_marks16(const char* __restrict__ text, int64_t base, int64_t bytes, unsigned& tok, unsigned& eol) {
    tok = eol = 0;
    if (base >= bytes) return;
    const uint4 w = *reinterpret_cast<const uint4*>(text + base);
    const unsigned v[4] = {w.x, w.y, w.z, w.w};
    unsigned ws = 0, nl = 0, cr = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned b = (v[k] >> (8 * j)) & 0xffu, bit = 1u << (4 * k + j);
            ws |= stream_space(b) ? bit : 0u;
            nl |= b == 10u ? bit : 0u;
            cr |= b == 13u ? bit : 0u;
        }
    const int64_t left = bytes - base;
    const unsigned valid = left >= 16 ? 0xffffu : ((1u << left) - 1u);
    ws = (ws | ~valid) & 0xffffu;   // what lies behind the text separates like white space and ends no line
    nl &= valid;
    cr &= valid;
    const bool prev_ws = base == 0 || stream_space(static_cast<unsigned char>(text[base - 1]));
    const bool next_nl = base + 16 < bytes && text[base + 16] == '\n';
    tok = ~ws & ((ws << 1) | (prev_ws ? 1u : 0u)) & 0xffffu;
    eol = nl | (cr & ~((nl >> 1) | (next_nl ? 0x8000u : 0u)));
}

// sum of `c` over the 256 threads of the block, valid in thread 0 (s_cnt: 4 ints of LDS)
__device__ __forceinline__ int tile_block_sum(int c, int* s_cnt) {
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = c;
    __syncthreads();
    return s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// number of marks the threads before this one hold (Hillis-Steele scan over the block's 256 counts; s_scan: 256 ints of LDS)
__device__ __forceinline__ int tile_block_exclusive(int mine, int* s_scan) {
    s_scan[threadIdx.x] = mine;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const int v = threadIdx.x >= off ? s_scan[threadIdx.x - off] : 0;
        __syncthreads();
        s_scan[threadIdx.x] += v;
        __syncthreads();
    }
    return s_scan[threadIdx.x] - mine;
}

// the set bits of `mask` (bit j: byte base + j is marked) as offsets out[k], out[k + 1], ... while k < cap
__device__ __forceinline__ void tile_write_marks(unsigned mask, int64_t base, int64_t k, int64_t cap, int64_t* __restrict__ out) {
    while (mask) {
        const int j = __ffs(mask) - 1;
        mask &= mask - 1;
        if (k < cap) out[k] = base + j;
        ++k;
    }
}

#endif  // __HIPCC__

}  // namespace bfh
