// The count / scan / scatter pattern over 4 KB text tiles that ingest.hip (newlines of the working file), stream.hip (line ends and token
// starts of a stream file) and mm.hip (line ends of a MatrixMarket file) share: every 256-thread block owns one tile, every thread 16 bytes
// of it.  Pass 1 counts the marked bytes per tile, an exclusive scan of the tile counts (exclusive_scan_i64, common.hpp) says where each
// tile's marks go, pass 2 writes their byte offsets in file order.  The two kernels of the Stream and the MatrixMarket builder are here.
#pragma once
#include "common.hpp"

namespace bfh {

constexpr int kTextTile = 4096;   // bytes per 256-thread block: 16 per thread

static inline int64_t text_tiles_of(int64_t bytes) { return (bytes + kTextTile - 1) / kTextTile; }

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

// ---- the marks of Python's text rules (stream_marks16) over a padded text.  kTokens = false is the line-end half alone (a MatrixMarket
// file): no token is counted, scanned or written and the token pointers are null -- decided at compile time, so that the half that is off
// costs nothing ----
// pass 1: tile_eol[tile] = line ends of the tile, tile_tok[tile] = token starts of the tile
template <bool kTokens>
__global__ __launch_bounds__(256) void text_count_marks_kernel(const char* __restrict__ text, int64_t bytes, int64_t* __restrict__ tile_tok,
                                                               int64_t* __restrict__ tile_eol) {
    __shared__ int s_tok[kTokens ? 4 : 1], s_eol[4];
    unsigned tok, eol;
    stream_marks16(text, static_cast<int64_t>(blockIdx.x) * kTextTile + threadIdx.x * 16, bytes, tok, eol);
    const int nt = kTokens ? tile_block_sum(__popc(tok), s_tok) : 0, ne = tile_block_sum(__popc(eol), s_eol);
    if (threadIdx.x == 0) {
        if (kTokens) tile_tok[blockIdx.x] = nt;
        tile_eol[blockIdx.x] = ne;
    }
}

// pass 2: eol_pos[k] = offset of the k-th line end, k < n_eol; tok_pos[k] = offset of the k-th token start, k < n_tok, tok_line[k] = its
// line = the line ends before it, which the scan of the line ends already holds (neither is written when tok_pos is null: the id file of a
// stream has no tokens)
template <bool kTokens>
__global__ __launch_bounds__(256) void text_write_marks_kernel(const char* __restrict__ text, int64_t bytes, const int64_t* __restrict__ tok_base,
                                                               const int64_t* __restrict__ eol_base, int64_t n_tok, int64_t n_eol,
                                                               int64_t* __restrict__ tok_pos, int32_t* __restrict__ tok_line,
                                                               int64_t* __restrict__ eol_pos) {
    __shared__ int s_tok[kTokens ? 256 : 1], s_eol[256];
    const int64_t base = static_cast<int64_t>(blockIdx.x) * kTextTile + threadIdx.x * 16;
    unsigned tok, eol;
    stream_marks16(text, base, bytes, tok, eol);
    const int before_tok = kTokens ? tile_block_exclusive(__popc(tok), s_tok) : 0, before_eol = tile_block_exclusive(__popc(eol), s_eol);
    const int64_t eol_at = eol_base[blockIdx.x] + before_eol;
    tile_write_marks(eol, base, eol_at, n_eol, eol_pos);
    if (!kTokens || !tok_pos) return;
    int64_t k = tok_base[blockIdx.x] + before_tok;
    for (unsigned rest = tok; rest; rest &= rest - 1, ++k) {
        const int j = __ffs(rest) - 1;
        if (k >= n_tok) break;
        tok_pos[k] = base + j;
        tok_line[k] = static_cast<int32_t>(eol_at + __popc(eol & ((1u << j) - 1u)));
    }
}

#endif  // __HIPCC__

}  // namespace bfh
