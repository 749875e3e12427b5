// Kernels of the one-shot ingestion calls and of the device text parser (ingest.hip): newline positions of a working file, the "%d %d %f"
// line parser with its strtof fast paths, the orientation of the parsed ids, the scatter of the lines the host re-parsed, and the split of
// sorted pair keys into minor ids and END offsets.  Integer atomics only, vector stores only.
//
// The text parser: (1) newline positions by a count / scan / scatter over 4 KB tiles (one pass of counting, one of writing; the scan of
// the tile counts is the one library primitive; the pattern's pieces are in text_tiles.hpp, shared with stream.hip and mm.hip); (2) one
// thread per line parses the two integers and the decimal number.  sscanf's "%f" is
// strtof: the CORRECTLY ROUNDED binary32 of the decimal string.  The kernel reproduces it exactly where one rounding suffices -- Clinger's
// fast paths: <= 2^24 in the digits and 10^|e| <= 10^10 is one exact-operand float operation; <= 2^53 and |e| <= 22 is one exact-operand
// double operation whose result is then rounded to float, which equals strtof unless the double lands within one ulp of a float rounding
// boundary -- and FLAGS every line it cannot guarantee (such a near-tie, > 19 significant digits, exponents outside the fast paths,
// subnormal / overflowing results, "inf" / "nan" / hex floats, integers beyond int, malformed lines).  (3) Flagged lines -- none on
// ordinary rating files -- are re-parsed on the host with the reference's own sscanf call.  Result: bit-identical triples by construction.
#pragma once
#include "common.hpp"
#include "csr_kernels.hpp"
#include "text_tiles.hpp"

namespace bfh {

// keys sorted: out_minor[i] = low word; indptr[m] = i + 1 for every major id m in [major(i), major(i+1)) -- one pass over the keys for both
__global__ __launch_bounds__(256) void ingest_unpack_kernel(const uint64_t* __restrict__ keys, int64_t n, int num_major, int32_t* __restrict__ out_minor,
                                                            int64_t* __restrict__ indptr) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t k = keys[i];
    out_minor[i] = static_cast<int32_t>(k & 0xFFFFFFFFull);
    const int m0 = static_cast<int>(k >> 32);
    const int m1 = i + 1 < n ? static_cast<int>(keys[i + 1] >> 32) : num_major;
    csr_write_ends(i, m0, m1, indptr);
}

// ---- newline positions.  These two follow getline (fileio.hpp:297-300): a line ends at '\n' and nowhere else, so they stay apart from
// text_tiles.hpp's marks kernels, which follow Python's universal newlines ('\r', "\r\n") ----
__global__ __launch_bounds__(256) void text_count_newlines_kernel(const char* __restrict__ text, int64_t bytes, int64_t* __restrict__ tile_count) {
    __shared__ int s_cnt[4];
    const int64_t base = static_cast<int64_t>(blockIdx.x) * kTextTile + threadIdx.x * 16;
    int c = 0;
    if (base + 16 <= bytes) {
        const uint4 w = *reinterpret_cast<const uint4*>(text + base);
        const unsigned v[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) c += ((v[k] >> (8 * j)) & 0xffu) == 10u;
    } else {
        for (int64_t i = base; i < bytes && i < base + 16; ++i) c += text[i] == '\n';
    }
    const int total = tile_block_sum(c, s_cnt);
    if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
}

// nl[k] = byte offset of the k-th '\n' (tile_base[] = exclusive scan of the tile counts), written only for k < cap
__global__ __launch_bounds__(256) void text_write_newlines_kernel(const char* __restrict__ text, int64_t bytes, const int64_t* __restrict__ tile_base,
                                                                  int64_t cap, int64_t* __restrict__ nl) {
    __shared__ int s_scan[256];
    const int64_t base = static_cast<int64_t>(blockIdx.x) * kTextTile + threadIdx.x * 16;
    unsigned mask = 0;   // bit j: byte base + j is a newline
    for (int j = 0; j < 16; ++j)
        if (base + j < bytes && text[base + j] == '\n') mask |= 1u << j;
    tile_write_marks(mask, base, tile_base[blockIdx.x] + tile_block_exclusive(__popc(mask), s_scan), cap, nl);
}

__device__ __forceinline__ bool txt_space(char ch) { return ch == ' ' || ch == '\t' || ch == '\r' || ch == '\v' || ch == '\f'; }

// "%d": skip white space, optional sign, digits.  false: not representable here (no digits, beyond int) -> the host re-parses the line
__device__ __forceinline__ bool txt_int(const char* __restrict__ t, int64_t& i, int64_t end, int& out) {
    while (i < end && txt_space(t[i])) ++i;
    bool neg = false;
    if (i < end && (t[i] == '-' || t[i] == '+')) { neg = t[i] == '-'; ++i; }
    int64_t v = 0;
    int nd = 0;
    while (i < end && t[i] >= '0' && t[i] <= '9') {
        v = v * 10 + (t[i] - '0');
        ++nd; ++i;
        if (v > 4294967296ll) return false;
    }
    if (nd == 0) return false;
    v = neg ? -v : v;
    if (v > 2147483647ll || v < -2147483648ll) return false;
    out = static_cast<int>(v);
    return true;
}

// "%f" = strtof on [+-]digits[.digits][(e|E)[+-]digits]; false: not guaranteed bit-exact here (see the header comment)
__device__ __forceinline__ bool txt_float(const char* __restrict__ t, int64_t& i, int64_t end, float& out) {
    while (i < end && txt_space(t[i])) ++i;
    bool neg = false;
    if (i < end && (t[i] == '-' || t[i] == '+')) { neg = t[i] == '-'; ++i; }
    unsigned long long w = 0;
    int sig = 0, nd = 0, e10 = 0;
    bool dot = false;
    for (; i < end; ++i) {
        const char ch = t[i];
        if (ch == '.' && !dot) { dot = true; continue; }
        if (ch < '0' || ch > '9') break;
        ++nd;
        if (sig == 0 && ch == '0') { if (dot) --e10; continue; }   // leading zeros carry no significance
        if (sig >= 19) return false;                                // more digits than one exact integer holds
        w = w * 10 + static_cast<unsigned>(ch - '0');
        ++sig;
        if (dot) --e10;
    }
    if (nd == 0) return false;          // "inf", "nan", ".", garbage
    if (i < end && (t[i] == 'x' || t[i] == 'X')) return false;   // hex float ("0x1p3"): strtof reads on
    if (i < end && (t[i] == 'e' || t[i] == 'E')) {
        int64_t j = i + 1;
        bool eneg = false;
        if (j < end && (t[j] == '-' || t[j] == '+')) { eneg = t[j] == '-'; ++j; }
        int ev = 0, ed = 0;
        while (j < end && t[j] >= '0' && t[j] <= '9') {
            if (ev < 100000) ev = ev * 10 + (t[j] - '0');
            ++ed; ++j;
        }
        if (ed > 0) { e10 += eneg ? -ev : ev; i = j; }   // "1e" / "1e+" : the exponent part is not consumed
    }
    if (w == 0) { out = neg ? -0.0f : 0.0f; return true; }
    const int ae = e10 < 0 ? -e10 : e10;
    if (w <= (1ull << 24) && ae <= 10) {        // both operands exact in binary32: ONE correctly rounded operation
        const float p10[11] = {1e0f, 1e1f, 1e2f, 1e3f, 1e4f, 1e5f, 1e6f, 1e7f, 1e8f, 1e9f, 1e10f};
        const float f = static_cast<float>(static_cast<unsigned>(w));
        const float r = e10 < 0 ? __fdiv_rn(f, p10[ae]) : __fmul_rn(f, p10[ae]);
        out = neg ? -r : r;
        return true;
    }
    if (w <= (1ull << 53) && ae <= 22) {        // both exact in binary64: one correctly rounded double, then the rounding to float
        const double p10[23] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
        const double dw = static_cast<double>(w);
        const double d = e10 < 0 ? __ddiv_rn(dw, p10[ae]) : __dmul_rn(dw, p10[ae]);
        if (!(d >= 1.17549435e-38 && d <= 3.4028234e38)) return false;      // subnormal or overflowing binary32: strtof's own business
        const unsigned long long bits = static_cast<unsigned long long>(__double_as_longlong(d));
        const unsigned low = static_cast<unsigned>(bits & 0x1fffffffull);    // the 29 bits the rounding to float drops
        if (low >= 0x0ffffffeu && low <= 0x10000002u) return false;          // within two double ulps of a float rounding boundary: double rounding could differ
        const float r = static_cast<float>(d);
        out = neg ? -r : r;
        return true;
    }
    return false;
}

// The line list: ends[] = the n_ends line ends of the text in file order; line g begins behind ends[g - 1] (line 0 at byte 0) and ends at ends[g]
// (the last, unterminated one at `bytes`).  Thread k parses line first + k.
__global__ __launch_bounds__(256) void text_parse_kernel(const char* __restrict__ text, int64_t bytes, const int64_t* __restrict__ ends, int64_t n_ends,
                                                         int64_t first, int64_t lines, int32_t* __restrict__ r, int32_t* __restrict__ c, float* __restrict__ v,
                                                         int64_t* __restrict__ redo, int64_t redo_cap, unsigned long long* __restrict__ n_redo) {
    const int64_t k = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (k >= lines) return;
    const int64_t g = first + k;
    int64_t i = g == 0 ? 0 : ends[g - 1] + 1;
    const int64_t end = g < n_ends ? ends[g] : bytes;
    int rr = 0, cc = 0;
    float vv = 0.f;
    const bool ok = txt_int(text, i, end, rr) && txt_int(text, i, end, cc) && txt_float(text, i, end, vv);
    r[k] = rr; c[k] = cc; v[k] = vv;
    if (!ok) {
        const unsigned long long slot = atomicAdd(n_redo, 1ull);
        if (slot < static_cast<unsigned long long>(redo_cap)) redo[slot] = k;
    }
}

// 1-based (row, col) -> 0-based (major, minor) of the orientation `sort_key` names; out-of-range ids are counted
__global__ __launch_bounds__(256) void text_orient_kernel(const int32_t* __restrict__ r, const int32_t* __restrict__ c, int64_t n, int sort_key, int num_major,
                                                          int num_minor, int32_t* __restrict__ major, int32_t* __restrict__ minor,
                                                          unsigned long long* __restrict__ n_bad) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    const int a = (sort_key == 2 ? c[i] : r[i]) - 1, b = (sort_key == 2 ? r[i] : c[i]) - 1;
    major[i] = a;
    minor[i] = b;
    if (a < 0 || a >= num_major || b < 0 || b >= num_minor) atomicAdd(n_bad, 1ull);
}

// re-parsed lines back to their places: line idx[j] takes (hr, hc, hv)[j]
__global__ __launch_bounds__(256) void text_scatter_kernel(const int64_t* __restrict__ idx, const int32_t* __restrict__ hr, const int32_t* __restrict__ hc,
                                                           const float* __restrict__ hv, int64_t m, int64_t total_lines, int32_t* __restrict__ r,
                                                           int32_t* __restrict__ c, float* __restrict__ v) {
    const int64_t j = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (j >= m) return;
    const int64_t k = idx[j];
    if (k < 0 || k >= total_lines) return;
    r[k] = hr[j]; c[k] = hc[j]; v[k] = hv[j];
}

}  // namespace bfh
