// numpy's pairwise float32 sum of a row of d elements on eight lanes -- the one summation order that the row normaliser
// (topk_normalize_kernel), the L2 ranking key (topk_half_sqnorm_kernel) and the squared distances (topk_sqdist_kernel, the L2 instance
// of eval_score_kernel) share, so that each of them has the bits of the reference's numpy line:
//   n < 8          one running sum, left to right;
//   8 <= n <= 128  r[i] = e[i], r[i] += e[8b + i] for every whole block of eight, ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the n % 8
//                  trailing elements one after the other;
//   n > 128        n2 = n / 2, n2 -= n2 % 8: sum(e[:n2]) + sum(e[n2:]), each half by the same rule.
// The element e[c] comes from a small functor, rounded to float32 BEFORE it is added (numpy materialises `x ** 2` as a float32 array):
//   SquareOf{a}        a[c]^2                 the normaliser's and the key's row norms, (feat ** 2).sum(-1)
//   SqDiffOf{a, b}     (a[c] - b[c])^2        distances, ((Q - p) ** 2).sum(-1): the difference is rounded, then its square
// Eight lanes per row: lane i holds r[i], the combine is the xor 1 / 2 / 4 butterfly (addition commutes, so every lane ends with the
// bits of numpy's expression); the short sums run on all eight lanes alike.  The eight lanes of a row must call together.
// `#pragma clang fp contract(off)`: the library is built with HIP's default contraction, which would fuse a square into the addition
// that follows it -- numpy rounds the square first.  __fmul_rn / __fadd_rn are plain operators in this toolchain and fuse all the
// same: the plain operators below, with contraction off, are the correctly rounded ones.  Sums run over d, never over the pitch ld:
// zero pad columns would change the blocks above.
#pragma once
#include "common.hpp"

namespace bfh {

constexpr int kPairwiseDepth = 24;   // halvings down to 128 columns of any d below 2^31

struct SquareOf {
    const float* a;
    __device__ __forceinline__ float operator()(int c) const {
#pragma clang fp contract(off)
        const float x = a[c];
        return x * x;
    }
};
struct SqDiffOf {
    const float *a, *b;
    __device__ __forceinline__ float operator()(int c) const {
#pragma clang fp contract(off)
        const float t = a[c] - b[c];
        return t * t;
    }
};

// the pairwise sum of e[lo .. lo + n), n <= 128 (i = this lane's place among the row's eight)
template <typename E>
__device__ __forceinline__ float pairwise_block_sum(const E& e, int lo, int n, int i) {
#pragma clang fp contract(off)
    float r = 0.f;
    int c = 0;
    if (n >= 8) {
        const int whole = n - (n & 7);
        r = e(lo + i);
        for (c = 8; c < whole; c += 8) {
            const float v = e(lo + c + i);
            r = r + v;
        }
        r = r + __shfl_xor(r, 1);
        r = r + __shfl_xor(r, 2);
        r = r + __shfl_xor(r, 4);
        c = whole;
    }
    for (; c < n; ++c) {
        const float v = e(lo + c);
        r = r + v;
    }
    return r;
}

// the pairwise sum of e[0 .. d), any d in [1, 2^31): every lane of the row returns it
template <typename E>
__device__ __forceinline__ float pairwise_row_sum(const E& e, int d, int i) {
#pragma clang fp contract(off)
    // the recursion as a loop: frame t = the right half still to be summed (hi_n[t] > 0) or the left half's sum waiting for it
    float left[kPairwiseDepth];
    int hi_lo[kPairwiseDepth], hi_n[kPairwiseDepth];
    int sp = 0, lo = 0, n = d;
    float s;
    for (;;) {
        while (n > 128) {
            int n2 = n / 2;
            n2 -= n2 % 8;
            hi_lo[sp] = lo + n2; hi_n[sp] = n - n2;
            ++sp;
            n = n2;
        }
        s = pairwise_block_sum(e, lo, n, i);
        while (sp > 0 && hi_n[sp - 1] == 0) s = left[--sp] + s;
        if (sp == 0) break;
        left[sp - 1] = s;
        lo = hi_lo[sp - 1]; n = hi_n[sp - 1];
        hi_n[sp - 1] = 0;
    }
    return s;
}

}  // namespace bfh
