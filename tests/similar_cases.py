"""Shared fixtures of the most_similar tests: the pure-numpy restatement of the reference's `Algo._normalize` (algo/base.py:26-28) with
numpy's summation order written out, and the factor matrices the tests rank.

`feat / sqrt((feat ** 2).sum(-1) + 1e-8)` on a C-contiguous float32 matrix: the squares are float32 arrays, `sum(-1)` adds each row in
numpy's pairwise order (below), `+ 1e-8` adds float32(1e-8), and the square root and the division are the correctly rounded float32 ones.
Every step here is an elementwise float32 operation over the rows, so each is rounded exactly as the scalar operation would be."""
import functools

import numpy as np

EPS = np.float32(1e-8)
ROWS = 600
# the planted rows of `factors`
ZERO = 17                     # a zero row: Fn = 0
DUP_A, DUP_B = 100, 200       # F[100:140] = F[200:240]
MULT = 300                    # F[300:320] = c_i * F[300], c_i > 0
NEG, NEG_OF = 450, 451        # F[450] = -F[451]
PLANTED = [ZERO, NEG, NEG_OF] + list(range(DUP_A, DUP_A + 40, 7)) + list(range(DUP_B, DUP_B + 40, 7)) + list(range(MULT, MULT + 20, 3))
NORMALIZE_DS = (1, 7, 8, 9, 20, 100, 128, 129, 136, 200, 255, 256, 300)


def pairwise_sum(a):
    """Row sums of the float32 matrix a [rows, n] in the order of numpy's pairwise summation of a contiguous run of n floats."""
    assert a.dtype == np.float32 and a.ndim == 2
    n = a.shape[1]
    if n < 8:
        res = np.zeros(a.shape[0], np.float32)
        for c in range(n):
            res = res + a[:, c]
        return res
    if n <= 128:
        r = a[:, :8].copy()
        whole = n - n % 8
        for b in range(8, whole, 8):
            r = r + a[:, b:b + 8]
        res = ((r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])) + ((r[:, 4] + r[:, 5]) + (r[:, 6] + r[:, 7]))
        for c in range(whole, n):
            res = res + a[:, c]
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return pairwise_sum(a[:, :n2]) + pairwise_sum(a[:, n2:])


def sum_of_squares(F):
    sq = F * F
    assert sq.dtype == np.float32
    return pairwise_sum(sq)


def normalize(F):
    """Fn: what `Algo._normalize` makes of the float32 matrix F."""
    return F / np.sqrt(sum_of_squares(F) + EPS)[:, np.newaxis]


def raw_factors(rows, d, seed):
    """Float factors whose rows have the scales 1e-3, 1 and 30, mixed by row."""
    rng = np.random.default_rng(seed)
    F = rng.normal(size=(rows, d)).astype(np.float32)
    scale = np.array([1e-3, 1.0, 30.0], np.float32)[rng.integers(0, 3, size=rows)]
    return np.ascontiguousarray(F * scale[:, np.newaxis])


@functools.lru_cache(maxsize=None)
def factors(d):
    """The 600-row matrix the GPU tests rank (treat it as read-only), with the planted rows."""
    F = raw_factors(ROWS, d, 5000 + d)
    F[ZERO] = 0.0
    F[DUP_A:DUP_A + 40] = F[DUP_B:DUP_B + 40]
    rng = np.random.default_rng(d)
    c = rng.uniform(0.25, 40.0, size=20).astype(np.float32)
    c[0] = 1.0
    base = (30.0 * rng.normal(size=d)).astype(np.float32)          # large enough for the 1e-8 under the root to vanish: cosine 1 up to rounding
    F[MULT:MULT + 20] = c[:, np.newaxis] * base
    F[NEG] = -F[NEG_OF]
    F.setflags(write=False)
    return F


def golden_input(d):
    """The 40 rows per d whose reference outputs tests/golden/similar_vectors.npz stores (seed = 9000 + d), zero row included."""
    F = raw_factors(40, d, 9000 + d)
    F[3] = 0.0
    return F
