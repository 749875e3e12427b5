"""Shared fixtures of the L2 ("score_func" = 1) tests: the numpy restatements of what the library computes under L2, the yardsticks in
float64, the tolerance of the float cases and the inputs.

Restatements (float32, numpy's pairwise order written out in similar_cases.pairwise_sum):

* ``half_norms(Q)``    hb_j = -0.5f * s_j, s_j = the float32 bits of ``(Q ** 2).sum(-1)``: the per-column bias of the ranking key;
* ``sqdist32(Q, p)``   the float32 bits of ``((Q - p) ** 2).sum(-1)``: what ``out_scores`` reports, what ``WARP._get_most_similar_L2``
                       returns (warp.py:126,132) and, as ``1 - sqdist32``, what ``WARP._get_scores`` predicts (warp.py:147).

The tolerance of the float cases (u = 2^-24, first order in u).  The library ranks query p by key_j = fl(dot_j + hb_j), where

* dot_j is the matrix cores' float32 sum of the d products p_c q_jc.  Whatever the order of the additions, every product passes through
  at most one rounding of its own and d - 1 additions: |dot_j - p.q_j| <= d u sum_c |p_c q_jc| <= d u |p| |q_j| (Cauchy-Schwarz);
* hb_j = -s_j / 2 (halving is exact), s_j a float32 sum of the d rounded squares: by the same count |s_j - |q_j|^2| <= d u |q_j|^2, so
  |hb_j + |q_j|^2 / 2| <= (d / 2) u |q_j|^2;
* the final addition rounds once more: u |dot_j + hb_j| <= u (|p| |q_j| + |q_j|^2 / 2).

Together |key_j - (p.q_j - |q_j|^2 / 2)| <= u [(d + 1) |p| |q_j| + (d + 1) / 2 |q_j|^2] <= eps(p, q_j) with
eps(p, q) = u [(d + 1) |p| |q| + (d + 3) / 2 |q|^2]: the stated form keeps one u |q|^2 of slack over the count above for the terms of
second order.  The squared distance is |p|^2 - 2 key_exact, so a key that is off by eps moves an item's place as a distance that is
off by 2 eps would, and two items can change places only while their distances are within 4 eps of each other:
tau_b = 4 max_j eps(p_b, q_j).  Hence, with D_k the float64 k-th smallest admissible distance of row b: every listed item has
D <= D_k + tau_b (else the k items at or below D_k would all rank in front of it) and every unlisted admissible item has D >= D_k - tau_b;
two neighbours of a list, ordered by key, report distances that are inverted by no more than tau_b."""
import functools

import numpy as np

import similar_cases as sc

U24 = 2.0 ** -24
DS = (1, 7, 8, 9, 20, 127, 128, 129, 136, 200, 256, 300)
GOLDEN_NQ, GOLDEN_ROWS = 6, 40


# ---- the restatements ----
def half_norms(Q):
    """hb [rows] float32: -0.5 * the float32 pairwise sum of the float32-rounded squares of each row."""
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    hb = np.float32(-0.5) * sc.sum_of_squares(Q)
    assert hb.dtype == np.float32
    return hb


def sqdist32(Q, p):
    """Row-wise float32 squared distances of Q [rows, d] to p ([d], or [rows, d] for pairs): fl(fl(q - p)^2) summed in numpy's pairwise order."""
    t = np.ascontiguousarray(Q, dtype=np.float32) - np.asarray(p, dtype=np.float32)
    sq = t * t
    assert sq.dtype == np.float32 and sq.ndim == 2
    return sc.pairwise_sum(sq)


def predictions32(P, Q, rows, cols):
    """WARP._get_scores under L2 (warp.py:147) on float32 factors: fl(1.0f - sqdist32)."""
    return np.float32(1.0) - sqdist32(P[rows], Q[cols])


# ---- the float64 yardsticks ----
def dist64(P, Q):
    """D [nq, rows]: the squared distances in float64, one query at a time."""
    P64, Q64 = np.asarray(P, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    return np.stack([((Q64 - p) ** 2).sum(-1) for p in P64])


def lists64(D, adm, k):
    """keys [nq, k]: per row the min(k, admissible) admissible columns by (distance ascending, index descending), then -1."""
    out = np.full((D.shape[0], k), -1, dtype=np.int32)
    for b in range(D.shape[0]):
        cols = np.flatnonzero(adm[b])
        order = cols[np.lexsort((-cols, D[b, cols]))][:k]
        out[b, :len(order)] = order
    return out


def admissible(nq, rows, self_idx=None, pool=None, seen=None):
    """bool [nq, rows]: inside the pool, not the query's own row, not in the query's seen run."""
    adm = np.ones((nq, rows), dtype=bool)
    if pool is not None and len(pool):
        adm[:] = False
        adm[:, np.asarray(pool)] = True
    if self_idx is not None:
        adm[np.arange(nq), np.asarray(self_idx)] = False
    if seen is not None:
        for b, run in enumerate(seen):
            adm[b, np.asarray(run, dtype=np.int64)] = False
    return adm


def eps(P, Q):
    """eps(p_b, q_j) [nq, rows] of the module docstring."""
    d = P.shape[1]
    pn = np.linalg.norm(np.asarray(P, np.float64), axis=1)[:, None]
    qn = np.linalg.norm(np.asarray(Q, np.float64), axis=1)[None, :]
    return U24 * ((d + 1) * pn * qn + (d + 3) / 2.0 * qn * qn)


def tau(P, Q):
    """tau_b [nq] = 4 max_j eps(p_b, q_j)."""
    return 4.0 * eps(P, Q).max(axis=1)


def tau_rule(keys, D, adm, tau_b, scores=None):
    """The tau rule over lists keys [nq, k].  Returns (rows that break it, largest observed share of tau).  A row breaks it when its list is
    not min(k, admissible) distinct admissible columns followed by -1, when a listed item lies beyond D_k + tau, an unlisted admissible
    one inside D_k - tau, or (scores given) two neighbours' reported distances are inverted by more than tau."""
    bad, share = [], 0.0
    k = keys.shape[1]
    for b in range(keys.shape[0]):
        n_adm = int(adm[b].sum())
        kk = min(k, n_adm)
        row = keys[b]
        listed = row[:kk].astype(np.int64)
        ok = (row[kk:] == -1).all() and (listed >= 0).all()
        ok = ok and len(np.unique(listed)) == kk and bool(adm[b, listed].all())
        if ok and 0 < kk:
            Dk = np.sort(D[b, adm[b]])[kk - 1]
            worst = float(D[b, listed].max() - Dk)
            rest = adm[b].copy()
            rest[listed] = False
            if rest.any():
                worst = max(worst, float(Dk - D[b, rest].min()))
            if scores is not None and kk > 1:
                s = scores[b, :kk].astype(np.float64)
                worst = max(worst, float((s[:-1] - s[1:]).max()))
            share = max(share, worst / tau_b[b])
            ok = worst <= tau_b[b]
        if not ok:
            bad.append(b)
    return bad, share


# ---- inputs ----
def golden_input(d):
    """The factors whose reference outputs tests/golden/l2_vectors.npz stores: P [6, d], Q [40, d], rows / cols of 12 pairs (seed 9100 + d)."""
    rng = np.random.default_rng(9100 + d)
    P = rng.normal(scale=0.4, size=(GOLDEN_NQ, d)).astype(np.float32)
    Q = rng.normal(scale=0.4, size=(GOLDEN_ROWS, d)).astype(np.float32)
    rows = rng.integers(0, GOLDEN_NQ, size=12).astype(np.int32)
    cols = rng.integers(0, GOLDEN_ROWS, size=12).astype(np.int32)
    return P, Q, rows, cols


@functools.lru_cache(maxsize=None)
def grid_matrix(d, rows, nq, seed, tie=False):
    """F [rows, d] with coordinates k / 8, |k| <= 8, drawn row by row and kept only while, for each of the first nq rows (the queries), the
    squared distances to all rows -- its own, 0, included -- stay distinct.  Dots, norms, keys and distances of such rows are multiples of
    1 / 128 far below 2^24 / 128: exact in float32 in any order.  `tie`: the last row is a copy of row nq (one planted tie per query)."""
    rng = np.random.default_rng(seed)
    F = np.zeros((rows, d), dtype=np.int64)
    taken = np.zeros((nq, 256 * d + 1), dtype=bool)      # taken[i, 64 * D]: query i has a kept row (itself: 0) at squared distance D
    n = 0
    for _ in range(400 * rows):
        if n == rows:
            break
        cand = rng.integers(-8, 9, size=d)
        m = min(n, nq)                                   # queries among the kept rows
        to_queries = ((F[:m] - cand) ** 2).sum(-1)
        if taken[np.arange(m), to_queries].any():
            continue
        if n < nq:                                       # a new query: its own distances to the kept rows must be distinct and not 0
            own = ((F[:n] - cand) ** 2).sum(-1)
            if len(np.unique(own)) != n or (own == 0).any():
                continue
            taken[n, own] = True
            taken[n, 0] = True
        taken[np.arange(m), to_queries] = True
        F[n] = cand
        n += 1
    assert n == rows, "grid_matrix(%d, %d, %d): too few distinct distances" % (d, rows, nq)
    if tie:
        F[rows - 1] = F[nq]
    F = np.ascontiguousarray(F.astype(np.float32) / np.float32(8.0))
    F.setflags(write=False)
    return F


@functools.lru_cache(maxsize=None)
def float_case(d, nq, rows, seed, near=4):
    """(P [nq, d], Q [rows, d]) inside the unit ball, as WARP projects its rows; the last near * min(nq, 8) rows of Q are near-duplicates of
    the first queries: q = p + r * unit vector, r = 1e-3 (1 + i / 100)."""
    rng = np.random.default_rng(seed)

    def ball(n, rmax):
        X = rng.normal(size=(n, d))
        X /= np.linalg.norm(X, axis=1, keepdims=True)
        return X * rng.uniform(0.15, rmax, size=(n, 1))
    P, Q = ball(nq, 0.99), ball(rows, 1.0)
    dup = min(near * min(nq, 8), rows // 2)
    for i in range(dup):
        e = rng.normal(size=d)
        Q[rows - dup + i] = P[i % min(nq, 8)] + 1e-3 * (1 + i / 100.0) * e / np.linalg.norm(e)
    P, Q = np.ascontiguousarray(P, dtype=np.float32), np.ascontiguousarray(Q, dtype=np.float32)
    P.setflags(write=False)
    Q.setflags(write=False)
    return P, Q


# ---- the validation restatement (evaluate/base.py:44-148 over L2 lists) ----
def seen_runs(train, rows):
    import eval_cases as ec
    return [ec.seen_of(train, int(u)) for u in rows]


def score_metrics(P, Q, vali):
    """(rmse, error) of evaluate/base.py:130-148 from the restated float32 predictions, the errors summed in float64."""
    err = (predictions32(P, Q, vali["row"], vali["col"]) - vali["val"]).astype(np.float64)
    assert len(err)
    return float(np.sqrt((err * err).sum() / len(err))), float(np.abs(err).sum() / len(err))
