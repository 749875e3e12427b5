"""What the eALS fold-in tests share: the rule of bfh_eals_fold_in restated in numpy (`fold`: np.float64 is the yardstick, np.float32 the
comparison run, every operation rounded and the sums taken entry by entry in eals.cc's order, eals.cc:199-233), the pattern CSR with a history
on either side of every class bound of csrc/eals_fold_kernels.hpp, and the envelope err(hip, f64) <= ref_eals.bound(err(float32 run, f64))."""
import functools
import os

import numpy as np

import helpers as H
from eals_cases import opt, record  # noqa: F401  (the tests take them from here)
from ref_eals import bound, relerr

EALS_FOLD_LDS, EALS_FOLD_BLOCK_MAX, EALS_HEAVY = 64 * 1024, 512, 4096      # csrc/eals_fold_kernels.hpp, csrc/eals_kernels.hpp
ITEMS = 6000
ALPHA, REG_U = float(np.float32(2.0)), float(np.float32(0.1))              # eals_cases.opt


def vdim_of(d):
    return (d + 31) // 32 * 32


def resident_max(vdim):
    """eals_fold_resident_max: the longest history that stays in LDS."""
    return min(EALS_FOLD_BLOCK_MAX, (EALS_FOLD_LDS // 4 - 5 * vdim - 8) // (vdim + 2))


def named_lengths(d):
    r = resident_max(vdim_of(d))
    return (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, r - 1, r, r + 1, EALS_HEAVY, EALS_HEAVY + 1)


def csr_of(lengths, seed):
    rng = np.random.default_rng(seed)
    keys = np.concatenate([np.sort(rng.choice(ITEMS, size=n, replace=False)) for n in lengths] + [np.zeros(0, np.int64)]).astype(np.int32)
    vals = (1 + rng.poisson(1.0, size=keys.shape[0])).astype(np.float32)
    return np.cumsum(lengths, dtype=np.int64), keys, vals


@functools.lru_cache(maxsize=None)
def pattern(d):
    """Histories of exactly named_lengths(d) entries, in that order, then a dozen of 1 .. 200 -> (indptr, keys, vals)."""
    rng = np.random.default_rng(11)
    return csr_of(list(named_lengths(d)) + [int(x) for x in rng.integers(1, 201, size=12)], 12)


@functools.lru_cache(maxsize=None)
def model(d, seed=0):
    """-> (P, Q, Cw) as eals_cases.problem makes them: normal(scale 0.3), Cw = 0.5 sqrt(pop) / sum over the pattern's keys; P: two unused rows."""
    rng = np.random.default_rng(seed)
    P = rng.normal(scale=0.3, size=(2, d)).astype(np.float32)
    Q = rng.normal(scale=0.3, size=(ITEMS, d)).astype(np.float32)
    pop = np.bincount(pattern(d)[1], minlength=ITEMS).astype(np.float64) ** 0.5
    return P, Q, (0.5 * pop / pop.sum()).astype(np.float32)


def rows_of(indptr):
    return list(zip(np.concatenate([[0], indptr[:-1]]).tolist(), indptr.tolist()))


def gram(Q, Cw, dt):
    CQ = np.sqrt(Cw.astype(dt))[:, None] * Q.astype(dt)
    return CQ.T @ CQ


def fold(Q, Cw, indptr, keys, vals, iters, init, dt, alpha=ALPHA, reg=REG_U):
    """The rule of bfh_eals_fold_in in `dt`, one history after the other -> [n, d] in dt."""
    seq = (lambda a: a.cumsum(dtype=dt)[-1] if a.size else dt(0)) if dt == np.float32 else (lambda a: a.sum())
    Q, C, S = Q.astype(dt), Cw.astype(dt), gram(Q, Cw, dt)
    alpha, reg = dt(alpha), dt(reg)
    D = Q.shape[1]
    out = np.zeros((indptr.shape[0], D), dt)
    for b, (beg, end) in enumerate(rows_of(indptr)):
        q, v = Q[keys[beg:end]], vals[beg:end].astype(dt)
        p = np.zeros(D, dt) if init is None else init[b].astype(dt)
        w = dt(1) + alpha * v
        m, wv = w - C[keys[beg:end]], w * v
        vhat = q @ p
        for _ in range(iters):
            for d in range(D):
                qd = q[:, d]
                f = vhat - p[d] * qd
                num = seq((wv - m * f) * qd) + (-seq(p * S[d]) + p[d] * S[d, d])
                den = seq(m * qd * qd) + (S[d, d] + reg)
                p[d] = num / den
                vhat = f + p[d] * qd
        out[b] = p
    return out


def solve(Q, Cw, keys, vals, alpha=ALPHA, reg=REG_U):
    """The fixed point of the rule for one history, float64: (S + sum_j m_j q q^T + reg I) p = sum_j w_j v_j q."""
    Q64, v = Q.astype(np.float64), vals.astype(np.float64)
    q, w = Q64[keys], 1.0 + alpha * v
    A = gram(Q, Cw, np.float64) + (q * (w - Cw.astype(np.float64)[keys])[:, None]).T @ q + reg * np.eye(Q.shape[1])
    return np.linalg.solve(A, q.T @ (w * v))


@functools.lru_cache(maxsize=None)
def references(d, with_init, iters=3):
    """The pattern's two runs, computed once per process -> (init or None, float32 run, float64 run)."""
    P, Q, Cw = model(d)
    ip, k, v = pattern(d)
    init = np.random.default_rng(5).normal(scale=0.3, size=(ip.shape[0], d)).astype(np.float32) if with_init else None
    return init, fold(Q, Cw, ip, k, v, iters, init, np.float32), fold(Q, Cw, ip, k, v, iters, init, np.float64)


def make_hip(d, P, Q, Cw, **kw):
    """A CyEALS with the model bound (no cache: fold_in needs none) -> (object, P, Q): the arrays it holds."""
    from buffalo_amd.backend import CyEALS
    g = CyEALS()
    path = H.write_opt(opt(d, **kw))
    assert g.init(path)
    os.unlink(path)
    P, Q = P.copy(), Q.copy()
    g.initialize_model(P, Q, Cw)
    return g, P, Q


def hold(section, X, cmp_run, f64, names=()):
    """Every row of the device run inside the envelope of the comparison run, over all rows and per named row; the figures go through `record`."""
    eo, eh = relerr(cmp_run, f64), relerr(X, f64)
    scale = np.abs(f64).max()
    per = [(n, np.abs(cmp_run[i] - f64[i]).max() / scale, np.abs(X[i] - f64[i]).max() / scale) for i, n in enumerate(names)]
    lines = ["err(float32 run, f64) %.3g err(hip, f64) %.3g ratio %.2f bound %.3g" % (eo, eh, eh / max(eo, 1e-30), bound(eo)),
             "  per row, entries: err(float32 run) / err(hip)  " + "  ".join("%d: %.2g / %.2g" % t for t in per)]
    record(section, lines)
    assert np.isfinite(X).all()
    assert eh <= bound(eo) and all(h <= bound(o) for _, o, h in per), "\n".join(lines)
