"""bfh_bpr_fold_in: the float64 restatement of its rule (include/buffalo_hip.h) and the cases of test_bpr_fold_in_cpu.py / _gpu.py.  u = 2^-24.
UNSAFE step: the float64 score lies within twice the float32 dot error (d + 2) u (sum |p_k dq_k| + |Qb[pos]| + |Qb[neg]|), plus 24 u for the two
float32 roundings of (x + 6) * 83, of a cell edge or of +-6; where that sum is 0 the score is 0 in either precision and its cell exact.
With every cell equal an error of p does not grow (p' = p (1 - lr reg) + ...) and a step adds the roundings of dq, g dq, reg p, their difference, the
product with lr and the sum, u (5 lr |dq_k| + (1 + 3 lr reg) |p_k|): |p_k - p64_k| <= (5 S_b + 1) u M_bk, M_bk = max over the steps of |p_k| + lr_t |dq_k|."""
import functools

import numpy as np

import ref_numpy as R

U24, ITEMS, ITERS, LR, MIN_LR, REG_U, RANDOM_SEED, SUB = 2.0 ** -24, 1000, 3, 0.05, 0.01, 0.025, 11, 40
INSTANCES = [(d, b, nn, sp) for d in (20, 64, 96, 128, 256) for b in (0, 1) for nn in (1, 3) for sp in (0, 1)]   # sp: 0 uniform, 1 cumulative table
# model seed per instance: the first whose float64 run has no unsafe step (a search on the CPU; test_bpr_fold_in_cpu.py holds each to it)
SEEDS = dict(zip(INSTANCES, [1, 0, 0, 0, 1, 1, 1, 0, 2, 0, 2, 5, 0, 0, 3, 1, 1, 0, 0, 1, 1, 0, 10, 0, 3, 0, 1, 2, 2, 1, 4, 0, 4, 2, 36, 50, 0, 2, 78, 93]))
CUM = np.cumsum(np.where(np.arange(ITEMS) < SUB, 60, 1)).astype(np.int64)   # the cumulative table: most draws fall into the first SUB items


@functools.lru_cache(maxsize=None)
def histories(G):
    """(indptr, keys): 0, 1, 2 keys; 15 .. 17, 33, 65 around the window of G steps; 8 G + 1: past the LDS keys; 30 of the 40 favoured items: chained rejections; 2; 7."""
    rng = np.random.default_rng(G)
    rows = [np.sort(rng.permutation(ITEMS)[:n]) for n in (0, 1, 2, 15, 16, 17, 33, 65, 8 * G + 1, 2, 7)]
    rows.insert(9, np.sort(rng.permutation(SUB)[:30]))
    return np.cumsum([r.shape[0] for r in rows]).astype(np.int64), np.concatenate(rows).astype(np.int32)


def model(d, use_bias, seed):
    """(Q, Qb, init), scales like 1 / d (the dot error grows with d, a cell stays 1 / 83 wide); init: zero but for rows 0, 6 and, far out (many cells), 2."""
    rng = np.random.default_rng(1000 + seed)
    Q = rng.normal(scale=3.0 / d, size=(ITEMS, d)).astype(np.float32)
    Qb = (rng.normal(scale=1.0 / d, size=(ITEMS, 1)) if use_bias else np.zeros((ITEMS, 1))).astype(np.float32)
    rng = np.random.default_rng(500 + seed)
    init = np.zeros((12, d), np.float32)
    init[[0, 6]] = rng.normal(scale=2.0 / d, size=(2, d)).astype(np.float32)
    init[2] = rng.normal(scale=8.0 / np.sqrt(d), size=d).astype(np.float32)
    return Q, Qb, init


@functools.lru_cache(maxsize=None)
def triples(G, nn, sp):
    """Per history the (t, pos, neg) of every step in order: the rule's draws, row ids 0 .. 11, verify_neg on."""
    indptr, keys = histories(G)
    table, out = CUM if sp else None, []
    for b in range(indptr.shape[0]):
        row, steps = keys[(indptr[b - 1] if b else 0):indptr[b]].tolist(), []
        for t, (j, pos), s in ((t, jp, s) for t in range(ITERS) for jp in enumerate(row) for s in range(nn)):
            for a in range(1 << 20):
                o = R.counter_draw(RANDOM_SEED, 5, (b << 32) | j, s, t, a)
                neg = (o[0] * ITEMS) >> 32 if table is None else int(np.searchsorted(table, (((o[1] << 32) | o[0]) * int(table[-1])) >> 64, side="left"))
                if neg not in row:
                    break
            steps.append((t, pos, neg))
        out.append(steps)
    return out


def fold_ref(Q, Qb, steps, init, use_bias, dtype=np.float64):
    """-> (rows [n, d], M [n, d], unsafe steps); dtype=np.float32 rounds every product and sum (the dot: numpy's float32 dot)."""
    T, table, lr0, lr1 = dtype, R.exp_table(), float(np.float32(LR)), float(np.float32(MIN_LR))   # the ABI takes floats
    lrs = [np.float32(lr0 - (lr0 - lr1) * t / ITERS) for t in range(ITERS)]
    Qd, Qbd, reg, d = Q.astype(T), Qb.astype(T)[:, 0], T(np.float32(REG_U)), Q.shape[1]
    out, M, unsafe = np.zeros((len(steps), d), T), np.zeros((len(steps), d)), 0
    for b, row_steps in enumerate(steps):
        p, m = init[b].astype(T), np.abs(init[b]).astype(np.float64)
        for t, pos, neg in row_steps:
            lr, dq = T(lrs[t]), Qd[pos] - Qd[neg]
            x, mag = T(np.dot(p, dq)), float(np.abs(p * dq).sum())
            if use_bias:
                x = T(x + T(Qbd[pos] - Qbd[neg]))
                mag += abs(float(Qbd[pos])) + abs(float(Qbd[neg]))
            m = np.maximum(m, np.abs(p) + float(lr) * np.abs(dq))
            g = T(0) if 6 < x else T(1) if x < -6 else T(table[int(T(T(x + T(6)) * T(83)))])
            if mag > 0:
                cc = (float(x) + 6.0) * 83.0
                unsafe += min(abs(cc - round(cc)) / 83.0, abs(float(x) - 6.0), abs(float(x) + 6.0)) < 2 * (d + 2) * U24 * mag + 24 * U24
            p = p + lr * (g * dq - reg * p)
        out[b], M[b] = p, m
    return out, M, unsafe


@functools.lru_cache(maxsize=None)
def instance(d, use_bias, nn, sp):
    """One parity instance with its float64 result (computed once, shared, not to be written)."""
    G = 16 if d <= 64 else 32 if d <= 128 else 64                              # lanes per history (csrc/bpr_fold_kernels.hpp)
    indptr, keys = histories(G)
    Q, Qb, init = model(d, use_bias, SEEDS[(d, use_bias, nn, sp)])
    steps = triples(G, nn, sp)
    f64, M, unsafe = fold_ref(Q, Qb, steps, init, use_bias)
    opt = dict(d=d, use_bias=bool(use_bias), num_negative_samples=nn, sampling_power=float(sp), verify_neg=True, reg_u=REG_U, random_seed=RANDOM_SEED)
    return dict(opt=opt, indptr=indptr, keys=keys, Q=Q, Qb=Qb, init=init, steps=steps, f64=f64, unsafe=unsafe, table=CUM if sp else None,
                bound=(5.0 * ITERS * np.diff(indptr, prepend=0) * nn + 1.0)[:, None] * U24 * M)
