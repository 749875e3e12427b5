"""bfh_warp_fold_in: the float64 restatement of its rule (include/buffalo_hip.h) and the cases of test_warp_fold_in_cpu.py / _gpu.py.  u = 2^-24.

UNSAFE decision: a comparison ui - uj < threshold whose float64 margin lies within twice the float32 score error (d + 2) u sum |terms| (the
terms of both scores: |p_k q_k|, or (p_k - q_k)^2 under l2).  Every instance has none (SEEDS: the first model seed whose float64 run has none,
a search on the CPU), so which positives a pass accepts, with which negative and at which trial, does not depend on the float32 rounding: the
counts are integers to compare exactly, and the rows differ by rounding alone.

ERROR BOUND, tracked coordinate by coordinate beside the float64 run (`envelope`); E_x bounds |x32 - x64|, every magnitude is the float64 run's:
  grad    A accepted terms w (qi - qj) - reg p, each product, difference and sum rounded, summed in any order (at most A + log2(NGB) + 1 sums
          deep):  E_g = (A + 8) u S + A reg E_p,  S = sum over the accepted of |w (qi - qj)| + reg |p|
  / cnt   E_g / cnt + u |g|;     g2 = g - reg2 p:  E_g2 = E_g + reg2 E_p + 2 u (|g| + reg2 |p|)
  adagrad v' = v + g2^2: E_v' = E_v + 2 |g2| E_g2 + E_g2^2 + 3 u v';  adam (b1 = b2 = b): E_m' = b E_m + (1 - b) E_g2 + 3 u (|m'| + |g2|),
          E_v' = b E_v + (1 - b) (2 |g2| E_g2 + E_g2^2) + 4 u v', both divided by c = 1 - b^(t+1) (+ u)
  sqrt    |sqrt a - sqrt b| <= min(sqrt |a - b|, |a - b| / (2 sqrt(min(a, b)))):  E_s, + u s
  step    ge = n / (s + eps):  E_ge = min((E_n + |ge| E_s) / (s + eps - E_s) + 3 u |ge|, 2)   -- |ge| <= 1 in either run (adagrad: g2^2 <= v';
          adam with b1 = b2: Cauchy-Schwarz), so 2 bounds the difference where the denominator's error reaches the denominator
  x       x = p + lr ge: E_x = E_p + lr E_ge + u (|x| + lr |ge|)
  project r = sqrt(sum x^2): E_r by the sqrt rule from sum (2 |x| E_x + E_x^2) + (d + 2) u r^2;  p' = x / max(1, r):
          E_p' = (E_x + |p'| E_r) / max(1, r - E_r) + u |p'|
Nothing in it is fitted to a device's output; test_warp_fold_in_cpu.py holds the float32 restatement to it.

The LDS key bound (8192 keys, csrc/warp_fold_kernels.hpp) is a constant of the kernel, so the history one key past it has its own instances
(BIG: one per lane-group class, 16384 items, that history alone); every other instance has ITEMS = 1000."""
import functools
import itertools

import numpy as np

import ref_sgd as S

U24, ITEMS, ITERS, LR, REG_U, BETA1, RANDOM_SEED, MAX_TRIALS = 2.0 ** -24, 1000, 3, 0.005, 0.025, 0.9, 11, 10
KMAX, ATTEMPT_CAP, LDS_KEYS, BIG_ITEMS = (MAX_TRIALS + 1) // 2, 4096, 8192, 16384
INSTANCES = list(itertools.product((20, 64, 96, 128, 256), ("dot", "l2"), ("adagrad", "adam"), (0, 1)))   # d, score_func, optimizer, per_coordinate_normalize
BIG = [(20, "dot", "adagrad", 1), (65, "l2", "adam", 0), (129, "dot", "adam", 1)]                         # the same fields; G = 16, 32, 64
ALL = [i + (False,) for i in INSTANCES] + [i + (True,) for i in BIG]
# model seed per instance: the first whose float64 run has no unsafe decision and every outcome (test_warp_fold_in_cpu.py holds each to it)
SEEDS = dict(zip(ALL, [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0, 1, 0, 0, 1, 2, 2, 0, 2, 6, 29, 6, 32, 0, 2, 11]))
group_of = lambda d: 16 if d <= 64 else 32 if d <= 128 else 64   # lanes per positive (csrc/fold_group.hpp), on vdim = d rounded up to 32
OUTCOMES = ("accepted at the first trial", "accepted later", "exhausted", "found with trial >= max_trials")


@functools.lru_cache(maxsize=None)
def histories(G, big=False):
    """(indptr, keys, items): 0, 1, 2, NGB - 1, NGB, NGB + 1, 2 NGB + 1 keys; 950 of the 1000 items (seen draws chained past one window of G); 997
    (Phi = log(max(1, 2 / trial)) = 0, draws cut by the attempt cap); all 1000 (no candidate at all); 7 (the start row outside the unit ball)."""
    rng, NGB = np.random.default_rng(G), 256 // G
    sizes, items = ([LDS_KEYS + 1], BIG_ITEMS) if big else ([0, 1, 2, NGB - 1, NGB, NGB + 1, 2 * NGB + 1, 950, 997, 1000, 7], ITEMS)
    rows = [np.sort(rng.permutation(items)[:n]) for n in sizes]
    return np.cumsum([r.shape[0] for r in rows]).astype(np.int64), np.concatenate(rows).astype(np.int32), items


@functools.lru_cache(maxsize=None)
def candidates(G, big=False):
    """Per history [ITERS, n, KMAX]: the first KMAX draws of the rule that are none of the row's keys (-1: the attempt cap came first)."""
    indptr, keys, items = histories(G, big)
    out = []
    for b, end in enumerate(indptr):
        row = keys[(indptr[b - 1] if b else 0):end]
        n, seen = row.shape[0], np.isin(np.arange(items), row)
        cand, found = np.full((ITERS, n, KMAX), -1, np.int64), np.zeros((ITERS, n), np.int64)
        for t in range(ITERS):
            pending = np.arange(n)
            for attempt in range(ATTEMPT_CAP):
                if not pending.size:
                    break
                o0, _ = S._draw(RANDOM_SEED, 6, (b << 32) | pending, np.zeros(pending.size), t, np.full(pending.size, attempt))
                c = ((o0 * np.uint64(items)) >> np.uint64(32)).astype(np.int64)
                hit = pending[~seen[c]]
                cand[t, hit, found[t, hit]] = c[~seen[c]]
                found[t, hit] += 1
                pending = pending[found[t, pending] < KMAX]
        out.append(cand)
    return out


def model(d, score, seed, n_rows, items):
    """(Q, init, threshold): item rows of norm about 1; start rows of norm about 0.5, row 2 zero, the last of norm about 2.  The threshold sits in
    the lower tail of ui - uj (a few per cent of the candidates violate it), where few margins are small."""
    rng = np.random.default_rng(1000 + seed)
    Q = rng.normal(scale=1.0 / np.sqrt(d), size=(items, d)).astype(np.float32)
    init = rng.normal(scale=0.5 / np.sqrt(d), size=(n_rows, d)).astype(np.float32)
    if n_rows > 2:
        init[-1] *= 4
        init[2] = 0
    return Q, init, (-1.6 * 0.5 * np.sqrt(2.0 / d) if score == "dot" else -1.6 * 2.0 / np.sqrt(d))


def score_of(p, q, l2):
    """(scores, sum |terms|) of p against the rows q [..., d], in p's dtype."""
    terms = -(p - q) * (p - q) if l2 else p * q
    return terms.sum(axis=-1, dtype=p.dtype), np.abs(terms).sum(axis=-1, dtype=np.float64)


def envelope(E, p, g, A, Sg, cnt, mom, vel, opt, t):
    """One pass of the docstring's error bound: E = (E_p, E_m, E_v) before the pass -> after it; all arguments are the float64 run's, before the step."""
    Ep, Em, Ev = E
    f = lambda v: float(np.float32(v))   # noqa: E731
    reg, reg2, lr, b, eps, u = f(REG_U), f(2 * REG_U), f(LR), f(BETA1), 1e-10, U24
    Eg = (A + 8) * u * Sg + A * reg * Ep
    if cnt:
        Eg, g = Eg / cnt + u * np.abs(g) / cnt, g / cnt
    g2 = g - reg2 * p
    Eg2 = Eg + reg2 * Ep + 2 * u * (np.abs(g) + reg2 * np.abs(p))
    dv = 2 * np.abs(g2) * Eg2 + Eg2 ** 2
    if opt == "adam":
        c = f(1.0 - BETA1 ** (t + 1))
        m1, v1 = b * mom + f(1 - BETA1) * g2, b * vel + f(1 - BETA1) * g2 * g2
        Em, Ev = b * Em + f(1 - BETA1) * Eg2 + 3 * u * (np.abs(m1) + np.abs(g2)), b * Ev + f(1 - BETA1) * dv + 4 * u * v1
        num, En, rad, Erad = m1 / c, Em / c + u * np.abs(m1 / c), v1 / c, Ev / c + u * v1 / c
    else:
        v1 = vel + g2 * g2
        Ev = Ev + dv + 3 * u * v1
        num, En, rad, Erad = g2, Eg2, v1, Ev
    sqrt_err = lambda a, Ea: np.minimum(np.sqrt(Ea), Ea / (2 * np.sqrt(np.maximum(a - Ea, 1e-300)))) + u * np.sqrt(a)   # noqa: E731
    s, Es = np.sqrt(rad), sqrt_err(rad, Erad)
    ge = num / (s + eps)
    den = s + eps - Es
    Ege = np.where(den > 0, np.minimum((En + np.abs(ge) * Es) / np.where(den > 0, den, 1.0) + 3 * u * np.abs(ge), 2.0), 2.0)
    x = p + lr * ge
    Ex = Ep + lr * Ege + u * (np.abs(x) + lr * np.abs(ge))
    r2 = float((x * x).sum())
    r, Er = np.sqrt(r2), float(sqrt_err(r2, float((2 * np.abs(x) * Ex + Ex ** 2).sum()) + (p.shape[0] + 2) * u * r2))
    pn = x / max(1.0, r)
    return (Ex + np.abs(pn) * Er) / max(1.0, r - Er) + u * np.abs(pn), Em, Ev


def fold_ref(c, dtype=np.float64):
    """-> rows [n, d], counts [n, 2] (scored negatives, accepted positives), bound [n, d], unsafe decisions, the outcomes seen.  dtype=np.float32
    rounds every product and sum (the restatement of the device's arithmetic up to the order of its sums); the bound is tracked in float64 only."""
    T, (d, score, optimizer, pcn), l2 = dtype, c["inst"], c["inst"][1] == "l2"
    indptr, keys, items = c["indptr"], c["keys"], c["Q"].shape[0]
    Qd, reg, thr = c["Q"].astype(T), T(np.float32(REG_U)), c["threshold"]
    opt = dict(optimizer=optimizer, beta1=BETA1, lr=LR, use_bias=False)
    n_rows = indptr.shape[0]
    out, counts, bound, unsafe, seen_outcomes = np.zeros((n_rows, d), T), np.zeros((n_rows, 2), np.int64), np.zeros((n_rows, d)), 0, set()
    for b in range(n_rows):
        row = keys[(indptr[b - 1] if b else 0):indptr[b]]
        n, p = row.shape[0], c["init"][b].astype(T)
        mom, vel, E = np.zeros(d, T), np.zeros(d, T), (np.zeros(d), np.zeros(d), np.zeros(d))
        for t in range(ITERS if n else 0):
            cand = c["cand"][b][t]                                              # [n, KMAX]
            qi = Qd[row]
            ui, mag_i = score_of(p, qi, l2)
            uj, mag_j = score_of(p, Qd[np.maximum(cand, 0)], l2)
            diff = (ui[:, None] - uj).astype(T).astype(np.float64)              # double(ui - uj), the difference rounded in the scores' precision
            viol = (diff < thr) & (cand >= 0)
            found, first = viol.any(axis=1), viol.argmax(axis=1)
            scored = np.where(found, first + 1, (cand >= 0).sum(axis=1))        # candidates scored: k = 1 .. KMAX at the trials 2 k - 1 <= max_trials
            trial = 2 * (first + 1)
            acc = found & (trial < MAX_TRIALS)
            decided = np.arange(KMAX)[None, :] < scored[:, None]
            unsafe += int((decided & (np.abs(diff - thr) < 2 * (d + 2) * U24 * (mag_i[:, None] + mag_j))).sum())
            seen_outcomes |= {OUTCOMES[0]} if (acc & (first == 0)).any() else set()
            seen_outcomes |= {OUTCOMES[1]} if (acc & (first > 0)).any() else set()
            seen_outcomes |= {OUTCOMES[2]} if (~found & (scored == KMAX)).any() else set()
            seen_outcomes |= {OUTCOMES[3]} if (found & ~acc).any() else set()
            counts[b] += (int(scored.sum()), int(acc.sum()))
            phi = np.log(np.maximum(1, (items - n - 1) // trial[acc]).astype(np.float64)).astype(np.float32).astype(T)
            w = phi * T(2) if l2 else phi
            dq = qi[acc] - Qd[cand[acc, first[acc]]]
            terms = w[:, None] * dq - reg * p
            g, A = terms.sum(axis=0, dtype=T), int(acc.sum())
            if T is np.float64:
                Sg = (np.abs(w[:, None] * dq) + reg * np.abs(p)).sum(axis=0)
                E = envelope(E, p, g, A, Sg, A if pcn else 0, mom, vel, optimizer, t)
            X, _, m2, vel2 = S.optimizer_step(p[None], g[None], mom[None] if optimizer == "adam" else None, vel[None], np.array([A]) if pcn else None,
                                              REG_U, opt, t, project=True)
            p, vel, mom = X[0], vel2[0], (m2[0] if optimizer == "adam" else mom)
        out[b], bound[b] = p, E[0]
    return out, counts, bound, unsafe, seen_outcomes


@functools.lru_cache(maxsize=None)
def instance(d, score, optimizer, pcn, big=False):
    """One parity instance with its float64 result (computed once, shared, not to be written)."""
    inst, G = (d, score, optimizer, pcn), group_of(d)
    indptr, keys, items = histories(G, big)
    Q, init, thr = model(d, score, SEEDS[inst + (big,)], indptr.shape[0], items)
    c = dict(inst=inst, indptr=indptr, keys=keys, Q=Q, init=init, threshold=float(thr), cand=candidates(G, big))
    c["opt"] = dict(d=d, score_func=score, optimizer=optimizer, per_coordinate_normalize=bool(pcn), threshold=float(thr), max_trials=MAX_TRIALS,
                    reg_u=REG_U, beta1=BETA1, random_seed=RANDOM_SEED)
    c["f64"], c["counts"], c["bound"], c["unsafe"], c["outcomes"] = fold_ref(c)
    return c
