"""Float64 run of one epoch of gradient accumulation and of the epoch-end optimizer step of the SGD base (adam / adagrad BPRMF
and WARP) -- the yardstick of the stage tests, what ref_eals.py is for eALS.  Written from the reference lines the device code
cites (lib/algo_impl/bpr/bpr.cc:119-181, lib/algo_impl/warp/warp.cc:128-170, lib/algo.cc:365-465, warp.cc:192-201), vectorised over
the triples of an epoch; the sigmoid table, the table lookup and the counter sampler are ref_numpy's, not restated.

`dtype=np.float64` is the yardstick: no float32 between the float32 state it is handed and the arrays it returns.  `dtype=
np.float32` is a restatement of the reference's arithmetic (every product and sum rounded to float32, a gradient row summed
triple by triple in the reference's order); tests/test_sgd_ref_cpu.py holds it to the C++ oracle.  The constants the reference
rounds to float32 before it uses them (lr, 2 reg, beta, 1 - beta^t, FEPS) are those float32 values in both runs: they are the
specification, not the arithmetic under test.

A stage of a backend is held to the oracle's own distance from the float64 run, row by row:
  gradient row r:   err[r] = max_k |X[r,k] - X64[r,k]| / S[r] <= stage_bound = ref_eals.bound(the oracle's worst row), plus order_term(n_r)
                    where every term is its own atomic add (accum_two_pass = 0, update_triples),
                    S[r] = max_k (|start[r,k]| + sum over the n_r terms row r received of |term[k]|): the scale a summation error of
                    that row has.  A row that received no term keeps its start bits.
  optimizer output: elementwise, relative to |f64|, <= ref_eals.bound(the worst element of the envelope run).
Which triples an epoch has, and which table cell a score takes, must not depend on float32 rounding, or no bound on a sum would
follow: `unsafe` counts the triples whose float64 score lies within the float32 dot error of a decision edge, and every committed
case has `unsafe == 0` (sgd_cases.SEEDS; searched on the CPU, where `unsafe_2x` -- the same count at twice the distance -- is 0 too:
the device's state at the second epoch differs from the restatement's, and from run to run, in its last bits).

`defect=` (float32 run) plants one mistake a device kernel could make; tests/test_sgd_ref_cpu.py shows that each one leaves the
stage bound, and that some of them do NOT move the trained model by 1e-4 (adagrad / adam divide a gradient by its own magnitude).
"""
import numpy as np

import ref_numpy as rn
from ref_eals import ULP32, bound, relerr  # noqa: F401  (bound / relerr: re-exported for the stage tests)

DEFECTS = (
    "drop_incidence_at_chunk_end",          # index GATHER_CHUNK - 1 of the item-sorted positive list is lost
    "second_flush_overwrites",              # a run cut by a chunk boundary keeps only its last part
    "count_pos_per_slot",                   # the per-positive counts (Q-9) taken once per negative slot
    "count_skips_unupdated_list",           # update_i / update_j = False stops the COUNT of that list too
    "bias_not_divided_without_use_bias",    # gradQb / count only under use_bias
    "grad_rezeroed",                        # the epoch starts from zero instead of from the step left in grad (Q-6)
    "feps_inside_sqrt",                     # sqrt(v + FEPS) for sqrt(v) + FEPS (Q-5)
    "beta2_from_beta2",                     # the option "beta2" is honoured (the reference reads "beta1" twice)
    "zero_count_divides",                   # a count of 0 divides
    "project_before_step",                  # WARP's projection ahead of the step
    "last_row_of_wave_skipped",             # the optimizer leaves the last row of a partly filled wave
    "phi_trial_off_by_one",                 # Phi from trial - 1
    "phi_zero_rejected",                    # a positive with Phi = 0 is not counted
    "row_term_once_per_run",                # (a sum c + b n) q of the gather taken with n = 1
    "gradq_row_scale",                      # gradQ[r] *= 1 + 0.3 sin(r)
)
U24 = 2.0 ** -24
FEPS = np.float32(1e-10)
STATE_NAMES = ("P", "Q", "Qb", "gradP", "gradQ", "gradQb", "momP", "momQ", "momQb", "velP", "velQ", "velQb")


class State:
    """The model and the optimizer state, [rows, d] (no padding columns) and [rows] for the bias column, in one dtype."""

    def __init__(self, P, Q, Qb, dtype=np.float64, iters=0, **rest):
        self.dtype, self.iters = dtype, int(iters)
        self.P, self.Q, self.Qb = np.array(P, dtype), np.array(Q, dtype), np.array(Qb, dtype).reshape(-1)
        for n in STATE_NAMES[3:]:
            like = self.P if n.endswith("P") else self.Qb if n.endswith("Qb") else self.Q
            setattr(self, n, np.array(rest[n], dtype).reshape(like.shape) if n in rest else np.zeros_like(like))

    def copy(self, dtype=None):
        return State(self.P, self.Q, self.Qb, dtype or self.dtype, self.iters, **{n: getattr(self, n) for n in STATE_NAMES[3:]})


# ---------------------------------------------------------------------------------------------
# the counter sampler (ref_numpy.counter_draw on arrays) and the triples of an epoch
# ---------------------------------------------------------------------------------------------
def _draw(seed, stream, pos_idx, slot, epoch, attempt):
    u64 = np.uint64
    o = rn.counter_draw(int(seed), int(stream), np.asarray(pos_idx).astype(u64), np.asarray(slot).astype(u64), int(epoch),
                        np.asarray(attempt).astype(u64))
    return o[0].astype(u64), o[1].astype(u64)


def _seen_matrix(csr):
    seen = np.zeros((csr.num_users, csr.num_items), bool)
    seen[csr.rows(), csr.keys] = True
    return seen


def bpr_triples(csr, opt, epoch, cum):
    """bpr.cc:104-118 with the counter sampler: (u, pos, neg) of triple  position * num_negative_samples + slot."""
    nn, I = int(opt["num_negative_samples"]), csr.num_items
    rows, seen = csr.rows().astype(np.int64), _seen_matrix(csr)
    pos_idx, slot = np.repeat(np.arange(csr.nnz), nn), np.tile(np.arange(nn), csr.nnz)
    u, pos = rows[pos_idx], csr.keys.astype(np.int64)[pos_idx]
    neg = np.full(u.shape[0], -1, np.int64)
    uniform = float(opt.get("sampling_power", 0.0)) == 0.0
    total = int(cum[-1]) if not uniform else 0
    pending, attempt = np.arange(u.shape[0]), 0
    while pending.size:
        o0, o1 = _draw(opt["random_seed"], 0, pos_idx[pending], slot[pending], epoch, np.full(pending.size, attempt))
        if uniform:
            cand = ((o0 * np.uint64(I)) >> np.uint64(32)).astype(np.int64)
        else:       # mulhi of the 64-bit draw and the table's total, then lower_bound (Q-4)
            r = np.array([(((int(b) << 32) | int(a)) * total) >> 64 for a, b in zip(o0, o1)], np.int64)
            cand = np.searchsorted(cum, r, side="left").astype(np.int64)
        ok = ~seen[u[pending], cand] if opt.get("verify_neg", True) else np.ones(pending.size, bool)
        neg[pending[ok]] = cand[ok]
        pending, attempt = pending[~ok], attempt + 1
    return u, pos, neg


def warp_candidates(csr, seed, epoch, kmax):
    """warp.cc:134-139: per positive the first `kmax` draws that its user has not seen, and the attempt each came from."""
    cache = csr.__dict__.setdefault("_warp_candidates", {})
    key = (int(seed), int(epoch), int(kmax))
    if key not in cache:
        rows, seen, n = csr.rows().astype(np.int64), _seen_matrix(csr), csr.nnz
        cand, att, found = np.full((n, kmax), -1, np.int64), np.full((n, kmax), -1, np.int64), np.zeros(n, np.int64)
        pending, attempt = np.arange(n), 0
        while pending.size:
            o0, _ = _draw(seed, 1, pending, np.zeros(pending.size), epoch, np.full(pending.size, attempt))
            c = ((o0 * np.uint64(csr.num_items)) >> np.uint64(32)).astype(np.int64)
            hit = pending[~seen[rows[pending], c]]
            cand[hit, found[hit]], att[hit, found[hit]] = c[~seen[rows[pending], c]], attempt
            found[hit] += 1
            pending, attempt = pending[found[pending] < kmax], attempt + 1
        cache[key] = (cand, att)
    return cache[key]


# ---------------------------------------------------------------------------------------------
# one epoch of gradient accumulation
# ---------------------------------------------------------------------------------------------
class Epoch:
    """What `epoch_gradients` returns: gP, gQ, gQb, cP, cQ, the triples (u, pos, neg; WARP: the accepted ones), S_P, S_Q, S_b,
    unsafe, and for WARP scored / accepted (totals) and k (per positive: 1-based index of the violating candidate, 0: none)."""


def _add_rows(G, S, idx, terms, N=None):
    """G[idx[t]] += terms[t] for t in order (np.add.at is sequential), S the same with |terms| in float64 (S None: skipped), N the
    number of terms per row."""
    np.add.at(G, idx, terms.astype(G.dtype, copy=False))
    if S is not None:
        np.add.at(S, idx, np.abs(terms).astype(np.float64))
        np.add.at(N, idx, 1)


def _item_sorted_keep(items, chunk, defect):
    """The two gather defects as a mask over an incidence list (in list order): which incidences still reach gradQ."""
    keep = np.ones(items.shape[0], bool)
    order = np.argsort(items, kind="stable")
    if defect == "drop_incidence_at_chunk_end" and order.shape[0] >= chunk:
        keep[order[chunk - 1]] = False
    if defect == "second_flush_overwrites":
        it = items[order]
        k = np.arange(order.shape[0])
        # index of the last incidence of the run each incidence belongs to
        ends = np.flatnonzero(np.concatenate([it[1:] != it[:-1], [True]]))
        last_of_run = ends[np.searchsorted(ends, k, side="left")]
        keep[order[(k // chunk) != (last_of_run // chunk)]] = False
    return keep


def epoch_gradients(state, csr, opt, epoch, kind, cum=None, defect=None, chunk=256, triples=None, table=None):
    """One epoch's add_jobs over the whole matrix from `state` (its dtype is the run's): the gradient buffers start from
    state.grad* (Q-6), the counts from 0.  kind: "bpr" | "warp".  `triples` (BPR): explicit (u, pos, neg) in place of the sampler's
    (the injected form; one slot per positive).  `table`: the 1000 float32 values of the sigmoid table the backend under test
    holds (OracleBPRMF.exp_table(): the table is data of the specification, and libm's expf and numpy's float32 exp differ by an ulp
    in a third of its entries); default ref_numpy.exp_table()."""
    assert defect is None or defect in DEFECTS, defect
    dt = state.dtype
    assert defect is None or dt == np.float32, "defects are planted into the float32 run"
    f64 = dt == np.float64
    P, Q, Qb = state.P, state.Q, state.Qb
    U, I, d = P.shape[0], Q.shape[0], P.shape[1]
    out = Epoch()
    zero = defect == "grad_rezeroed"
    gP, gQ, gQb = (np.zeros_like(g) if zero else g.copy() for g in (state.gradP, state.gradQ, state.gradQb))
    S_P, S_Q, S_b = (np.abs(g).astype(np.float64) if f64 else None for g in (gP, gQ, gQb))
    cP, cQ = np.zeros(U, np.int64), np.zeros(I, np.int64)
    N_P, N_Q, N_b = np.zeros(U, np.int64), np.zeros(I, np.int64), np.zeros(I, np.int64)
    out.unsafe = out.unsafe_2x = 0
    if kind == "bpr":
        nn = 1 if triples is not None else int(opt["num_negative_samples"])
        u, pos, neg = triples if triples is not None else bpr_triples(csr, opt, epoch, cum)
        u, pos, neg = (np.asarray(a, np.int64) for a in (u, pos, neg))
        table = (rn.exp_table() if table is None else np.asarray(table, np.float32)).astype(dt)
        dq = Q[pos] - Q[neg]
        prod = P[u] * dq
        x = prod.sum(axis=1, dtype=dt)
        if opt["use_bias"]:
            x = x + (Qb[pos] - Qb[neg])
        # bpr.cc:124-131 (rn.bpr_logit on arrays): float * int in the run's type, truncated
        cell = np.clip(((x + dt(6)) * dt(1000 // 6 // 2)).astype(np.int64), 0, 999)
        c = np.where(x > 6, dt(0), np.where(x < -6, dt(1), table[cell])).astype(dt)
        if f64:
            # the float32 dot error (d + 2) 2^-24 sum |p (q_i - q_j)|, the bias terms counted into the sum, plus what the lookup itself
            # rounds: x + 6 (half an ulp of a number below 8, or below 16), its product with 83, and the sum with the bias difference
            delta = (d + 2) * U24 * (np.abs(prod).sum(axis=1) + (np.abs(Qb[pos]) + np.abs(Qb[neg]) if opt["use_bias"] else 0.0)) \
                + U24 * (np.where(x + 6.0 < 8.0, 8.0, 16.0) + (x + 6.0) + 2 * np.abs(x))
            y = (x + 6.0) * 83.0
            edge = np.minimum(y - np.floor(y), np.ceil(y) - y) / 83.0
            edge = np.where(np.abs(x) <= 6.0, edge, np.inf)
            out.unsafe = int(((edge <= delta) | (np.abs(np.abs(x) - 6.0) <= delta)).sum())
            out.unsafe_2x = int(((edge <= 2 * delta) | (np.abs(np.abs(x) - 6.0) <= 2 * delta)).sum())
        ui, uj = bool(opt["update_i"]), bool(opt["update_j"])
        _add_rows(gP, S_P, u, c[:, None] * dq, N_P)                                   # bpr.cc:145
        ideriv = c[:, None] * P[u]                                                # bpr.cc:134
        keep_p = keep_n = np.ones(u.shape[0], bool)
        if defect in ("drop_incidence_at_chunk_end", "second_flush_overwrites"):
            first = np.arange(0, u.shape[0], nn)                                  # the positive list has one incidence per position
            keep_p = np.repeat(_item_sorted_keep(pos[first], chunk, defect), nn)
            keep_n = _item_sorted_keep(neg, chunk, defect) if defect == "second_flush_overwrites" else keep_n
        # the reference adds +deriv to the positive's row and -deriv to the negative's triple by triple: one interleaved list
        idx = np.stack([pos, neg], axis=1).reshape(-1)
        terms = np.stack([ideriv, -ideriv], axis=1).reshape(-1, d)
        bterm = np.stack([c, -c], axis=1).reshape(-1)
        on = np.stack([ui & keep_p, uj & keep_n], axis=1).reshape(-1)
        _add_rows(gQ, S_Q, idx[on], terms[on], N_Q)                                    # bpr.cc:147-155
        if opt["use_bias"]:
            _add_rows(gQb, S_b, idx[on], bterm[on], N_b)
        # Q-9: a negative counts per triple, the positive and the user once per position, whatever update_i / update_j say
        per_pos = np.arange(0, u.shape[0], nn) if defect != "count_pos_per_slot" else np.arange(u.shape[0])
        skip = defect == "count_skips_unupdated_list"
        if not (skip and not uj):
            np.add.at(cQ, neg, 1)
        np.add.at(cP, u[per_pos], 1)
        if not (skip and not ui):
            np.add.at(cQ, pos[per_pos], 1)
        out.u, out.pos, out.neg = u, pos, neg
    else:
        assert kind == "warp", kind
        max_trial, thr, l2 = int(opt["max_trials"]), float(opt["threshold"]), opt.get("score_func") == "l2"
        kmax = max(1, (max_trial + 1) // 2)                                       # candidate k is scored while 2k - 1 <= max_trials
        cand, att = warp_candidates(csr, opt["random_seed"], epoch, kmax)
        rows, keys = csr.rows().astype(np.int64), csr.keys.astype(np.int64)
        n = csr.nnz

        def score(a, b):                                                          # warp.cc:21-28
            if not l2:
                return (a * b).sum(axis=-1, dtype=dt), np.abs(a * b).sum(axis=-1)
            df = a - b
            return -(df * df).sum(axis=-1, dtype=dt), (df * df).sum(axis=-1)
        s_i, a_i = score(P[rows], Q[keys])
        s_j, a_j = score(P[rows][:, None, :], Q[cand])
        diff = (s_i[:, None] - s_j).astype(dt)
        viol = diff.astype(np.float64) < thr
        if max_trial < 1:
            viol[:] = False
        found = viol.any(axis=1)
        k = np.where(found, viol.argmax(axis=1) + 1, 0)
        n_scored = np.where(found, k, kmax if max_trial >= 1 else 0)
        trial = np.where(found, 2 * k, 2 * kmax + 1)                              # Q-10
        acc = found & (trial < max_trial)                                         # warp.cc:148-149
        if f64:
            delta = (d + 2) * U24 * (a_i[:, None] + a_j) + 2 * U24 * (np.abs(s_i[:, None]) + np.abs(s_j))
            was_scored = np.arange(1, kmax + 1)[None, :] <= n_scored[:, None]
            out.unsafe = int((was_scored & (np.abs(diff - thr) <= delta)).sum())
            out.unsafe_2x = int((was_scored & (np.abs(diff - thr) <= 2 * delta)).sum())
        nseen = np.bincount(rows, minlength=U)[rows]
        tr = trial - 1 if defect == "phi_trial_off_by_one" else trial
        phi64 = np.log(np.maximum(1, (I - nseen - 1) // np.maximum(tr, 1)).astype(np.float64))
        if defect == "phi_zero_rejected":
            acc = acc & (phi64 > 0)
        t = np.flatnonzero(acc)
        u, pos, neg = rows[t], keys[t], cand[t, k[t] - 1]
        phi = phi64[t].astype(dt)[:, None]
        ru, ri, rj = (dt(np.float32(opt[r])) for r in ("reg_u", "reg_i", "reg_j"))
        if not l2:                                                                # warp.cc:30-40
            ud, idv, jdv = phi * (Q[pos] - Q[neg]), phi * P[u], -(phi * P[u])
        else:                                                                     # warp.cc:42-52
            ud, idv, jdv = phi * dt(2) * (Q[pos] - Q[neg]), phi * (P[u] - Q[pos]), -phi * (P[u] - Q[neg])
        _add_rows(gP, S_P, u, ud - ru * P[u], N_P)                                     # warp.cc:152-154
        ri, rj = np.full((t.shape[0], 1), ri, dt), np.full((t.shape[0], 1), rj, dt)
        if defect == "row_term_once_per_run":                                     # b n q_item with n = 1: the regulariser once per item and list
            for items, r in ((pos, ri), (neg, rj)):
                later = np.ones(items.shape[0], bool)
                later[np.unique(items, return_index=True)[1]] = False
                r[later] = 0
        ti, tj = idv - ri * Q[pos], jdv - rj * Q[neg]
        idx = np.stack([pos, neg], axis=1).reshape(-1)
        _add_rows(gQ, S_Q, idx, np.stack([ti, tj], axis=1).reshape(-1, d), N_Q)
        np.add.at(cP, u, 1)
        np.add.at(cQ, pos, 1)
        np.add.at(cQ, neg, 1)
        out.u, out.pos, out.neg = u, pos, neg
        out.k, out.attempt = k, np.where(found, att[np.arange(n), np.maximum(k, 1) - 1], -1)
        out.trial, out.phi, out.accepted_mask = trial, phi64, acc
        out.scored, out.accepted = int(n_scored.sum()), int(acc.sum())
    if defect == "gradq_row_scale":
        gQ *= (1 + 0.3 * np.sin(np.arange(I))).astype(dt)[:, None]
    out.gP, out.gQ, out.gQb, out.cP, out.cQ = gP, gQ, gQb, cP, cQ
    if f64:
        out.S_P, out.S_Q, out.S_b = S_P.max(axis=1), S_Q.max(axis=1), S_b
        # T_*: the same without the start values -- 0 exactly for a row that received no term
        out.T_P = (S_P - np.abs(state.gradP)).max(axis=1)
        out.T_Q = (S_Q - np.abs(state.gradQ)).max(axis=1)
        out.T_b = S_b - np.abs(state.gradQb)
        out.N_P, out.N_Q, out.N_b = N_P, N_Q, N_b
    return out


# ---------------------------------------------------------------------------------------------
# the epoch-end optimizer step
# ---------------------------------------------------------------------------------------------
def optimizer_step(X, grad, mom, vel, cnt, reg, opt, iters, project=False, bias=False, defect=None, rpw=1):
    """algo.cc:382-465 over one matrix ([rows, d]) or over the bias column ([rows], bias=True), warp.cc:192-201 behind it when
    `project`.  cnt: the per-row counts, or None without per_coordinate_normalize.  Returns the new (X, grad, mom, vel) in X's dtype;
    grad is the transformed step (Q-6)."""
    dt = X.dtype.type
    f = lambda v: dt(np.float32(v))   # noqa: E731  the reference rounds these to float32 before use
    X, grad, mom, vel = X.copy(), grad.copy(), (None if mom is None else mom.copy()), vel.copy()
    X0 = X.copy()
    col = (lambda a: a) if X.ndim == 1 else (lambda a: a[:, None])

    def projected(Y):
        nrm = np.sqrt((Y * Y).sum(axis=1, dtype=dt))
        return Y / np.maximum(dt(1), nrm)[:, None]
    if project and defect == "project_before_step":
        X = projected(X)
    if cnt is not None:                                                           # Q-9
        c = np.asarray(cnt)
        nz = c != 0
        if defect == "zero_count_divides":
            nz = np.ones_like(nz)
        if not (bias and defect == "bias_not_divided_without_use_bias" and not opt["use_bias"]):
            with np.errstate(divide="ignore", invalid="ignore"):
                grad[nz] = grad[nz] / col(c[nz].astype(dt))
    if bias and not opt["use_bias"]:                                              # algo.cc:415: the column is divided and left
        return X, grad, mom, vel
    grad = grad - X * f(2 * reg)
    with np.errstate(divide="ignore", invalid="ignore"):
        return _transform_and_step(X, X0, grad, mom, vel, opt, iters, project, projected, defect, rpw, f, dt)


def _transform_and_step(X, X0, grad, mom, vel, opt, iters, project, projected, defect, rpw, f, dt):
    if opt["optimizer"] == "adam":
        b1 = float(opt["beta1"])
        b2 = float(opt["beta2"]) if defect == "beta2_from_beta2" else b1          # sic: algo.cc:396
        mom = f(b1) * mom + f(1.0 - b1) * grad
        vel = f(b2) * vel + f(1.0 - b2) * (grad * grad)
        m_hat, v_hat = mom / f(1.0 - b1 ** (iters + 1)), vel / f(1.0 - b2 ** (iters + 1))
        grad = m_hat / (np.sqrt(v_hat + dt(FEPS)) if defect == "feps_inside_sqrt" else np.sqrt(v_hat) + dt(FEPS))
    else:
        vel = vel + grad * grad
        grad = grad / (np.sqrt(vel + dt(FEPS)) if defect == "feps_inside_sqrt" else np.sqrt(vel) + dt(FEPS))
    X = X + f(opt["lr"]) * grad
    if project and defect != "project_before_step":
        X = projected(X)
    if defect == "last_row_of_wave_skipped" and X.shape[0] % rpw:
        X[-1] = X0[-1]
    return X.astype(dt), grad.astype(dt), mom, vel.astype(dt)


def step_state(state, ep, opt, kind, defect=None, rpw_p=1, rpw_q=1):
    """update_parameters: the gradients and counts of `ep` through optimizer_step over P, Qb and Q; returns the new State."""
    pcn = bool(opt.get("per_coordinate_normalize"))
    proj = kind == "warp"
    o = dict(opt, use_bias=bool(opt.get("use_bias", False)))
    adam = opt["optimizer"] == "adam"
    s = state.copy()
    s.P, s.gradP, s.momP, s.velP = optimizer_step(state.P, ep.gP, state.momP if adam else None, state.velP, ep.cP if pcn else None,
                                                  opt["reg_u"], o, state.iters, proj, defect=defect, rpw=rpw_p)
    s.Qb, s.gradQb, s.momQb, s.velQb = optimizer_step(state.Qb, ep.gQb, state.momQb if adam else None, state.velQb, ep.cQ if pcn else None,
                                                      opt.get("reg_b", 0.0), o, state.iters, False, bias=True, defect=defect)
    s.Q, s.gradQ, s.momQ, s.velQ = optimizer_step(state.Q, ep.gQ, state.momQ if adam else None, state.velQ, ep.cQ if pcn else None,
                                                  opt["reg_i"], o, state.iters, proj, defect=defect, rpw=rpw_q)
    for n in ("momP", "momQ", "momQb"):
        if getattr(s, n) is None:
            setattr(s, n, np.zeros_like(getattr(state, n)))
    s.iters = state.iters + 1
    return s


def train(state, csr, opt, kind, epochs, cum=None, defect=None, chunk=256, table=None):
    """`epochs` epochs of add_jobs + update_parameters from `state` in its dtype; returns (final State, the epochs' Epoch records)."""
    eps = []
    for e in range(epochs):
        ep = epoch_gradients(state, csr, opt, state.iters, kind, cum=cum, defect=defect, chunk=chunk, table=table)
        state = step_state(state, ep, opt, kind, defect=defect)
        eps.append(ep)
    return state, eps


# ---------------------------------------------------------------------------------------------
# the stage errors
# ---------------------------------------------------------------------------------------------
def order_term(n):
    """What a float32 sum of n terms may differ by, relative to S, when it is taken in an order that the HARDWARE decides: every term
    its own atomic add (accum_two_pass = 0, update_triples).  Each of the n additions rounds the running sum, which is at most S, by at
    most 2^-24 S, uniformly: a random walk whose standard deviation is at most sqrt(n) 2^-24 S / sqrt(3).  The oracle's error is ONE draw
    of that walk (its loop order), the device's another, and a new one in every run; where few rows carry the scale -- the 32 entries
    of gradQb, of which two have more than a thousand terms -- 2.5 x the oracle's draw is no envelope of the device's (design
    `adam-d20-nn3-atomic-seed4`: 3.6 ... 4.0 x in three runs).  Four standard deviations."""
    return 4.0 * np.sqrt(np.asarray(n, np.float64) / 3.0) * U24


def stage_bound(err_oracle_worst, n_terms, hardware_order=False):
    """Per row: ref_eals.bound of the oracle's worst row; with `hardware_order` (per-triple atomics) plus the order term of the row's
    own number of terms.  The two-pass path sums a sorted run in registers, in one fixed order: it gets no such term."""
    b = bound(err_oracle_worst) + np.zeros(np.shape(n_terms))
    return b + order_term(n_terms) if hardware_order else b


def row_err(X, X64, S):
    """Per row: max_k |X - X64| / S over the rows with S > 0 (a 1-D array is a column of one-entry rows); the rest must keep their
    bits, which the caller asserts with `untouched`."""
    X, X64 = np.asarray(X, np.float64), np.asarray(X64, np.float64)
    dev = np.abs(X - X64) if X.ndim == 1 else np.abs(X - X64).max(axis=1)
    err = np.zeros(dev.shape[0])
    nz = S > 0
    err[nz] = dev[nz] / S[nz]
    return err


def elem_err(X, X64):
    """Elementwise |X - X64| / |X64| (0 where both are 0)."""
    X, X64 = np.asarray(X, np.float64), np.asarray(X64, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.abs(X - X64) / np.abs(X64)
    e[(X64 == 0) & (X == 0)] = 0.0
    return np.nan_to_num(e, nan=np.inf)


def untouched(X, start, S):
    """Rows that received nothing (S = 0) hold their start bit for bit."""
    z = S == 0
    return bool(np.array_equal(np.asarray(X)[z].view(np.uint32), np.asarray(start, np.float32)[z].view(np.uint32)))
