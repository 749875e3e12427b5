"""The yardstick of the item-major walk tests: the sequential replay of one closed component's triples in walk order
(walk_cases.py), in float64 and in the reference's float32, the classification of components into clean / safe, the device bound
and the planted defects that show it has teeth.

The step is the loop body of /root/reference/lib/algo_impl/bpr/bpr.cc:119-171 (Q-1: the user step sees the updated item rows); the
float32 form is `ref_numpy.bpr_sgd_step`, the float64 form below keeps the float32 constants (learning rate, regularisation) and the
float32 sigmoid table, and takes the bias step in double as the reference does."""
import numpy as np

import helpers as H
import ref_numpy as rn
import walk_cases as W

U24, U23 = 2.0 ** -24, 2.0 ** -23
DET = dict(sampler="counter", pos_order="csr", inline=True)
_traces, _items = {}, {}


def start_model(case, d, model_seed):
    """P, Q, Qb (float32, d columns).  Rows small enough that a dot product's float32 error is far below a table cell (1 / 83):
    sigma = 0.6 / sqrt(d), at most 0.1."""
    s = np.float32(min(0.1, 0.6 / np.sqrt(d)))
    key = (case.csr.num_items, d, model_seed)
    if key not in _items:            # the item side is large (up to 470 MB): one copy per (catalogue, d, seed), never written to
        rng = np.random.default_rng([model_seed, d])
        Q = rng.standard_normal((case.csr.num_items, d), dtype=np.float32) * s
        Qb = rng.standard_normal((case.csr.num_items, 1), dtype=np.float32) * np.float32(0.05)
        Q.flags.writeable = Qb.flags.writeable = False
        _items[key] = (Q, Qb)
    P = np.random.default_rng([model_seed, d, case.csr.num_users]).standard_normal((case.csr.num_users, d), dtype=np.float32) * s
    return (P,) + _items[key]


def negatives(oracle, case, opt, epochs):
    """[epochs, nnz, nn] the negatives the counter sampler draws (the oracle's trace; they do not depend on the model)."""
    from conftest import bpr_opt
    key = (id(case), opt["random_seed"], epochs, opt.get("verify_neg", True))
    if key not in _traces:
        csr = case.csr
        o = bpr_opt(d=4, lr=0.05, min_lr=0.05, num_iters=epochs, random_seed=opt["random_seed"], num_negative_samples=case.nn)
        P = np.zeros((csr.num_users, 4), np.float32)
        Q = np.zeros((csr.num_items, 4), np.float32)
        Qb = np.zeros((csr.num_items, 1), np.float32)
        tr = H.run_oracle_sgd(oracle.OracleBPRMF, o, csr, P, Q, Qb, epochs=epochs, modes=DET, trace=True).get_trace()
        n = csr.nnz * case.nn
        assert tr.shape[0] == epochs * n
        tr = tr.reshape(epochs, csr.nnz, case.nn, 3)
        assert (tr[..., 0] == csr.rows()[None, :, None]).all() and (tr[..., 1] == csr.keys[None, :, None]).all()
        _traces[key] = np.ascontiguousarray(tr[..., 2])
    return _traces[key]


def classify(case, negs):
    """clean[c]: no row of component c is touched by a triple outside it, over every epoch.  A negative that is a positive item of
    the matrix -- the component's own included: the walk holds a positive row in registers and a negative row in a replica, two
    copies -- spoils the drawer and the owner; a negative two components draw spoils both."""
    clean = np.ones(case.n_comp, bool)
    owner = {}
    for c in range(case.n_comp):
        for i in case.items[c]:
            owner[int(i)] = c
    drawn = {}
    comp = case.comp
    for e in range(negs.shape[0]):
        for pos in range(negs.shape[1]):
            for j in negs[e, pos]:
                j, c = int(j), int(comp[pos])
                if j in owner:
                    clean[c] = clean[owner[j]] = False
                elif drawn.setdefault(j, c) != c:
                    clean[c] = clean[drawn[j]] = False
    return clean


class Result:
    """users / items: the global ids of the rows; P, Q, Qb: their values after the replay; worst: the smallest distance of a
    triple's (x + 6) * 83 from a table edge over the float32 dot's error bound (float64 replay only; < 1: unsafe)."""


def _rows(case, negs, c):
    pos = W.walk_positions(case, c)
    items = np.unique(np.concatenate([case.items[c], negs[:, pos].reshape(-1)]))
    return pos, case.users[c], items


def replay(case, negs, c, model, opt, table, dtype, defect=None, flush=None):
    """Component c's triples, every epoch, in walk order, from `model` = (P, Q, Qb) float32 [., d].  `defect` = (name, step): see
    DEFECTS (float32 only).  `flush` (float32 only): per item id, the triples between two flushes of its register-resident copy
    (the device's "im_flush_every"; None = 1 everywhere) -- the grouping in which the bias steps of a run reach memory."""
    P0, Q0, Qb0 = model
    pos, users, items = _rows(case, negs, c)
    d = P0.shape[1]
    P, Q, Qb = P0[users].astype(dtype), Q0[items].astype(dtype), Qb0[items].astype(dtype)
    ul = {int(u): k for k, u in enumerate(users)}
    il = {int(i): k for k, i in enumerate(items)}
    lr = opt["lr"]
    f = np.float32
    lr32, ru, ri, rj = (float(f(opt[k])) for k in ("lr", "reg_u", "reg_i", "reg_j"))
    worst, step = np.inf, 0
    before_u, hist_i = {}, []
    csr = case.csr
    rows = csr.rows()
    seq = [(e, ul[int(rows[p])], il[int(csr.keys[p])], il[int(negs[e, p, slot])])
           for e in range(negs.shape[0]) for p in pos for slot in range(case.nn)]
    # The walk never stores a bias, it ADDS the step to the copy in memory, b + fl(b' - b): the flush of the register-resident item
    # (dbi_acc: the steps since the last flush, summed in float32), the atomic of a hot negative (dbj), the delta rule of the merge for
    # a replica's entry (B + (b' - B)).  A bias that a step carries through zero keeps the rounding of where it came from, which the
    # reference's b' = fl(...) does not have.  The step b' itself is the reference's, in double, on the walk's LOCAL copy of the
    # positive's bias: `loc`, beside what it owes memory (`acc`) -- flush_item / re_pending of csrc/bpr_item_major.hpp.
    cur, loc, acc, since, pending, bre = -1, f(0), f(0), 0, False, f(0)

    def end_run():
        if cur >= 0:
            Qb[cur, 0] = Qb[cur, 0] + acc

    for t, (e, u, i, j) in enumerate(seq):
        if dtype == np.float32:
            if defect and defect[1] == step and defect[0] == "lost_step":
                step += 1
                continue
            if i != cur:
                end_run()
                cur, loc, acc, since, pending = i, Qb[i, 0], f(0), 0, False
            if defect and defect[1] == step:
                if defect[0] == "stale_user":
                    P[u] = before_u[u]
                if defect[0] == "other_half_bias":
                    loc = Qb[j, 0]
                if defect[0] == "flush_twice":
                    Q[i] += Q[i] - hist_i[-8]
            before_u[u] = P[u].copy()
            hist_i.append(Q[i].copy())
            mem, bj0 = Qb[i, 0], Qb[j, 0]
            Qb[i, 0] = loc
            rn.bpr_sgd_step(P, Q, Qb, u, i, j, lr, opt, table)
            acc = acc + f(Qb[i, 0] - loc)
            loc = Qb[i, 0]
            Qb[i, 0] = mem
            Qb[j, 0] = bj0 + f(Qb[j, 0] - bj0)
            since += 1
            if pending:
                loc, pending = bre + acc, False
            goes_on = t + 1 < len(seq) and seq[t + 1][0] == e and seq[t + 1][2] == i
            if not goes_on:
                end_run()
                cur = -1
            elif since >= (1 if flush is None else int(flush[items[i]])):
                Qb[i, 0] = Qb[i, 0] + acc
                bre, acc, since, pending = Qb[i, 0], f(0), 0, opt["use_bias"]
            if defect and defect[1] == step and defect[0] == "fold_without_dqi":
                Q[i] = hist_i[-1]          # the step taken behind a flush never reaches the item row
            step += 1
            continue
        diff = Q[i] - Q[j]
        x = float(P[u] @ diff)
        S = float(np.abs(P[u] * diff).sum())
        bi, bj = (float(Qb[i, 0]), float(Qb[j, 0])) if opt["use_bias"] else (0.0, 0.0)
        x += bi - bj
        y = (x + 6.0) * 83.0
        edge = abs(y - round(y)) if -6.0 <= x <= 6.0 else 83.0 * (abs(x) - 6.0)
        bound = 83.0 * U24 * ((d + 4) * S + 4.0 * (abs(bi) + abs(bj)))
        worst = min(worst, edge / max(bound, 1e-300))
        logit = 0.0 if x > 6.0 else (1.0 if x < -6.0 else float(table[int(y)]))
        idv = logit * P[u]
        if opt["update_i"]:
            Q[i] += lr32 * (idv - ri * Q[i])
            if opt["use_bias"]:
                Qb[i, 0] += lr * (logit - opt["reg_b"] * Qb[i, 0])
        if opt["update_j"]:
            Q[j] += lr32 * (-idv - rj * Q[j])
            if opt["use_bias"]:
                Qb[j, 0] += lr * (-logit - opt["reg_b"] * Qb[j, 0])
        P[u] += lr32 * (logit * (Q[i] - Q[j]) - ru * P[u])
        step += 1
    r = Result()
    r.users, r.items, r.P, r.Q, r.Qb, r.worst, r.steps = users, items, P, Q, Qb, worst, step
    return r


def row_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).reshape(a.shape[0], -1).max(axis=1)


def ratio(got, r32, r64):
    """max over the rows of P, Q and the entries of Qb of err(got, f64) / (2.5 err(f32 replay, f64) + 4 * 2^-23 * max|f64 row|):
    the device bound holds iff this is <= 1.  `got` = (P, Q, Qb) on the replay's rows."""
    worst = 0.0
    for g, a32, a64 in zip(got, (r32.P, r32.Q, r32.Qb), (r64.P, r64.Q, r64.Qb)):
        bound = 2.5 * row_err(a32, a64) + 4.0 * U23 * np.abs(a64).reshape(a64.shape[0], -1).max(axis=1)
        worst = max(worst, float((row_err(g, a64) / bound).max()))
    return worst


# name -> (kind of the component it is planted in, step)
DEFECTS = {"lost_step": ("run", 30), "stale_user": ("grid", 20), "fold_without_dqi": ("run", 17), "other_half_bias": ("run", 33),
           "flush_twice": ("run", 40)}


def design_opt(design):
    from conftest import bpr_opt
    kw = dict(d=design["d"], lr=0.05, min_lr=0.05, num_iters=design["epochs"], random_seed=design["seed"],
              num_negative_samples=design["nn"], compute_loss_on_training=False)
    kw.update(design["opt"])
    return bpr_opt(**kw)


def design_case(design):
    return W.case(design["variant"], design["nn"], W.num_items_for(W.vdim_of(design["d"])))


_judged = {}


def ref_table(oracle):
    """The sigmoid table of bpr.cc:57-63 as the reference's own C++ evaluates it (the library builds its table the same way, on the
    host).  NOT `ref_numpy.exp_table()`: numpy's float32 exp differs from std::exp(float) in the last bit of 361 of the 1,000 cells,
    2e-7 of a step -- invisible in a factor row, an ulp of where it started in a bias that a step carries through zero."""
    if "t" not in _table:
        _table["t"] = oracle.OracleBPRMF().exp_table()
    return _table["t"]


_table = {}


def judge(oracle, design):
    """Everything the device test compares against, once per design: (case, opt, negs, model, clean, [(r32, r64) or None per
    component])."""
    if design["name"] in _judged:
        return _judged[design["name"]]
    table = ref_table(oracle)
    case, opt = design_case(design), design_opt(design)
    negs = negatives(oracle, case, opt, design["epochs"])
    clean = classify(case, negs)
    model = start_model(case, design["d"], design["model_seed"])
    refs = []
    for c in range(case.n_comp):
        refs.append((replay(case, negs, c, model, opt, table, np.float32), replay(case, negs, c, model, opt, table, np.float64)) if clean[c] else None)
    out = (case, opt, negs, model, clean, refs)
    _judged[design["name"]] = out
    return out


def usable(clean, refs):
    return np.array([bool(clean[c]) and refs[c][1].worst >= 1.0 for c in range(len(refs))])
