"""Shapes and drivers the CFR envelope tests share (test_cfr_ref_cpu.py, test_cfr_rows_gpu.py, test_cfr_gpu.py).

CoFactor builds its three row systems with the ALS Gramian kernel (csrc/als_kernels.hpp, als_gram_kernel) run through four switches
nobody else sets: `ctx` (weight 1, coefficient v - bias_self - bias_other), `accumulate` (two passes add into one slot),
`out_scale` and `ff_scale`.  The kernel eats a row in 64-entry chunks, in pairs, the last pair of an odd row half padding; a row
above 4,096 entries is cut into work items that add into the row's slot (als_core.hpp, work_list).  `pattern` puts a row on
either side of every one of those bounds into every one of the four passes, and gives every pass more work items than the launch
has waves, so some wave takes a second ticket.  `tiny_a` / `tiny_b`: two matrices of one shape with different row bounds.
"""
import functools
import os

import numpy as np

import helpers as H
from conftest import tiny_csr
from ref_cfr import ARRAYS, F64CFR, bound, relerr

NAMED_LENGTHS = (0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 8193)     # 8193 = 2732 + 2732 + 2729: three chunks, odd tail
N_PATTERN = 8300        # users = items: the smallest square shape that holds a three-chunk row beside 63 untouched ids
FIRST_FREE = 64         # the long rows draw their columns from ids >= 64, so rows 0 .. 53 of the other orientation stay exact
N_LONG = len(NAMED_LENGTHS) + 40
CHUNKED_CALLS = ((0, 14), (14, 14), (14, 54), (54, 5000), (5000, N_PATTERN))
WAVES_PER_CU = 16       # launch_gram_to_slots: min(ceil(n / 4), 4 CUs) blocks of 4 waves


def opt(d, optimizer, **kw):
    o = {"d": d, "num_workers": 2, "num_cg_max_iters": 3, "alpha": 4.0, "l": 0.7, "eps": 1e-10, "reg_u": 0.1, "reg_i": 0.2, "reg_c": 0.3,
         "compute_loss": True, "optimizer": optimizer, "cg_tolerance": 1e-10, "num_iters": 2, "model_path": "", "data_opt": {}}
    o.update(kw)
    return o


def lengths_of(csr):
    return np.diff(np.concatenate([[0], csr.indptr]))


def _long_rows(rng, lengths, n_cols, first):
    """Rows of exactly `lengths` entries, columns drawn from [first, n_cols) -> (rows, cols)."""
    rows = np.repeat(np.arange(len(lengths)), lengths)
    cols = np.concatenate([np.sort(rng.choice(np.arange(first, n_cols), size=n, replace=False)) for n in lengths])
    return rows, cols


def _csr(n_rows, n_cols, rows, cols, vals):
    from buffalo_amd.synth import CSR
    key = rows.astype(np.int64) * n_cols + cols
    assert np.unique(key).shape[0] == key.shape[0]
    order = np.argsort(key, kind="stable")
    cnt = np.bincount(rows, minlength=n_rows)
    return CSR(n_rows, n_cols, np.cumsum(cnt, dtype=np.int64), cols[order].astype(np.int32), vals[order].astype(np.float32))


class Case:
    """rating matrix (user-major `csr`, item-major `t`) and the item x item context matrix `ctx`."""
    def __init__(self, csr, ctx):
        self.csr, self.t, self.ctx = csr, csr.transpose(), ctx
        self.users, self.items = csr.num_users, csr.num_items
        assert ctx.num_users == ctx.num_items == self.items

    def work_items(self):
        """Work items of the four Gramian passes (user, item <- users, item <- contexts, context): one per row with entries, the rows
        above 4,096 entries one per chunk (als_core.hpp, work_list)."""
        def items(m):
            n = lengths_of(m)
            total = int((n > 0).sum())
            for k in n[n > 4096].tolist():
                nch = -(-k // 4096)
                per = (-(-k // nch) + 1) & ~1       # chunks of ceil(n / nch) entries, rounded up to even
                total += -(-k // per) - 1
            return total
        return {"user": items(self.csr), "item<-user": items(self.t), "item<-context": items(self.ctx), "context": items(self.ctx)}


@functools.lru_cache(maxsize=None)
def pattern():
    """U = I = 8,300.  The rating matrix is A u B^T: A gives user rows 0 .. 53 the NAMED_LENGTHS, then 40 lengths of 1 .. 200, on
    items >= 64; B gives item rows 0 .. 53 the same lengths on users >= 64; every user and every item from 64 on gets two more
    entries.  Items 54 .. 63 have no user entries at all: they are solved from their one context entry.  The context matrix: rows
    0 .. 53 of those lengths, every row above them the one entry (x, (7x + 1) mod N).  About 65,000 rating entries and 32,000 context entries."""
    rng = np.random.default_rng(23)
    N = N_PATTERN
    lengths = list(NAMED_LENGTHS) + [int(x) for x in rng.integers(1, 201, size=40)]
    ar, ac = _long_rows(rng, lengths, N, FIRST_FREE)                # user rows 0 .. 53
    bi, bu = _long_rows(rng, lengths, N, FIRST_FREE)                # item rows 0 .. 53
    M = N - FIRST_FREE                                              # 8236 = 4 x 29 x 71: 3 and 5 are units, both maps are bijections
    u = np.arange(FIRST_FREE, N)
    e1, e2 = FIRST_FREE + (3 * (u - FIRST_FREE) + 5) % M, FIRST_FREE + (5 * (u - FIRST_FREE) + 11) % M
    keep = e1 != e2
    rows = np.concatenate([ar, bu, u, u[keep]])
    cols = np.concatenate([ac, bi, e1, e2[keep]])
    rows = np.concatenate([rows, np.arange(N_LONG, FIRST_FREE)])    # users 54 .. 63: one entry each, so that only row 0 is empty
    cols = np.concatenate([cols, FIRST_FREE + np.arange(N_LONG, FIRST_FREE)])
    key = np.unique(rows.astype(np.int64) * N + cols)
    rows, cols = key // N, key % N
    csr = _csr(N, N, rows, cols, 1 + rng.poisson(1.0, size=rows.shape[0]))
    cr, cc = _long_rows(rng, lengths, N, 0)
    x = np.arange(N_LONG, N)
    cr, cc = np.concatenate([cr, x]), np.concatenate([cc, (7 * x + 1) % N])
    ctx = _csr(N, N, cr, cc, rng.normal(1.0, 1.0, size=cr.shape[0]))
    case = Case(csr, ctx)
    for m in (case.csr, case.t, case.ctx):
        assert tuple(lengths_of(m)[:N_LONG]) == tuple(lengths), lengths_of(m)[:N_LONG]
    assert not lengths_of(case.t)[N_LONG:FIRST_FREE].any() and lengths_of(case.ctx)[N_LONG:].min() == 1
    return case


def assert_second_tickets(case, cus):
    """Every Gramian pass of a whole-matrix call must hold more work items than the launch has waves on a device of `cus` CUs."""
    for name, n in case.work_items().items():
        assert n > WAVES_PER_CU * cus, "pass %s: %d work items do not outnumber %d waves (%d CUs assumed)" % (name, n, WAVES_PER_CU * cus, cus)


@functools.lru_cache(maxsize=None)
def tiny(seed):
    """The 150 x 90 / 90 x 90 shapes of test_cfr_gpu.py."""
    return Case(tiny_csr(U=150, I=90, density=0.1, seed=seed, counts=True), tiny_csr(U=90, I=90, density=0.15, seed=seed + 1, counts=True))


@functools.lru_cache(maxsize=None)
def gaps():
    """The 6 x 5 case of test_cfr_gpu.py: users 1 and 3 empty, items 1 and 4 without context entries."""
    from buffalo_amd.synth import CSR
    return Case(CSR(6, 5, [2, 2, 3, 3, 5, 6], [0, 3, 1, 0, 4, 2], np.array([1, 2, 1, 3, 1, 2], np.float32)),
                CSR(5, 5, [1, 1, 3, 4, 4], [2, 0, 4, 1], np.array([0.5, 1.5, 0.25, 2.0], np.float32)))


def case_of(name):
    if name == "pattern":
        return pattern()
    if name == "gaps":
        return gaps()
    return tiny({"tiny_a": 3, "tiny_b": 13}[name])


def arrays(case, d, seed=9):
    """The float32 start state: the five arrays, normal(scale 0.2)."""
    rng = np.random.default_rng(seed)
    f = lambda r, c: rng.normal(scale=0.2, size=(r, c)).astype(np.float32)     # noqa: E731
    return {"user": f(case.users, d), "item": f(case.items, d), "context": f(case.items, d), "item_bias": f(case.items, 1),
            "context_bias": f(case.items, 1)}


def bind(obj, arrs):
    for name in ARRAYS:
        obj.set_embedding(arrs[name], name.encode("utf8"))


# one update, in the calls of `ranges` (row ranges like BufferedDataMatrix.fetch_batch hands them out) -> the summed loss
def update_user(obj, case, ranges=None):
    obj.precompute(b"item")
    return sum(obj.partial_update_user(a, b, case.csr.indptr, *_chunk(case.csr, a, b)) for a, b in ranges or [(0, case.users)])


def update_item(obj, case, ranges=None):
    obj.precompute(b"user")
    return sum(obj.partial_update_item(a, b, case.t.indptr, *_chunk(case.t, a, b), case.ctx.indptr, *_chunk(case.ctx, a, b))
               for a, b in ranges or [(0, case.items)])


def update_context(obj, case, ranges=None):
    return sum(obj.partial_update_context(a, b, case.ctx.indptr, *_chunk(case.ctx, a, b)) for a, b in ranges or [(0, case.items)])


def _chunk(m, a, b):
    if b == a:
        return m.keys[:0], m.vals[:0]
    return H.chunk_arrays(m, a, b)


UPDATES = {"U": update_user, "I": update_item, "C": update_context}
SINGLE_STEPS = ("U", "I", "C")                  # each from the same float32 state
STEPS_THEN_EPOCH = ("U", "I", "C", "E")         # ... then one free-running epoch (cfr.py: users, items, contexts) from that state


class Snap:
    """The five arrays after one step and the loss(es) its calls returned."""
    def __init__(self, step, arrs, loss):
        self.step, self.arrs, self.loss = step, arrs, loss


def run(make, case, d, optimizer, schedule, ranges=None, start=None, **kw):
    """Drive one backend (`make()` -> object with CyCFR's surface, initialised here) through `schedule`: every step binds fresh
    copies of the start state, so single steps do not compound -> [Snap per step]."""
    path = H.write_opt(opt(d, optimizer, **kw))
    start = start or arrays(case, d)
    try:
        obj = make()
        assert obj.init(path)
        return [step(obj, case, s, start, ranges) for s in schedule]
    finally:
        os.unlink(path)


def step(obj, case, s, start, ranges=None):
    arrs = {k: v.copy() for k, v in start.items()}
    bind(obj, arrs)
    loss = [UPDATES[u](obj, case, ranges) for u in ("UIC" if s == "E" else s)]
    return Snap(s, arrs, loss)


@functools.lru_cache(maxsize=None)
def references(name, d, optimizer, schedule):
    """The oracle's and the yardstick's runs of one case, computed once per process and shared: ([oracle Snap], [f64 Snap])."""
    from oracle import oracle as orc
    orc.build()
    case = case_of(name)
    return run(orc.OracleCFR, case, d, optimizer, schedule), run(F64CFR, case, d, optimizer, schedule)


EPOCH_NEIGHBOURS = 5


@functools.lru_cache(maxsize=None)
def epoch_distance(name, d, optimizer):
    """The oracle's distance to float64 after the free-running epoch, as the envelope of an "E" step takes it: per array the LARGEST
    of err(oracle, f64) over the case's start state and EPOCH_NEIGHBOURS neighbours of it, in each of which one entry in a thousand
    of `item`, `context` and `context_bias` is moved by one float32 ulp (oracle and yardstick both run from the neighbour).

    Why: the third update of the epoch solves systems of condition 250 .. 900 (items of norm 5 .. 6 after the item step) in three
    float32 CG steps, whose rounding error is cond x 2^-24 and changes with the last bit of any input -- while the result itself does
    not (the same neighbours move the float64 run by less than 1e-6, third result).  The oracle's own distance is therefore one draw from a wide cloud:
    over these six starts of `pattern`, d = 33 it is 2.3e-5 .. 6.5e-5 for `context_bias` and 7.3e-6 .. 1.6e-5 for `context`
    (profiles/cfr_parity.txt), a spread of 2.8 that the factor 2.5 on a single draw cannot hold.  The device's last bits differ from
    the oracle's from the first update on (and from run to run in the rows above 4,096 entries, whose chunks add in ticket order),
    so it draws from that cloud too.  The single steps keep the single oracle run: the issue's bound as it stands.
    -> ({array: distance}, [{array: err} per start], [{array: relerr(f64 of the start, f64 of start 0)} per start])"""
    from oracle import oracle as orc
    orc.build()
    case = case_of(name)
    base = arrays(case, d)
    rng = np.random.default_rng(1)
    draws, moved, f0 = [], [], None
    for k in range(1 + EPOCH_NEIGHBOURS):
        start = {n: v.copy() for n, v in base.items()}
        if k:
            for n in ("item", "context", "context_bias"):
                m = rng.random(start[n].shape) < 1e-3
                start[n][m] = np.nextafter(start[n][m], np.float32(np.inf))
        o = run(orc.OracleCFR, case, d, optimizer, ("E",), start=start)[0]
        f = run(F64CFR, case, d, optimizer, ("E",), start=start)[0]
        f0 = f0 or f
        draws.append({n: relerr(o.arrs[n], f.arrs[n]) for n in ARRAYS})
        moved.append({n: relerr(f.arrs[n], f0.arrs[n]) for n in ARRAYS})
    return {n: max(e[n] for e in draws) for n in ARRAYS}, draws, moved


def hold(section, hip, orc, f64, named=None, epoch=None):
    """Every array of every snapshot of the device run inside the envelope of the oracle's; the figures are recorded first.
    `named`: print the per-row errors of the first `named` rows of the arrays a step wrote, so that a failure names a row length.
    `epoch`: the oracle's distance an "E" step is held to (`epoch_distance`); required where the schedule has one."""
    lines, bad = [], []
    touched = {"U": ("user",), "I": ("item", "item_bias"), "C": ("context", "context_bias"), "E": ARRAYS}
    for h, o, f in zip(hip, orc, f64):
        for name in ARRAYS:
            eo, eh = relerr(o.arrs[name], f.arrs[name]), relerr(h.arrs[name], f.arrs[name])
            if h.step == "E":
                assert epoch[name] >= eo
                eo = epoch[name]
            if name not in touched[h.step]:
                assert eo == 0.0 and eh == 0.0, (h.step, name, eo, eh)      # a step leaves the other arrays alone
                continue
            ln = "step %s %-12s err(oracle, f64) %.3g%s err(hip, f64) %.3g ratio %.2f of bound %.3g: %.2f" % (
                h.step, name, eo, " (largest of %d starts)" % (1 + EPOCH_NEIGHBOURS) if h.step == "E" else "", eh, eh / max(eo, 1e-30), bound(eo),
                eh / bound(eo))
            lines.append(ln)
            if not eh <= bound(eo) or not np.isfinite(h.arrs[name]).all():
                bad.append(ln)
            if named and h.step != "E":
                scale = np.abs(f.arrs[name]).max()
                per = ["%d: %.2g / %.2g" % (n, np.abs(o.arrs[name][i] - f.arrs[name][i]).max() / scale,
                                            np.abs(h.arrs[name][i] - f.arrs[name][i]).max() / scale) for i, n in enumerate(NAMED_LENGTHS[:named])]
                lines.append("  per row, entries: err(oracle) / err(hip)  " + "  ".join(per))
    record(section, lines)
    assert not bad, "\n".join(lines)
    return lines


def record(section, lines):
    """Print the measured figures of one case (pytest -s shows them); with BFH_CFR_PARITY_OUT=<file> they are appended to that file
    as well -- profiles/cfr_parity.txt is the output of such a run, so that a plain test run leaves the checkout clean."""
    text = "".join("%s | %s\n" % (section, ln) for ln in lines)
    print(text, end="")
    out = os.environ.get("BFH_CFR_PARITY_OUT")
    if out:
        with open(out, "a") as f:
            f.write(text)
