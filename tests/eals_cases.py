"""Shapes and drivers the eALS envelope tests share (test_eals_ref_cpu.py, test_eals_rows_gpu.py, test_eals_gpu.py).

csrc/eals_handle.hpp sends a row to one of three kernels by its entry count: light (<= 256, registers), mid (257 .. 4096, one wave,
a shared scratch slot of `cap` entries), heavy (> 4096, one 1024-thread block, its own slot).  `pattern` puts a row on either side
of every one of those bounds and of the 64-entry rounding of the slots; `many` has more mid and more heavy rows than the launches
have groups on a 256-CU device, so some group takes a second ticket; `heavy` is the smallest matrix whose item rows all run on the
block-per-row kernel.
"""
import functools
import os

import numpy as np

import helpers as H
from conftest import tiny_csr
from ref_eals import F64EALS

EALS_LIGHT, EALS_HEAVY = 256, 4096      # csrc/eals_kernels.hpp
NAMED_LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, 319, 320, 321, 1024, 4095, 4096, 4097, 4160, 4161, 6000)
PATTERN_COLS = 6000


def opt(d, **kw):
    o = {"d": d, "num_workers": 2, "alpha": 2.0, "reg_u": 0.1, "reg_i": 0.2, "num_iters": 3, "c0": 0.5, "exponent": 0.5, "model_path": "",
         "data_opt": {}}
    o.update(kw)
    return o


@functools.lru_cache(maxsize=None)
def pattern(side):
    """Long side: rows of exactly NAMED_LENGTHS entries, in that order, then 40 rows of 1 .. 200; 6,000 columns.  "user": the long
    rows are user rows (axis 0, Cw gathered per entry); "item": the transpose, the long rows are item rows (axis 1, cx per row)."""
    from buffalo_amd.synth import CSR
    rng = np.random.default_rng(11)
    lengths = list(NAMED_LENGTHS) + [int(x) for x in rng.integers(1, 201, size=40)]
    keys = np.concatenate([np.sort(rng.choice(PATTERN_COLS, size=n, replace=False)) for n in lengths]).astype(np.int32)
    vals = (1 + rng.poisson(1.0, size=keys.shape[0])).astype(np.float32)
    csr = CSR(len(lengths), PATTERN_COLS, np.cumsum(lengths, dtype=np.int64), keys, vals)
    assert side in ("user", "item")
    return csr if side == "user" else csr.transpose()


@functools.lru_cache(maxsize=None)
def many():
    """4,200 user rows of 504 .. 520 entries (mid) and 520 item rows of 4138 .. 4173 entries (heavy)."""
    csr = tiny_csr(U=4200, I=520, density=0.99, seed=5, counts=True)
    lu, li = lengths_of(csr), lengths_of(csr.transpose())
    assert EALS_LIGHT < lu.min() and lu.max() <= EALS_HEAVY < li.min(), (lu.min(), lu.max(), li.min(), li.max())
    return csr


@functools.lru_cache(maxsize=None)
def heavy():
    """12 item rows of about 4,275 entries: every one on the block-per-row kernel; user rows of <= 12 entries."""
    csr = tiny_csr(U=4500, I=12, density=0.95, seed=4, counts=True)
    assert lengths_of(csr.transpose()).min() > EALS_HEAVY
    return csr


def lengths_of(csr):
    return np.diff(np.concatenate([[0], csr.indptr]))


def matrix(name):
    if name == "tiny":
        return tiny_csr(U=120, I=70, density=0.12, seed=1, counts=True)
    if name == "empty_rows":
        from buffalo_amd.synth import CSR
        return CSR(6, 5, [2, 2, 3, 3, 5, 6], [0, 3, 1, 0, 4, 2], np.array([1, 2, 1, 3, 1, 2], np.float32))
    if name == "long":     # item rows of ~540 entries (mid), user rows of ~54
        return tiny_csr(U=600, I=60, density=0.9, seed=2, counts=True)
    if name == "mid":      # item rows of ~2,300 entries: the upper half of the one-wave class
        return tiny_csr(U=2500, I=24, density=0.92, seed=4, counts=True)
    if name == "heavy":
        return heavy()
    if name == "many":
        return many()
    assert name in ("pattern_user", "pattern_item"), name
    return pattern(name[8:])


def problem(name, d, seed=0):
    """-> (csr, P, Q, Cw): float32 factors normal(scale 0.3); Cw = 0.5 sqrt(pop) / sum (eals.py:50-53 at c0 0.5, exponent 0.5)."""
    csr = matrix(name)
    rng = np.random.default_rng(seed)
    P = rng.normal(scale=0.3, size=(csr.num_users, d)).astype(np.float32)
    Q = rng.normal(scale=0.3, size=(csr.num_items, d)).astype(np.float32)
    pop = np.bincount(csr.keys, minlength=csr.num_items).astype(np.float64) ** 0.5
    Cw = (0.5 * pop / pop.sum()).astype(np.float32)
    return csr, P, Q, Cw


# schedules: "I" = fresh object, initialize_model from the case's float32 state, both caches; "0" / "1" = update(axis)
HALVES_THEN_EPOCH = ("I", "0", "I", "1", "I", "0", "1")                 # one half-epoch on each axis from the same state, one epoch
HALVES_THEN_2_EPOCHS = HALVES_THEN_EPOCH + ("0", "1")
ONE_EPOCH = ("I", "0", "1")
TWO_EPOCHS = ("I", "0", "1", "0", "1")


class Snap:
    """What a backend holds after one `update`: the factors and the loss read through either orientation."""
    def __init__(self, step, axis, P, Q, loss):
        self.step, self.axis, self.P, self.Q, self.loss = step, axis, P, Q, loss

    def X(self):
        return self.P if self.axis == 0 else self.Q


def bind(obj, prob):
    """initialize_model on copies of the case's factors + both caches -> (P, Q) the object now updates."""
    csr, P0, Q0, Cw = prob
    t = csr.transpose()
    P, Q = P0.copy(), Q0.copy()
    obj.initialize_model(P, Q, Cw)
    obj.precompute_cache(csr.nnz, csr.indptr, csr.keys, 0)
    obj.precompute_cache(csr.nnz, t.indptr, t.keys, 1)
    return P, Q


def step(obj, prob, axis, P, Q, k=0, losses=True):
    csr = prob[0]
    t = csr.transpose()
    m = csr if axis == 0 else t
    assert obj.update(m.indptr, m.keys, m.vals, axis)
    Pn, Qn = obj.factors() if hasattr(obj, "factors") else (P, Q)
    loss = None
    if losses:
        loss = (obj.estimate_loss(csr.nnz, csr.indptr, csr.keys, csr.vals, 0)[1], obj.estimate_loss(csr.nnz, t.indptr, t.keys, t.vals, 1)[1])
    return Snap(k, axis, Pn.copy(), Qn.copy(), loss)


def run(make, d, prob, schedule, losses=True):
    """Drive one backend (`make()` -> object with CyEALS's surface) through `schedule` -> [Snap per update]."""
    path = H.write_opt(opt(d))
    snaps, obj, P, Q = [], None, None, None
    try:
        for k, s in enumerate(schedule):
            if s == "I":
                obj = make()
                assert obj.init(path)
                P, Q = bind(obj, prob)
            else:
                snaps.append(step(obj, prob, int(s), P, Q, k, losses))
    finally:
        os.unlink(path)
    return snaps


@functools.lru_cache(maxsize=None)
def references(name, d, schedule, seed=0):
    """The oracle's and the yardstick's runs of one case, computed once per process and shared: ([oracle Snap], [f64 Snap])."""
    from oracle import oracle as orc
    orc.build()
    prob = problem(name, d, seed)
    return run(orc.OracleEALS, d, prob, schedule), run(F64EALS, d, prob, schedule)


def record(section, lines):
    """Print the measured figures of one case (pytest -s shows them); with BFH_EALS_PARITY_OUT=<file> they are appended to that
    file as well -- profiles/eals_parity.txt is the output of such a run, so that a plain test run leaves the checkout clean."""
    text = "".join("%s | %s\n" % (section, ln) for ln in lines)
    print(text, end="")
    out = os.environ.get("BFH_EALS_PARITY_OUT")
    if out:
        with open(out, "a") as f:
            f.write(text)
