"""Yardsticks and drivers the fold-in tests share (test_als_fold_in_cpu.py, test_als_fold_in_gpu.py).

bfh_als_fold_in solves, for every row b of a CSR of histories with entries (k_j, v_j), n_b of them, against the other factor Y
(axis 0: Q, reg_u; axis 1: P, reg_i):

    A = Y^T Y + alpha sum_j v_j y_kj y_kj^T + reg ada I      ada = n_b under adaptive_reg, else 1
    y = sum_j (1 + alpha v_j) y_kj
    out[b] = A^-1 y                                         n_b == 0: the zero row

`fold_f64` is that in float64 (np.linalg.solve), `fold_f32` the same in float32 with an unblocked Cholesky (the comparison run at d = 128,
where the oracle's ALS is forced to iALS++), `oracle_fold` the float32 oracle: an OracleALS with optimizer "llt", zeros for the side being
solved and the histories as its matrix -- one precompute + partial_update, whose rows with entries ARE the fold-in.

The bound is ref_eals.bound as it stands, over all rows and per named row of als_cases.pattern():
relerr(hip, f64) <= 2.5 x relerr(comparison run, f64) + 4 x 2^-23, relerr of a row taken against that row's own largest entry.
"""
import functools
import os

import numpy as np

import als_cases as AC
import helpers as H
from ref_eals import bound, relerr

ALPHA, REG = 4.0, (0.2, 0.3)      # als_cases.opt: alpha, (reg_u, reg_i)
DEFECTS = ("drop_last_entry", "reg_not_adaptive", "y_without_one", "skip_last_diagonal")


def rows_of(m):
    beg = np.concatenate([[0], m.indptr[:-1]])
    return [(int(b), int(e)) for b, e in zip(beg, m.indptr)]


def _system(Y, FF, k, v, reg, adaptive, dt, defect=None):
    """(A, y) of one history in dtype `dt`; `defect` plants one of DEFECTS."""
    d = Y.shape[1]
    n = k.shape[0]
    if defect == "drop_last_entry":
        k, v = k[:-1], v[:-1]
    Yk = Y[k].astype(dt)
    w = (dt(ALPHA) * v.astype(dt)).astype(dt)
    A = (FF + (Yk * w[:, None]).T @ Yk).astype(dt)
    ada = dt(n) if adaptive and defect != "reg_not_adaptive" else dt(1)
    diag = np.full(d, dt(reg) * ada, dtype=dt)
    if defect == "skip_last_diagonal":
        diag[-1] = 0
    A[np.arange(d), np.arange(d)] += diag
    c = w if defect == "y_without_one" else (dt(1) + w).astype(dt)
    y = (Yk * c[:, None]).sum(axis=0, dtype=dt)
    return A, y


def fold_f64(m, Y, axis, adaptive=False, rows=None):
    """Section 1 of the issue in float64: [rows, d]."""
    Y64 = Y.astype(np.float64)
    FF = Y64.T @ Y64
    out = np.zeros((m.num_users, Y.shape[1]))
    bounds = rows_of(m)
    todo = [b for b in (range(m.num_users) if rows is None else rows) if bounds[b][1] > bounds[b][0]]
    for i in range(0, len(todo), 64):
        systems = [_system(Y64, FF, m.keys[slice(*bounds[b])], m.vals[slice(*bounds[b])], REG[axis], adaptive, np.float64) for b in todo[i:i + 64]]
        out[todo[i:i + 64]] = np.linalg.solve(np.stack([s[0] for s in systems]), np.stack([s[1] for s in systems])[:, :, None])[:, :, 0]
    return out


def cholesky_solve_f32(A, y):
    """Unblocked float32 Cholesky (column by column, every operation rounded to float32) and the two triangular solves, for a stack of
    systems A [n, d, d], y [n, d] at once (the loop over columns is the Python loop, the systems ride along in numpy)."""
    A = np.array(A, dtype=np.float32)
    z = np.array(y, dtype=np.float32)
    d = A.shape[1]
    for j in range(d):
        A[:, j, j] = np.sqrt(A[:, j, j])
        A[:, j + 1:, j] /= A[:, j, j][:, None]
        l = A[:, j + 1:, j]
        A[:, j + 1:, j + 1:] -= l[:, :, None] * l[:, None, :]
    for r in range(d):
        z[:, r] = (z[:, r] - np.einsum("nk,nk->n", A[:, r, :r], z[:, :r])) / A[:, r, r]
    for r in range(d - 1, -1, -1):
        z[:, r] = (z[:, r] - np.einsum("nk,nk->n", A[:, r + 1:, r], z[:, r + 1:])) / A[:, r, r]
    return z


def fold_f32(m, Y, axis, adaptive=False, rows=None, defect=None, defect_row=None):
    """The same in float32; `defect` (one of DEFECTS) is planted in row `defect_row` only."""
    Y32 = np.ascontiguousarray(Y, dtype=np.float32)
    FF = (Y32.T @ Y32).astype(np.float32)
    out = np.zeros((m.num_users, Y.shape[1]), dtype=np.float32)
    bounds = rows_of(m)
    todo = [b for b in (range(m.num_users) if rows is None else rows) if bounds[b][1] > bounds[b][0]]
    for i in range(0, len(todo), 32):
        systems = [_system(Y32, FF, m.keys[slice(*bounds[b])], m.vals[slice(*bounds[b])], REG[axis], adaptive, np.float32,
                           defect if b == defect_row else None) for b in todo[i:i + 32]]
        out[todo[i:i + 32]] = cholesky_solve_f32(np.stack([s[0] for s in systems]), np.stack([s[1] for s in systems]))
    return out


def kw_of(adaptive, optimizer=None):
    kw = {"adaptive_reg": True} if adaptive else {}
    if optimizer:
        kw["optimizer"] = optimizer
    return AC.K(**kw)


def oracle_fold(case, axis, Y, d, adaptive=False):
    """The float32 oracle's fold-in (d < 128): zeros for the side being solved, `Y` for the other, one llt half-epoch over the histories."""
    from oracle import oracle as orc
    orc.build()
    obj, path = orc.OracleALS(), H.write_opt(AC.opt(d, kw_of(adaptive, "llt")))
    try:
        assert obj.init(path)
    finally:
        os.unlink(path)
    m = case.mat(axis)
    X = np.zeros((m.num_users, d), dtype=np.float32)
    Yc = np.ascontiguousarray(Y, dtype=np.float32).copy()
    obj.initialize_model(*((X, Yc) if axis == 0 else (Yc, X)))
    obj.precompute(axis)
    obj.partial_update(0, m.num_users, m.indptr, m.keys, m.vals, axis)
    assert np.array_equal(Yc, Y)
    return X


def comparison_rows(n_rows, d):
    """The rows the comparison run is evaluated on.  The oracle (d < 128) runs every row.  fold_f32 (d = 128) costs a Python loop of 128 numpy
    steps per 32 rows, 15 s over pattern()'s 8,300: it runs the N_LONG rows that carry the lengths and every 16th row behind them.  Its distance
    from float64 is a MAXIMUM over rows, so leaving rows out can only lower it, and the bound with it -- never widen it."""
    if d < 128:
        return np.arange(n_rows)
    return np.concatenate([np.arange(min(AC.N_LONG, n_rows)), np.arange(AC.N_LONG, n_rows, 16)])


@functools.lru_cache(maxsize=None)
def references(d, adaptive=False, axis=0):
    """(comparison run, float64 yardstick, the factor folded against [rows, d], the rows the comparison run holds) of als_cases.pattern(),
    computed once per process.  axis 0: the user rows against Q; axis 1: the item rows (the transposed matrix) against P.  d = 128: the
    comparison run is fold_f32 on comparison_rows (zeros elsewhere)."""
    case = AC.pattern()
    P, Q = AC.start(case, d)
    Y = Q if axis == 0 else P
    m = case.mat(axis)
    rows = comparison_rows(m.num_users, d)
    f64 = fold_f64(m, Y, axis, adaptive)
    cmp_run = oracle_fold(case, axis, Y, d, adaptive) if d < 128 else fold_f32(m, Y, axis, adaptive, rows)
    for a in (cmp_run, f64, Y, rows):
        a.setflags(write=False)
    return cmp_run, f64, Y, rows


def err_over(X, f64, rows=None):
    """relerr over the rows `rows` (all: None), against the largest entry of the WHOLE yardstick."""
    sel = slice(None) if rows is None else rows
    return float(np.abs(np.asarray(X, np.float64)[sel] - f64[sel]).max() / max(np.abs(f64).max(), 1e-30))


def hold(section, X, cmp_run, f64, rows=None, named=AC.NAMED):
    """X inside the envelope of the comparison run: over all rows of X (the comparison run's distance taken over `rows`, see comparison_rows)
    and per named row, a row's relerr against its own largest entry; the figures are recorded first (als_cases.record)."""
    eo, eh = err_over(cmp_run, f64, rows), err_over(X, f64)
    lines = ["all rows: err(comparison, f64) %.3g err(run, f64) %.3g ratio %.2f of bound %.3g: %.2f" % (eo, eh, eh / max(eo, 1e-30), bound(eo), eh / bound(eo))]
    bad = [] if eh <= bound(eo) and np.isfinite(X).all() else [lines[0]]
    per = []
    for i in range(named):
        ro, rh = relerr(cmp_run[i], f64[i]), relerr(X[i], f64[i])
        per.append("%d: %.2g / %.2g" % (AC.NAMED_LENGTHS[i], ro, rh))
        if not rh <= bound(ro):
            bad.append("row %d (%d entries): err(comparison) %.3g err(run) %.3g bound %.3g" % (i, AC.NAMED_LENGTHS[i], ro, rh, bound(ro)))
    lines.append("  per row, entries: err(comparison) / err(run)  " + "  ".join(per))
    AC.record(section, lines)
    assert not bad, "\n".join(bad + lines)
    return lines


def make_hip(d, adaptive=False, modes=None, optimizer=None):
    """A CyALS at d with the options of als_cases.opt (optimizer "ialspp" unless named: fold_in solves exactly whatever it is)."""
    return AC.make_hip(d, kw_of(adaptive, optimizer), modes)


def bind(obj, case, d, P=None, Q=None):
    """initialize_model with the signed-normal start of als_cases (or the given factors), padded to vdim -> (P, Q) as bound."""
    P0, Q0 = AC.start(case, d)
    vdim = AC.vdim_of(d)
    Pp, Qp = H.pad((P0 if P is None else P).copy(), vdim), H.pad((Q0 if Q is None else Q).copy(), vdim)
    obj.initialize_model(Pp, Qp)
    return Pp, Qp
