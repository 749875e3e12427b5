"""The float64 ALS yardstick (ref_numpy.als_half_epoch_f64_fast) held to the per-entry loop version and to the oracle, and proof that
the device bound built on it has teeth: single-point mistakes of the kind a row kernel can make, planted into the float64
evaluation, land far outside 2.5 x err(oracle, f64) + 4 ulp.

Measured (profiles/als_parity.txt, part 1): on the signed start of als_cases.py the oracle sits 3.6e-7 .. 6.7e-6 from float64 over every
(case, d, options) the device file runs -- `pattern` at d = 32 .. 300 on all three solver kinds, `pattern_outliers`, `tiny_a` / `tiny_b`.
CAP is the largest of them with 2x headroom, rounded up to the next power of ten."""
import numpy as np
import pytest

import als_cases as AC
import ref_numpy as rn
from ref_eals import bound, relerr

CAP = 1e-4      # set from 6.7e-6 (pattern_outliers, d = 160, item side; 2x passes 1e-5); a case above it does not belong in the envelope tests

# every (case, d, options) test_als_rows_gpu.py runs
YARDSTICK_CASES = [("pattern", 32, AC.K()), ("pattern", 64, AC.K()), ("pattern", 96, AC.K()), ("pattern", 128, AC.K()),
                   ("pattern", 40, AC.K(optimizer="ldlt", adaptive_reg=True)), ("pattern", 70, AC.K(optimizer="manual_cg", num_cg_max_iters=5)),
                   ("pattern", 100, AC.K(block_size=7)), ("pattern", 160, AC.K()), ("pattern", 192, AC.K()), ("pattern", 224, AC.K()),
                   ("pattern", 256, AC.K()), ("pattern", 160, AC.K(block_size=64)), ("pattern", 160, AC.K(block_size=96)), ("pattern", 300, AC.K()),
                   ("pattern_outliers", 96, AC.K()), ("pattern_outliers", 128, AC.K()), ("pattern_outliers", 160, AC.K()),
                   ("tiny_a", 128, AC.K()), ("tiny_b", 128, AC.K())]


def test_pattern_has_the_rows_it_promises():
    case = AC.pattern()
    for m in (case.csr, case.t):
        n = AC.lengths_of(m)
        assert tuple(n[:AC.NAMED]) == AC.NAMED_LENGTHS and n[0] == 0 and (n[1:] > 0).all()
    assert AC.chunks_of_row(4097) == [2050, 2047] and AC.chunks_of_row(8192) == [4096, 4096] and AC.chunks_of_row(8193) == [2732, 2732, 2729]
    AC.assert_second_tickets(case, 256, 16)         # the MI355X has 256 CUs: 4,096 waves per launch of the Gramian kernels
    out = AC.pattern_outliers()
    for m in (out.csr, out.t):
        assert AC.deferred(m) == (AC.N_DEF, AC.N_DEF_ROWS) and AC.N_DEF * 4 <= AC.work_items(m)
    a, b = AC.case_of("tiny_a"), AC.case_of("tiny_b")
    assert (a.users, a.items) == (b.users, b.items) and not np.array_equal(a.csr.indptr, b.csr.indptr) and not np.array_equal(a.t.indptr, b.t.indptr)


@pytest.mark.parametrize("d,kw", [(128, AC.K()), (100, AC.K(block_size=7)), (70, AC.K(optimizer="manual_cg", num_cg_max_iters=5)),
                                  (40, AC.K(optimizer="ldlt", adaptive_reg=True))])
def test_fast_driver_is_the_loop_version(d, kw):
    """200 sampled rows of `pattern`, every named length up to 1025 among them: the half-epoch driver (matrix products, short rows many
    at a time) against the per-entry loops of ialspp_row_f64 / als_normal_equations, both float64."""
    case = AC.pattern()
    o = AC.opt(d, kw)
    P, Q = AC.start(case, d)
    named = [i for i, n in enumerate(AC.NAMED_LENGTHS) if n <= 1025]
    rows = sorted(set(named) | set(np.random.default_rng(3).choice(np.arange(AC.NAMED, case.users), 200 - len(named), replace=False).tolist()))
    worst = 0.0
    for axis in (0, 1):
        X, Y = (P, Q) if axis == 0 else (Q, P)
        ff = (Y.astype(np.float64).T @ Y.astype(np.float64))
        m = case.mat(axis)
        T, nume, deno = rn.als_half_epoch_f64_fast(X, Y, ff, m, o, axis, rows=rows)
        reg = o["reg_u"] if axis == 0 else o["reg_i"]
        want_n = want_d = 0.0
        for u in rows:
            keys, vals = m.row(u)
            if not len(keys):
                assert np.array_equal(T[u], X[u].astype(np.float64))
                continue
            if d >= 128 or o["optimizer"] == "ialspp":
                want = rn.ialspp_row_f64(X, Y, ff, u, keys, vals, o["alpha"], reg, o["block_size"])
            else:
                A, y = rn.als_normal_equations(X, Y, ff, u, keys, vals, o["alpha"], reg, o["adaptive_reg"])
                want = rn.manual_cg_f64(X[u], A, y, iters=o["num_cg_max_iters"], tol=o["cg_tolerance"], eps=o["eps"]) \
                    if o["optimizer"] == "manual_cg" else np.linalg.solve(A, y)
            worst = max(worst, float(np.abs(T[u] - want).max() / np.abs(want).max()))
            ln, ld = rn.als_loss_terms(X, Y, ff, u, keys, vals, o["alpha"], reg, o["adaptive_reg"], axis)
            want_n, want_d = want_n + ln, want_d + ld
        assert abs(nume - want_n) <= 1e-12 * abs(want_n) and abs(deno - want_d) <= 1e-12 * max(abs(want_d), 1.0), (axis, nume, want_n, deno, want_d)
    AC.record("cpu fast driver vs loop version, pattern d=%d %s" % (d, dict(kw)), ["largest row difference over %d rows x 2 sides: %.3g" % (len(rows), worst)])
    assert worst <= 1e-12, worst


@pytest.mark.parametrize("name,d,kw", YARDSTICK_CASES)
def test_yardstick_follows_the_oracle(name, d, kw):
    orc, f64 = AC.references(name, d, kw)
    lines, worst = [], 0.0
    for o, f in zip(orc, f64):
        e = relerr(o.X, f.X)
        worst = max(worst, e)
        per = np.abs(o.X - f.X).max(axis=1) / np.abs(f.X).max()
        q = float(np.quantile(per, 0.999))
        lines.append("axis %d: err(oracle, f64) %.3g; per row 99.9 %% quantile %.3g, largest row / quantile %.2f; loss oracle %.9g %.9g f64 %.12g %.12g" % (
            o.axis, e, q, per.max() / q, o.loss[0], o.loss[1], f.loss[0], f.loss[1]))
        # the oracle's double accumulators over float per-entry terms against the float64 sums
        assert abs(o.loss[0] - f.loss[0]) <= 1e-6 * abs(f.loss[0]) and abs(o.loss[1] - f.loss[1]) <= 1e-6 * max(abs(f.loss[1]), 1.0), lines
        # no heavy tail: the bound of the device test is a maximum over rows, and must not be one ill-conditioned row's error
        assert per.max() <= 10 * q, lines
    AC.record("cpu yardstick vs oracle, %s d=%d %s" % (name, d, dict(kw)), lines + ["largest %.3g (cap %g)" % (worst, CAP)])
    assert worst <= CAP, lines


def _work_order(m):
    """Rows in work-list order: longest first, ties in row order (als_core.hpp, work_list; the chunks of a heavy row left aside)."""
    n = AC.lengths_of(m)
    rows = np.flatnonzero(n > 0)
    return rows[np.argsort(-np.minimum(n[rows], AC.HEAVY), kind="stable")].tolist()


def _planted(defect, case, axis, X):
    """-> (rows the defect changes, keyword arguments of als_half_epoch_f64_fast that plant it)."""
    m = case.mat(axis)
    n = AC.lengths_of(m)
    named = list(range(AC.NAMED))
    if defect == "tail_entry_lost":             # entry n - 1 dropped where it is alone in its group of 16
        rows = [r for r in named if n[r] % 16 == 1 and n[r] > 1]
        return rows, dict(entries=lambda u, k, v: (k[:-1], v[:-1]))
    if defect == "pad_lane_weighted":           # the one padding lane of the last group (row 0 of the other factor) with the row's last weight
        rows = [r for r in named if n[r] % 16 == 15]
        return rows, dict(entries=lambda u, k, v: (np.append(k, 0).astype(k.dtype), np.append(v, v[-1]).astype(v.dtype)))
    if defect == "chunk_added_twice":           # the last chunk's tile and gradient added to the row's slot twice
        rows = [AC.NAMED_LENGTHS.index(4097), AC.NAMED_LENGTHS.index(8193)]

        def twice(u, k, v):
            last = AC.chunks_of_row(len(k))[-1]
            return np.concatenate([k, k[-last:]]), np.concatenate([v, v[-last:]])
        return rows, dict(entries=twice)
    assert defect == "stale_row_header"         # a one-entry row solved with the p0 of the work item before it
    order = _work_order(m)
    rows = [r for r in named if n[r] == 1]
    return rows, dict(start=lambda u: X[order[order.index(u) - 1]])


DEFECTS = ("tail_entry_lost", "pad_lane_weighted", "chunk_added_twice", "stale_row_header")
TEETH_CASES = [(128, AC.K()), (70, AC.K(optimizer="manual_cg", num_cg_max_iters=5))]


# (the dense solvers do not read the row they replace: llt / ldlt solve A x = y outright, and manual_cg drops a start whose residual
#  is larger than |y| (algo.cc:66-69), which a random row's always is -- a stale p0 is an iALS++ defect, planted at d = 128 only)
@pytest.mark.parametrize("defect,d,kw", [(f, d, kw) for d, kw in TEETH_CASES for f in DEFECTS if not (f == "stale_row_header" and d < 128)])
def test_the_device_bound_has_teeth(defect, d, kw):
    """Each planted single-point mistake moves the factor by at least 10 x what the envelope allows a device run; per row the figure is
    printed, and rows where one entry among thousands stays under 10 x are named in the profile (the bound stays)."""
    case = AC.pattern()
    orc, f64 = AC.references("pattern", d, kw)
    P, Q = AC.start(case, d)
    lines, ratios = [], []
    for axis in (0, 1):
        X, Y = (P, Q) if axis == 0 else (Q, P)
        rows, plant = _planted(defect, case, axis, X)
        assert rows
        bad, _, _ = rn.als_half_epoch_f64_fast(X, Y, f64[axis].ff, case.mat(axis), AC.opt(d, kw), axis, rows=rows, **plant)
        allowed = bound(relerr(orc[axis].X, f64[axis].X))
        scale = np.abs(f64[axis].X).max()
        per = {int(AC.lengths_of(case.mat(axis))[r]): float(np.abs(bad[r] - f64[axis].X[r]).max() / scale / allowed) for r in rows}
        ratios.append(max(per.values()))
        lines.append("%s, axis %d: device bound %.3g; moved / bound per row (entries: ratio) %s%s" % (
            defect, axis, allowed, "  ".join("%d: %.0f" % kv for kv in per.items()),
            "; UNDER 10 x: rows of %s entries" % [k for k, v in per.items() if v < 10] if min(per.values()) < 10 else ""))
    AC.record("cpu teeth, pattern d=%d %s" % (d, dict(kw)), lines)
    assert all(r >= 10 for r in ratios), lines
