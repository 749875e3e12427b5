"""ALS on the device against the float64 yardstick (ref_numpy.als_half_epoch_f64_fast): the row lengths at which the kernels that only
ALS runs change course (als_cases.py maps every length of `pattern` to its branch), on every kernel family one partial_update chooses
between -- and every test first asserts, through the plan read-back ("als_last_*", include/buffalo_hip.h), that the family it names is
the one that ran.

The bound everywhere: err(hip, f64) <= 2.5 x err(oracle, f64) + 4 x 2^-23 (ref_eals.bound) per half-epoch, both from the same float32
state, each backend against the recurrence started from its own Gramian (the device's FF is held to float64 at 1e-5 by
test_als_gpu.py::test_precompute_gramian_mfma, at this shape too).  The loss: |hip - f64| <= |oracle - f64| + 8 x 2^-24 |f64|
(ref_eals.loss_bound).  What was measured (ratios per case and per named row) is in profiles/als_parity.txt."""
import numpy as np
import pytest

import als_cases as AC
from ref_eals import loss_bound

pytestmark = pytest.mark.gpu

PC0, PC2, F32, NOREG = {"als_pc": 0}, {"als_pc": 2}, {"als_split_f16": 0}, {"als_inreg": 0}
# id: (d, options, modes, the path and the split flag the plan must report, consumers per CU of that kernel's launch)
#   16 waves per CU for the Gramian kernels (and as many rows in flight for the fallback), 4 pairs per CU for als_pc_kernel,
#   als_wide_blocks_per_cu(T, split) workgroups for the wide kernel
DESIGNS = {
    "pairs-64": (64, AC.K(), PC2, "pairs", 1, 4), "pairs-96": (96, AC.K(), {}, "pairs", 1, 4), "pairs-128": (128, AC.K(), {}, "pairs", 1, 4),
    "wave-64": (64, AC.K(), {}, "wave", 1, 16), "wave-96": (96, AC.K(), PC0, "wave", 1, 16), "wave-128": (128, AC.K(), PC0, "wave", 1, 16),
    "fp32-128": (128, AC.K(), F32, "wave", 0, 16),
    "scratch-128": (128, AC.K(), NOREG, "scratch", 0, 16),
    "wave-32": (32, AC.K(), {}, "wave", 0, 16),                                  # T = 1: in-register, the fp32 instruction (the split form starts at T = 2)
    "dense-40": (40, AC.K(optimizer="ldlt", adaptive_reg=True), {}, "scratch", 0, 16),
    "dense-70": (70, AC.K(optimizer="manual_cg", num_cg_max_iters=5), {}, "scratch", 0, 16),
    "dense-100": (100, AC.K(block_size=7), {}, "scratch", 0, 16),               # iALS++ with padding and another block size: als_solve_kernel
    "wide-160": (160, AC.K(), {}, "wide", 1, 3), "wide-224": (224, AC.K(), {}, "wide", 1, 1),
    "wide-192": (192, AC.K(), {}, "wide", 1, 2), "wide-256": (256, AC.K(), {}, "wide", 0, 2),     # as the handle chooses: split up to T = 7
    "fallback-160-bs64": (160, AC.K(block_size=64), {}, "fallback", 0, 16),     # als_ialspp_kernel<4, 1>
    "fallback-160-bs96": (160, AC.K(block_size=96), {}, "fallback", 0, 16),     # <4, 2>
    "fallback-300": (300, AC.K(), {}, "fallback", 0, 16),                       # vdim 320: <8, 1>, the last block 12 wide
}


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _assert_plans(hip, path, split, case=None, n_def=(0, 0)):
    """Every call of both half-epochs ran `path` (a call without rows: none) on the work list the host expects."""
    for h in hip:
        assert h.plans
        for p in h.plans:
            if p["path"] == "none":
                continue
            assert (p["path"], p["split"]) == (path, split), (h.axis, p)
            if path != "fallback":                      # the fallback walks rows, not a work list
                assert p["n_work"] > 0 and (p["n_def"], p["n_def_rows"]) == n_def, (h.axis, p)
        if case is not None and len(h.plans) == 1 and path != "fallback":
            m = case.mat(h.axis)
            assert h.plans[0]["n_work"] == AC.work_items(m) and h.plans[0]["n_heavy"] == int((AC.lengths_of(m) > AC.HEAVY).sum()), h.plans


def _f64_of(case, d, kw, hip):
    return AC.f64_run(case, d, kw, [h.ff for h in hip])


def _properties(hip, case, d):
    state = AC.start(case, d)
    for h in hip:
        assert np.isfinite(h.X).all()
        assert not h.pad.any()                                          # padding columns stay 0
        assert np.array_equal(h.X[0], state[h.axis][0])                 # the row without entries keeps its bits


@pytest.mark.parametrize("design", list(DESIGNS))
def test_row_lengths_and_their_edges(design):
    d, kw, modes, path, split, per_cu = DESIGNS[design]
    case = AC.pattern()
    cus = _cus()
    hip = AC.run("hip", case, d, kw, modes)
    _assert_plans(hip, path, split, case)
    AC.assert_second_tickets(case, cus, per_cu)
    orc, f64 = AC.references("pattern", d, kw)
    AC.hold("rows pattern %s (%d CUs)" % (design, cus), hip, orc, f64, _f64_of(case, d, kw, hip), named=AC.NAMED)
    _properties(hip, case, d)


@pytest.mark.parametrize("d,path", [(96, "pairs"), (128, "pairs"), (160, "wide")])
def test_deferred_rows_at_the_edges(d, path):
    """Weights outside the f16 path in rows AT the bounds: a one-entry row, one group, one key chunk, the second chunk of 65, the
    longest one-item row, and single chunks of the 4,097- and 8,193-entry rows (slot = the heavy row's; whole rows: n_heavy + j).
    The pairs send those items to the fp32 instruction; the wide kernel falls back to its fp32 form for the whole call."""
    case = AC.pattern_outliers()
    hip = AC.run("hip", case, d, AC.K(), {"als_split_wcut": AC.WCUT})
    _assert_plans(hip, path, int(path == "pairs"), case, n_def=(AC.N_DEF, AC.N_DEF_ROWS))
    orc, f64 = AC.references("pattern_outliers", d, AC.K())
    AC.hold("deferred rows pattern_outliers d=%d %s" % (d, path), hip, orc, f64, _f64_of(case, d, AC.K(), hip), named=AC.NAMED)
    _properties(hip, case, d)


def test_chunked_calls():
    """Every half-epoch made in the calls [0, 14) [14, 14) [14, 72) [72, 5000) [5000, N), keys / vals handed over per call.  A row of
    one work item reads its own entries, FF, the other factor and the split scale (max |Q| alone): bit-identical to the one-call
    run.  The chunks of the rows above 4,096 entries add into their slot in ticket order: those rows may differ."""
    d, kw = 128, AC.K()
    case = AC.pattern()
    one = AC.run("hip", case, d, kw)
    cut = AC.run("hip", case, d, kw, ranges=AC.chunked_calls)
    _assert_plans(one, "pairs", 1, case)
    _assert_plans(cut, "pairs", 1)
    assert [[p["path"] for p in h.plans] for h in cut] == [["pairs", "none", "pairs", "pairs", "pairs"]] * 2
    orc, f64 = AC.references("pattern", d, kw)
    AC.hold("chunked calls pattern d=%d" % d, cut, orc, f64, _f64_of(case, d, kw, cut), named=AC.NAMED)
    _properties(cut, case, d)
    lines = []
    for a, b in zip(one, cut):
        light = AC.lengths_of(case.mat(a.axis)) <= AC.HEAVY
        diff = np.flatnonzero((a.X != b.X).any(axis=1))
        lines.append("axis %d: %d rows differ from the one-call run, %d of them of one work item%s; loss one call %r chunked %r" % (
            a.axis, diff.shape[0], int(light[diff].sum()), (" (rows %s)" % diff[:8].tolist()) if diff.shape[0] else "", a.loss, b.loss))
        assert not light[diff].any(), lines
        assert abs(a.loss[0] - b.loss[0]) <= 1e-9 * abs(a.loss[0]) and a.loss[1] == b.loss[1], lines      # double sums in another order
    AC.record("chunked calls pattern d=%d" % d, lines)


@pytest.mark.parametrize("d,modes,path", [(96, {}, "pairs"), (64, {}, "wave"), (160, {}, "wide")])
def test_losses_against_float64(d, modes, path):
    """(nume, deno) as als.cc:175-200 forms them, from the rows BEFORE their solve.  The device sums in double like the oracle's
    accumulators, so it gets no factor over the oracle's distance, only the rounding of the float-sized terms."""
    case = AC.pattern()
    hip = AC.run("hip", case, d, AC.K(), modes)
    _assert_plans(hip, path, 1, case)
    orc, f64 = AC.references("pattern", d, AC.K())
    fh = _f64_of(case, d, AC.K(), hip)
    lines, bad = [], []
    for h, o, f, g in zip(hip, orc, f64, fh):
        for k, name in enumerate(("nume", "deno")):
            allowed = loss_bound(o.loss[k], f.loss[k])
            ln = "axis %d %s: f64 %.12g |oracle - f64| %.3g |hip - f64| %.3g allowed %.3g" % (h.axis, name, g.loss[k], abs(o.loss[k] - f.loss[k]),
                                                                                            abs(h.loss[k] - g.loss[k]), allowed)
            lines.append(ln)
            if not abs(h.loss[k] - g.loss[k]) <= allowed:
                bad.append(ln)
    AC.record("losses pattern d=%d %s" % (d, path), lines)
    assert not bad, "\n".join(lines)
    off = AC.run("hip", case, d, AC.K(compute_loss_on_training=False), modes)
    _assert_plans(off, path, 1, case)
    for h, o in zip(hip, off):
        assert o.loss == (0.0, 0.0)
        light = AC.lengths_of(case.mat(h.axis)) <= AC.HEAVY         # (the chunks of the three longer rows add in ticket order, run by run)
        assert np.array_equal(h.X[light], o.X[light])               # the rows do not depend on the switch, bit for bit


def _half_on(obj, case, axis, P, Q, keys=True):
    """One half-epoch on the model the handle holds (no re-binding): P / Q are the host arrays it writes back to."""
    m = case.mat(axis)
    obj.precompute(axis)
    loss = obj.partial_update(0, m.num_users, m.indptr, *(AC.chunk(m, 0, m.num_users) if keys else (None, None)), axis)
    return (P if axis == 0 else Q).copy(), loss, AC.plan_of(obj)


def _fresh(case, d, P, Q):
    g = AC.make_hip(d)
    P, Q = P.copy(), Q.copy()
    AC.bind(g, case, P, Q, True)
    return g, P, Q


def test_a_used_handle_follows_the_matrix_it_is_handed():
    """One CyALS, d = 128.  `tiny_a` and `tiny_b` have one shape and different row bounds: whatever the handle remembers of the first
    (work lists, weight scans, the auto-resident copy, the interleaved factor, FF p0, scratch) must not reach the second."""
    d = 128
    a, b, big = AC.case_of("tiny_a"), AC.case_of("tiny_b"), AC.pattern()
    g = AC.make_hip(d)
    P, Q = AC.start(a, d)
    AC.bind(g, a, P, Q, True)
    for axis in (0, 1):                                             # one free-running epoch on tiny_a
        assert _half_on(g, a, axis, P, Q)[2]["path"] == "pairs"
    lines = []
    # set_placeholder with tiny_b, then a half-epoch of each side: a fresh handle started from the same factors gives the same bits
    g.set_placeholder(b.csr.indptr, b.t.indptr, b.csr.nnz + 1)
    for axis in (0, 1):
        f, Pf, Qf = _fresh(b, d, P, Q)
        want, wl, _ = _half_on(f, b, axis, Pf, Qf)
        got, gl, plan = _half_on(g, b, axis, P, Q)
        lines.append("set_placeholder tiny_b, axis %d: %d rows differ from a fresh handle's, loss %r / %r" % (axis, int((got != want).any(axis=1).sum()), gl, wl))
        assert plan["path"] == "pairs" and np.array_equal(got, want) and gl == wl, lines
    # the same through set_resident_csr: tiny_a resident, used, then tiny_b resident (keys / vals NULL in the calls)
    for axis, m in ((0, a.csr), (1, a.t)):
        g.set_resident_csr(axis, m.indptr, m.keys, m.vals)
        _half_on(g, a, axis, P, Q, keys=False)
    for axis, m in ((0, b.csr), (1, b.t)):
        g.set_resident_csr(axis, m.indptr, m.keys, m.vals)
    for axis in (0, 1):
        f, Pf, Qf = _fresh(b, d, P, Q)
        want, wl, _ = _half_on(f, b, axis, Pf, Qf)
        got, gl, plan = _half_on(g, b, axis, P, Q, keys=False)
        lines.append("set_resident_csr tiny_b, axis %d: %d rows differ from a fresh handle's, loss %r / %r" % (axis, int((got != want).any(axis=1).sum()), gl, wl))
        assert plan["path"] == "pairs" and np.array_equal(got, want) and gl == wl, lines
    # from the start state the used handle is inside the envelope like a fresh one (AC.half binds the model again)
    g2 = AC.make_hip(d)
    AC.half(g2, a, 0, AC.start(a, d), d, True)
    used = [AC.half(g2, b, axis, AC.start(b, d), d, True) for axis in (0, 1)]
    orc, f64 = AC.references("tiny_b", d, AC.K())
    AC.hold("used handle: tiny_a then tiny_b d=%d" % d, used, orc, f64, _f64_of(b, d, AC.K(), used))
    # initialize_model again with FEWER rows: a user row depends on its own entries and the items alone
    n = 100
    Ps, Qs = AC.start(b, d)
    fewer = Ps[:n].copy()
    g2.initialize_model(fewer, Qs.copy())
    g2.set_placeholder(b.csr.indptr, b.t.indptr, b.csr.nnz + 1)
    g2.precompute(0)
    g2.partial_update(0, n, b.csr.indptr, *AC.chunk(b.csr, 0, n), 0)
    assert np.array_equal(fewer, used[0].X[:n])
    from buffalo_amd.backend import BuffaloHipError
    with pytest.raises(BuffaloHipError, match="bad row range"):
        g2.partial_update(0, n + 1, b.csr.indptr, *AC.chunk(b.csr, 0, n + 1), 0)
    # `pattern` after the tiny shapes: scratch, FF p0, the interleaved copy and the work cache have only seen smaller ones
    hip = [AC.half(g2, big, axis, AC.start(big, d), d, True) for axis in (0, 1)]
    _assert_plans(hip, "pairs", 1, big)
    fresh = AC.run("hip", big, d)
    for h, f in zip(hip, fresh):
        diff = np.flatnonzero((h.X != f.X).any(axis=1))
        lines.append("pattern after tiny, axis %d: %d rows differ from a fresh handle's (rows %s)" % (h.axis, diff.shape[0], diff[:8].tolist()))
        assert (AC.lengths_of(big.mat(h.axis))[diff] > AC.HEAVY).all(), lines
    orc, f64 = AC.references("pattern", d, AC.K())
    AC.hold("used handle: pattern after tiny d=%d" % d, hip, orc, f64, _f64_of(big, d, AC.K(), hip), named=AC.NAMED)
    # a call of rows without any entries: row 0 of `pattern` alone
    Pb, Qb = (x.copy() for x in AC.start(big, d))
    AC.bind(g2, big, Pb, Qb, True)
    for axis in (0, 1):
        g2.precompute(axis)
        assert g2.partial_update(0, 1, big.mat(axis).indptr, *AC.chunk(big.mat(axis), 0, 1), axis) == (0.0, 0.0)
        plan = AC.plan_of(g2)
        assert plan["n_work"] == 0 and plan["n_heavy"] == 0, plan
    assert np.array_equal(Pb, AC.start(big, d)[0]) and np.array_equal(Qb, AC.start(big, d)[1])
    AC.record("used handle d=%d" % d, lines)
