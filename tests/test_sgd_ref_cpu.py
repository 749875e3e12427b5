"""The yardstick of the SGD accumulate stage tests (ref_sgd.py) held to the C++ oracle, the cases of sgd_cases.py held to what they
were built to contain, and the planted defects that show the stage bound has teeth where the end-to-end tests have none.

Why the stage tests exist (test_gradq_row_scale_is_invisible_end_to_end): adagrad and adam divide a gradient by its own running
magnitude, so with reg = 0 a positive per-row scale on gradQ cancels out of the trained model -- 1 + 0.3 sin(row) on every gradQ
row moves Q by 8.9e-8 (helpers.relerr after three epochs, the measure of test_bpr_gpu.py / test_warp_gpu.py; asserted < 1e-4), while
the gradient stage sees it 177,000 x over its bound."""
import numpy as np
import pytest

from conftest import bpr_opt, warp_opt
import helpers as H
import ref_sgd as rs
import sgd_cases as sc

ORACLE_MODES = dict(sampler="counter", pos_order="csr", inline=True)
_cases = {}


def _case(name):
    if name not in _cases:
        _cases[name] = sc.make_case(name)
    return _cases[name]


def _oracle(orc, kind, opt, csr, cum, state):
    P, Q, Qb = state.P.astype(np.float32), state.Q.astype(np.float32), state.Qb.astype(np.float32).reshape(-1, 1)
    o = (orc.OracleWARP if kind == "warp" else orc.OracleBPRMF)()
    assert o.init(H.write_opt(opt))
    o.initialize_model(P, Q, Qb, csr.nnz)
    if cum is not None:
        o.set_cumulative_table(cum, csr.num_items)
    o.set_modes(**ORACLE_MODES)
    o.trace(True)
    o.launch_workers()
    return o, (P, Q, Qb)


# ---------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------
def test_pattern_holds_every_run_it_was_built_for():
    case = _case("pattern")
    csr, C = case["csr"], case["C"]
    assert C == 256 and csr.num_users == 2 * C + 9 and csr.num_items == 32 and csr.nnz < 3000
    seen = dict(case["seen"])
    ds = sc.BPR_DESIGNS[0]
    assert ds["nn"] == 2
    opt = bpr_opt(**sc.bpr_options(ds))
    u, pos, neg = rs.bpr_triples(csr, opt, 0, H.cum_table(csr, opt))
    seen.update(sc.seen_negative_list(neg, C, csr.num_items, 7))
    for d, rpw in ((20, 8), (40, 4), (100, 2), (200, 1), (320, 1), (520, 1)):
        seen["rpw %d at vdim %d: the user side ends on a lone row, the item side on a full wave" % (rpw, sc.vdim_of(d))] = \
            sc.rpw_of(sc.vdim_of(d)) == rpw and csr.num_users % rpw == (1 if rpw > 1 else 0) and csr.num_items % rpw == 0
    assert all(seen.values()), [k for k, v in seen.items() if not v]


def test_pattern_wide_has_more_chunks_than_compute_units():
    case = _case("pattern_wide")
    assert all(case["seen"].values()), [k for k, v in case["seen"].items() if not v]


def test_warp_pattern_reaches_every_branch_of_the_trial_loop():
    case = _case("warp_pattern")
    csr, I = case["csr"], case["csr"].num_items
    per_user = np.diff(np.concatenate([[0], csr.indptr]))
    P, Q, Qb = sc.init_state(csr, sc.WARP_D, sc.SEEDS["warp"], sc.WARP_SCALE)
    st = rs.State(P, Q, Qb, np.float64)
    e = {mt: rs.epoch_gradients(st, csr, warp_opt(**sc.warp_options("dot", mt, thr)), 0, "warp") for mt, thr in sc.WARP_TRIALS[:6]}
    e20, e12 = e[20], e[12]
    rows = csr.rows()
    heavy = np.isin(rows, np.flatnonzero(per_user >= 0.9 * I))
    seen = dict(case["seen"])
    seen.update({
        "Phi = 0 is accepted and counted": bool((e20.accepted_mask & (e20.phi == 0)).any()),
        "k takes 1, 2, 3, 4, 5": all((e20.k == k).any() for k in (1, 2, 3, 4, 5)),
        "k of 8 or more": bool((e20.k >= 8).any()),
        "positives that run out of trials": bool((e12.k == 0).any() and (e20.k == 0).any()),
        "a violator that max_trials rejects (trial >= max_trials)": bool(((e12.k > 0) & ~e12.accepted_mask).any()),
        "the violating candidate beyond attempt 8 (past the pre-drawn candidates)": bool((e20.attempt[heavy] >= 8).any()),
        "the violating candidate beyond attempt 64 (the second 64-draw batch)": bool((e20.attempt[heavy] >= 64).any()),
        "max_trials 1 and 2 accept nothing, 3 and 4 only k = 1": e[1].accepted == 0 and e[2].accepted == 0 and e[3].accepted > 0
        and bool((e[3].k[e[3].accepted_mask] == 1).all() and (e[4].k[e[4].accepted_mask] == 1).all()),
    })
    assert all(seen.values()), [k for k, v in seen.items() if not v]
    lo = rs.epoch_gradients(st, csr, warp_opt(**sc.warp_options("dot", 12, -1e9)), 0, "warp")
    hi = rs.epoch_gradients(st, csr, warp_opt(**sc.warp_options("dot", 12, 1e9)), 0, "warp")
    assert lo.accepted == 0 and not lo.gP.any() and not lo.gQ.any() and not lo.cP.any() and not lo.cQ.any()
    assert hi.scored == csr.nnz and hi.accepted == csr.nnz and (hi.trial == 2).all()


# ---------------------------------------------------------------------------------------------
# the float32 restatement against the oracle, unsafe == 0 on every design
# ---------------------------------------------------------------------------------------------
def _two_epochs_against_oracle(oracle, kind, opt, csr, cum, state32, n_chunks, rtol, atol, epochs=2):
    adam = opt["optimizer"] == "adam"
    o, model = _oracle(oracle, kind, opt, csr, cum, state32)
    state, seen_trace = state32, 0
    names = [n for n in rs.STATE_NAMES[3:] if adam or not n.startswith("mom")]
    table = o.exp_table() if kind == "bpr" else None
    for epoch in range(epochs):
        e64 = rs.epoch_gradients(state.copy(np.float64), csr, opt, epoch, kind, cum=cum, table=table)
        assert e64.unsafe == 0 and e64.unsafe_2x == 0, (epoch, e64.unsafe, e64.unsafe_2x)
        e32 = rs.epoch_gradients(state, csr, opt, epoch, kind, cum=cum, table=table)
        before = o.stats()
        for a, b in H.chunks_of(csr, n_chunks):
            o.add_jobs(a, b, csr.indptr, H.chunk_arrays(csr, a, b)[0])
        tr = o.get_trace()[seen_trace:]
        seen_trace += tr.shape[0]
        np.testing.assert_array_equal(tr, np.stack([e32.u, e32.pos, e32.neg], axis=1))
        np.testing.assert_array_equal(tr, np.stack([e64.u, e64.pos, e64.neg], axis=1))
        if kind == "warp":
            after = o.stats()
            assert (after["scored_negatives"] - before["scored_negatives"], after["updates"] - before["updates"]) == (e32.scored, e32.accepted) \
                == (e64.scored, e64.accepted)
        for n, g in (("gradP", e32.gP), ("gradQ", e32.gQ), ("gradQb", e32.gQb)):
            np.testing.assert_allclose(o.state(n).reshape(g.shape), g, rtol=rtol, atol=atol, err_msg=n)
        # the step from the ORACLE's float32 gradients (every stage starts both sides from the same float32 values, as on the device:
        # a first adagrad step is +-1 / (1 + FEPS / |g|), which carries an ulp of a cancelled g into the fourth digit)
        e32.gP, e32.gQ, e32.gQb = (o.state(n).reshape(g.shape) for n, g in (("gradP", e32.gP), ("gradQ", e32.gQ), ("gradQb", e32.gQb)))
        o.update_parameters()
        state = rs.step_state(state, e32, opt, kind)
        for n in names:
            np.testing.assert_allclose(o.state(n).reshape(getattr(state, n).shape), getattr(state, n), rtol=rtol, atol=atol, err_msg="%s epoch %d" % (n, epoch))
        for n, a in zip(("P", "Q", "Qb"), model):
            np.testing.assert_allclose(a.reshape(getattr(state, n).shape), getattr(state, n), rtol=rtol, atol=atol, err_msg=n)
        state = rs.State(*model, np.float32, epoch + 1, **{n: o.state(n) for n in names})
    o.join()


@pytest.mark.parametrize("ds", sc.BPR_DESIGNS, ids=lambda ds: ds["name"])
def test_bpr_restatement_matches_oracle_and_no_triple_is_unsafe(oracle, ds):
    csr = _case(ds["case"])["csr"]
    opt = bpr_opt(**sc.bpr_options(ds))
    P, Q, Qb = sc.design_state(ds, csr)
    _two_epochs_against_oracle(oracle, "bpr", opt, csr, H.cum_table(csr, opt), rs.State(P, Q, Qb, np.float32), ds["n_chunks"], 2e-5, 2e-7, ds["epochs"])


@pytest.mark.parametrize("max_trials,threshold", sc.WARP_TRIALS)
@pytest.mark.parametrize("score_func", ["dot", "l2"])
def test_warp_restatement_matches_oracle_and_no_decision_is_unsafe(oracle, score_func, max_trials, threshold):
    csr = _case("warp_pattern")["csr"]
    opt = warp_opt(**sc.warp_options(score_func, max_trials, threshold))
    P, Q, Qb = sc.init_state(csr, sc.WARP_D, sc.SEEDS["warp"], sc.WARP_SCALE)
    _two_epochs_against_oracle(oracle, "warp", opt, csr, None, rs.State(P, Q, Qb, np.float32), 2, 3e-5, 3e-7)


# ---------------------------------------------------------------------------------------------
# the planted defects
# ---------------------------------------------------------------------------------------------
def _gradient_stage_rejects(oracle, kind, opt, csr, cum, state32, defect, chunk, hardware_order=False):
    """Epoch 1 (it starts from the step epoch 0 left in grad): does the stage bound, with the oracle as the envelope, reject the
    float32 run that carries `defect`?  Returns (rejected, worst ratio to the bound)."""
    o, _ = _oracle(oracle, kind, opt, csr, cum, state32)
    o.add_jobs(0, csr.num_users, csr.indptr, csr.keys)
    o.update_parameters()
    # both from the oracle's float32 state
    adam = opt["optimizer"] == "adam"
    s1 = rs.State(o._keep["P"], o._keep["Q"], o._keep["Qb"], np.float32, 1,
                  **{n: o.state(n) for n in rs.STATE_NAMES[3:] if adam or not n.startswith("mom")})
    table = o.exp_table() if kind == "bpr" else None
    e64 = rs.epoch_gradients(s1.copy(np.float64), csr, opt, 1, kind, cum=cum, table=table)
    bad = rs.epoch_gradients(s1, csr, opt, 1, kind, cum=cum, defect=defect, chunk=chunk, table=table)
    o.add_jobs(0, csr.num_users, csr.indptr, csr.keys)
    worst, rejected = 0.0, False
    for n, g, g64, S, N in (("gradP", bad.gP, e64.gP, e64.S_P, e64.N_P), ("gradQ", bad.gQ, e64.gQ, e64.S_Q, e64.N_Q),
                            ("gradQb", bad.gQb, e64.gQb, e64.S_b, e64.N_b)):
        b = rs.stage_bound(rs.row_err(o.state(n).reshape(g64.shape), g64, S).max(), N, hardware_order)
        worst = max(worst, (rs.row_err(g, g64, S) / b).max())
    rejected = worst > 1 or not np.array_equal(bad.cP, e64.cP) or not np.array_equal(bad.cQ, e64.cQ)
    if kind == "warp":
        rejected = rejected or (bad.scored, bad.accepted) != (e64.scored, e64.accepted)
    o.join()
    return rejected, worst


def _step_stage_rejects(kind, optimizer, vdim, use_bias, defect):
    """The drawn inputs of test_sgd_optimizer_gpu.py (sgd_cases.step_rng / draw_step_inputs: the same arrays), first and second call: does the elementwise bound, with the clean float32 run
    as the envelope, reject the float32 run that carries `defect`?"""
    warp, d, rpw = kind == "warp", vdim - 5, sc.rpw_of(vdim)
    opt = dict(warp_opt(d=d) if warp else bpr_opt(d=d, use_bias=use_bias, reg_b=0.03), optimizer=optimizer, per_coordinate_normalize=True, lr=0.05)
    opt["use_bias"] = bool(opt.get("use_bias", False))
    rng, rows = sc.step_rng(kind, optimizer, vdim), sc.step_rows(vdim)
    calls = [{s: sc.draw_step_inputs(rng, rows[s], d, warp) for s in "PQ"}]             # the device file's draws, in its order
    calls.append({s: sc.draw_step_inputs(rng, rows[s], d, warp, calls[0][s][5]) for s in "PQ"})
    worst = 0.0
    for side in "PQ":
        X, Xb = calls[0][side][:2]
        m, v = np.zeros_like(X), np.zeros_like(X)
        for call in range(2):
            _, _, g, gb, cnt, _ = calls[call][side]
            for bias, (x_, g_) in ((False, (X, g)), (True, (Xb, gb))):
                m_, v_ = (m, v) if not bias else (np.zeros(rows[side], np.float32), np.zeros(rows[side], np.float32))
                args = lambda dt: (x_.astype(dt), g_.astype(dt), m_.astype(dt) if optimizer == "adam" else None, v_.astype(dt), cnt,  # noqa: E731
                                   opt.get("reg_b", 0.0) if bias else opt["reg_u"], opt, call)
                w64 = rs.optimizer_step(*args(np.float64), project=warp and not bias, bias=bias)
                w32 = rs.optimizer_step(*args(np.float32), project=warp and not bias, bias=bias)
                bad = rs.optimizer_step(*args(np.float32), project=warp and not bias, bias=bias, defect=defect, rpw=rpw)
                for a64, a32, ab in zip(w64, w32, bad):
                    if a64 is not None:
                        with np.errstate(over="ignore", invalid="ignore"):
                            worst = max(worst, rs.elem_err(ab, a64).max() / rs.bound(rs.elem_err(a32, a64).max()))
                if not bias:
                    X, _, m, v = w32
                    m = np.zeros_like(X) if m is None else m
    return worst > 1, worst


GRADIENT_DEFECTS = {   # defect -> (kind, what to change in the design's options)
    "drop_incidence_at_chunk_end": ("bpr", {}), "second_flush_overwrites": ("bpr", {}), "count_pos_per_slot": ("bpr", {}),
    "count_skips_unupdated_list": ("bpr", dict(update_j=False)), "grad_rezeroed": ("bpr", {}), "gradq_row_scale": ("bpr", {}),
    "phi_trial_off_by_one": ("warp", {}), "phi_zero_rejected": ("warp", {}), "row_term_once_per_run": ("warp", {}),
}
STEP_DEFECTS = {       # defect -> (kind, optimizer, vdim, use_bias)
    "bias_not_divided_without_use_bias": ("bpr", "adam", 32, False), "feps_inside_sqrt": ("bpr", "adagrad", 64, True),
    "beta2_from_beta2": ("bpr", "adam", 96, True), "zero_count_divides": ("bpr", "adagrad", 128, True),
    "project_before_step": ("warp", "adagrad", 288, False), "last_row_of_wave_skipped": ("bpr", "adagrad", 32, True),
}


def _final_model_relerr(kind, opt, csr, cum, state32, defect):
    clean, _ = rs.train(state32, csr, opt, kind, 3, cum=cum)
    bad, _ = rs.train(state32, csr, opt, kind, 3, cum=cum, defect=defect)
    if not (np.isfinite(bad.P).all() and np.isfinite(bad.Q).all()):
        return float("inf")
    return max(H.relerr(bad.P, clean.P), H.relerr(bad.Q, clean.Q))


def _defect_setup(kind, change):
    if kind == "warp":
        csr = _case("warp_pattern")["csr"]
        opt = warp_opt(**dict(sc.warp_options("dot", 20, 0.0), num_iters=3, **change))
        P, Q, Qb = sc.init_state(csr, sc.WARP_D, sc.SEEDS["warp"], sc.WARP_SCALE)
        return csr, opt, None, rs.State(P, Q, Qb, np.float32)
    ds = sc.BPR_DESIGNS[0]
    csr = _case(ds["case"])["csr"]
    opt = bpr_opt(**dict(sc.bpr_options(ds), num_iters=3, **change))
    P, Q, Qb = sc.design_state(ds, csr)
    return csr, opt, H.cum_table(csr, opt), rs.State(P, Q, Qb, np.float32)


def test_every_defect_is_named_once():
    assert sorted(list(GRADIENT_DEFECTS) + list(STEP_DEFECTS)) == sorted(rs.DEFECTS)


@pytest.mark.parametrize("defect", sorted(GRADIENT_DEFECTS))
def test_gradient_stage_rejects_defect(oracle, defect):
    kind, change = GRADIENT_DEFECTS[defect]
    csr, opt, cum, st = _defect_setup(kind, change)
    clean_rejected, clean_worst = _gradient_stage_rejects(oracle, kind, opt, csr, cum, st, None, 256)
    rejected, worst = _gradient_stage_rejects(oracle, kind, opt, csr, cum, st, defect, sc.gather_chunk())
    rejected_hw, worst_hw = _gradient_stage_rejects(oracle, kind, opt, csr, cum, st, defect, sc.gather_chunk(), hardware_order=True)
    end_to_end = _final_model_relerr(kind, opt, csr, cum, st, defect)
    print("%-34s stage: %8.1f x the bound, %8.1f x with the order term of the per-triple-atomic designs (clean float32 run %.2f x)   "
          "final model after 3 epochs: relerr %.3e" % (defect, worst, worst_hw, clean_worst, end_to_end))
    assert not clean_rejected and clean_worst <= 1
    assert rejected and rejected_hw


@pytest.mark.parametrize("defect", sorted(STEP_DEFECTS))
def test_step_stage_rejects_defect(defect):
    rejected, worst = _step_stage_rejects(*STEP_DEFECTS[defect], defect)
    clean_rejected, clean_worst = _step_stage_rejects(*STEP_DEFECTS[defect], None)
    csr, opt, cum, st = _defect_setup(STEP_DEFECTS[defect][0], dict(optimizer=STEP_DEFECTS[defect][1]))
    end_to_end = _final_model_relerr(STEP_DEFECTS[defect][0], opt, csr, cum, st, defect)
    print("%-34s stage: %8.1f x the bound (clean float32 run %.2f x)   final model after 3 epochs: relerr %.3e" % (defect, worst, clean_worst, end_to_end))
    assert not clean_rejected
    assert rejected


@pytest.mark.parametrize("optimizer", ["adagrad", "adam"])
def test_gradq_row_scale_is_invisible_end_to_end(optimizer):
    """The reason this file exists: with reg = 0 the optimizer cancels a per-row scale of the gradient."""
    csr, opt, cum, st = _defect_setup("bpr", dict(optimizer=optimizer, reg_u=0.0, reg_i=0.0, reg_j=0.0, reg_b=0.0, per_coordinate_normalize=False))
    hidden = _final_model_relerr("bpr", opt, csr, cum, st, "gradq_row_scale")
    csr, opt, cum, st = _defect_setup("bpr", dict(optimizer=optimizer, per_coordinate_normalize=False))
    shown = _final_model_relerr("bpr", opt, csr, cum, st, "gradq_row_scale")
    print("gradq_row_scale under %s: relerr of the model after 3 epochs %.3e with reg = 0, %.3e with reg = 0.025" % (optimizer, hidden, shown))
    assert hidden < 1e-4
