"""The stage between `add_jobs` and `update_parameters` of the gradient-accumulating SGD paths (adam / adagrad BPRMF, WARP) against the
float64 run of ref_sgd.epoch_gradients: gradP, gradQ, gradQb row by row, countP / countQ and the WARP statistics exactly.

Each epoch is its own comparison from ONE float32 state: the device's P, Q, Qb, grad*, mom*, vel* are read at the start of the epoch,
the yardstick and a fresh oracle (epoch counter advanced, state written through `state_view`) are loaded with them, all three run the
epoch's add_jobs, and a device row must satisfy
    max_k |dev - f64| / S[row]  <=  2.5 x (the oracle's worst row) + 4 x 2^-23                                    (ref_sgd.stage_bound)
-- plus order_term(terms of the row) on the designs whose every term is its own atomic add (accum_two_pass = 0, update_triples): a
float32 sum in hardware order is another draw of the random walk of its roundings than the oracle's loop order, and a new one in
every run; `adam-d20-nn3-atomic-seed4` is the design on which gradQb[3], 1,566 same-sign terms, lands at 3.6 ... 4.0 x the oracle's
draw (profiles/sgd_accumulate_parity.txt) --
while a row that received no term keeps its start bits.  The second epoch starts from the step the first left in grad (Q-6).
`unsafe == 0` is asserted on every device state: no triple's table cell, no WARP decision depends on float32 rounding.

Kernels and the designs that reach their branches (sgd_cases.py has the run lengths of `pattern`):
  bpr_update_kernel<.., SGD=false>   every BPR design; two_pass = 0: one atomic row add per triple and item row; `inject`: update_triples
  grad_gather_kernel<K, UN>          d 20 / 200 / 320 / 520 = K 1 / 4 / 8 / 16, UN 8 / 8 / 4 / 2; runs cut by one and by two chunk
                                     bounds, one-incidence runs on either side of a bound, the 37-incidence last chunk; n_chunks = 3 and
                                     a resident matrix (the kept positive list); `wide`: more chunks than waves (gather_waves_per_cu = 1)
  incidence_count_kernel             update_i = False / update_j = False: the list is counted, not gathered (Q-9)
  fill_rows_kernel                   every non-injected design (the row id of every staged entry)
  warp_presample_kernel, warp_update_kernel   warp_presample 0 / 4 / 8, max_trials 1 ... 20, thresholds -1e9 / +1e9, users that have seen
                                     all but one or two items (Phi = 0) and 90 % (candidates beyond the pre-drawn attempts), dot and l2"""
import numpy as np
import pytest

from conftest import bpr_opt, warp_opt
import helpers as H
import ref_sgd as rs
import sgd_cases as sc

pytestmark = pytest.mark.gpu

ORACLE_MODES = dict(sampler="counter", pos_order="csr", inline=True)
_cases = {}


def _case(name):
    if name not in _cases:
        _cases[name] = sc.make_case(name)
    return _cases[name]


def _device_state(obj, P, Q, Qb, d, adam, iters):
    U, I, vdim = P.shape[0], Q.shape[0], P.shape[1]
    st = {}
    for n in rs.STATE_NAMES[3:]:
        if n.startswith("mom") and not adam:
            continue
        rows = U if n.endswith("P") else I
        t = obj.device_tensor(n, (rows,) if n.endswith("Qb") else (rows, vdim)).cpu().numpy().copy()
        if t.ndim == 2:
            assert np.all(t[:, d:] == 0), (n, "padding columns")
            t = t[:, :d]
        st[n] = t
    return rs.State(P[:, :d], Q[:, :d], Qb, np.float32, iters, **st)


def _loaded_oracle(cls, opt, csr, cum, state, adam):
    """A fresh oracle brought to the device's epoch and float32 state."""
    P, Q, Qb = state.P.copy(), state.Q.copy(), state.Qb.reshape(-1, 1).copy()
    o = cls()
    assert o.init(H.write_opt(opt))
    o.initialize_model(P, Q, Qb, csr.nnz)
    if cum is not None:
        o.set_cumulative_table(cum, csr.num_items)
    o.set_modes(**ORACLE_MODES)
    o.launch_workers()
    for _ in range(state.iters):
        o.update_parameters()
    P[:], Q[:], Qb[:] = state.P, state.Q, state.Qb.reshape(-1, 1)
    for n in rs.STATE_NAMES[3:]:
        if n.startswith("mom") and not adam:
            continue
        o.state_view(n)[:] = getattr(state, n).reshape(-1)
    return o, (P, Q, Qb)


def _read_stage(obj, U, I, d, vdim):
    out = {}
    for n, rows in (("gradP", U), ("gradQ", I)):
        t = obj.device_tensor(n, (rows, vdim)).cpu().numpy().copy()
        assert np.all(t[:, d:] == 0), (n, "padding columns")
        out[n] = t[:, :d]
    out["gradQb"] = obj.device_tensor("gradQb", (I,)).cpu().numpy().copy()
    out["countP"] = obj.device_tensor("countP", (U,), dtype="int32").cpu().numpy().copy()
    out["countQ"] = obj.device_tensor("countQ", (I,), dtype="int32").cpu().numpy().copy()
    return out


def _compare(tag, dev, o, e64, start, report, hardware_order=False):
    for n, g64, S, T, N in (("gradP", e64.gP, e64.S_P, e64.T_P, e64.N_P), ("gradQ", e64.gQ, e64.S_Q, e64.T_Q, e64.N_Q),
                            ("gradQb", e64.gQb, e64.S_b, e64.T_b, e64.N_b)):
        orc = o.state(n).reshape(g64.shape)
        e_o, e_d = rs.row_err(orc, g64, S), rs.row_err(dev[n], g64, S)
        b = rs.stage_bound(e_o.max(), N, hardware_order)
        w = int((e_d / b).argmax())
        report.append("%-44s %-6s dev %.3e  oracle %.3e  ratio %.2f | worst row %d (%d terms): dev %.3e  bound %.3e = %.2f x"
                      % (tag, n, e_d.max(), e_o.max(), e_d.max() / max(e_o.max(), rs.ULP32), w, N[w], e_d[w], b[w], e_d[w] / b[w]))
        assert np.isfinite(dev[n]).all(), (tag, n)
        assert (e_d <= b).all(), (tag, n, w, float(e_d[w]), float(b[w]), float(e_o.max()))
        assert rs.untouched(dev[n], getattr(start, n), T), (tag, n, "a row that received nothing changed")
    np.testing.assert_array_equal(dev["countP"], e64.cP, err_msg=tag)
    np.testing.assert_array_equal(dev["countQ"], e64.cQ, err_msg=tag)


def _prepare(cls, opt, csr, P, Q, Qb, modes, n_chunks, resident, cum):
    obj = cls()
    assert obj.init(H.write_opt(dict(opt, accelerator=True)))
    for k, v in modes.items():
        obj.set_mode(k, v)
    obj.initialize_model(P, Q, Qb, csr.nnz)
    if cum is not None:
        obj.set_cumulative_table(cum, csr.num_items)
    sizes = [int(csr.indptr[b - 1]) - (0 if a == 0 else int(csr.indptr[a - 1])) for a, b in H.chunks_of(csr, n_chunks)]
    obj.set_placeholder(csr.indptr, max(sizes) + 1)
    obj.initialize_model(P, Q, Qb, csr.nnz, True)
    if cum is not None:
        obj.set_cumulative_table(cum, csr.num_items)
    if resident:
        obj.set_resident_csr(csr.indptr, csr.keys)
    return obj


def _add_jobs(obj, csr, n_chunks, resident=False):
    for a, b in H.chunks_of(csr, n_chunks):
        keys, _ = H.chunk_arrays(csr, a, b)
        obj.add_jobs(a, b, csr.indptr, None if resident else keys)


@pytest.mark.parametrize("ds", sc.BPR_DESIGNS, ids=lambda ds: ds["name"])
def test_bpr_gradients_and_counts(oracle, ds):
    from buffalo_amd.backend import CyBPR
    case = _case(ds["case"])
    csr, d = case["csr"], ds["d"]
    vdim, adam = sc.vdim_of(d), ds["optimizer"] == "adam"
    opt = bpr_opt(**sc.bpr_options(ds))
    cum = H.cum_table(csr, opt)
    if ds["gather_waves_per_cu"]:
        import torch
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        assert -(-csr.nnz // case["C"]) > cus * ds["gather_waves_per_cu"], "the gather's grid-stride loop would not take a second chunk"
    P0, Q0, Qb = sc.design_state(ds, csr)
    P, Q = H.pad(P0, vdim), H.pad(Q0, vdim)
    modes = dict(chunk=64, accum_two_pass=ds["two_pass"])
    if ds["gather_waves_per_cu"]:
        modes["gather_waves_per_cu"] = ds["gather_waves_per_cu"]
    obj = _prepare(CyBPR, opt, csr, P, Q, Qb, modes, ds["n_chunks"], ds["resident"], cum)
    report = []
    for epoch in range(ds["epochs"]):
        obj.set_mode("epoch", epoch)
        start = _device_state(obj, P, Q, Qb, d, adam, epoch)
        triples = rs.bpr_triples(csr, opt, epoch, cum) if ds["inject"] else None
        o, _ = _loaded_oracle(oracle.OracleBPRMF, opt, csr, cum, start, adam)
        # the sigmoid table is the oracle's: both backends fill theirs with the host's expf (bpr.cc:57-63)
        e64 = rs.epoch_gradients(start.copy(np.float64), csr, opt, epoch, "bpr", cum=cum, triples=triples, table=o.exp_table())
        assert e64.unsafe == 0, (ds["name"], epoch, e64.unsafe)
        _add_jobs(o, csr, ds["n_chunks"])
        if ds["inject"]:
            u, pos, neg = (np.ascontiguousarray(a, np.int32) for a in triples)
            obj.update_triples(u, pos, neg, opt["lr"])
        else:
            _add_jobs(obj, csr, ds["n_chunks"], ds["resident"])
        dev = _read_stage(obj, csr.num_users, csr.num_items, d, vdim)
        _compare("%s epoch %d" % (ds["name"], epoch), dev, o, e64, start, report, sc.hardware_order(ds))
        # the item nobody has and nobody draws: no count, no gradient (epoch 1: `untouched` held the bits of the step left there) ...
        assert int(e64.cQ[7]) == 0 and e64.T_Q[7] == 0 and int(dev["countQ"][7]) == 0
        if epoch == 0:
            assert not dev["gradQ"][7].any() and dev["gradQb"][7] == 0
        o.join()
        q7 = Q[7].view(np.uint32).copy()                                   # all vdim columns
        obj.update_parameters()                                            # copies the model back into P, Q, Qb
        if ds["reg"] == 0.0:                                               # ... and with reg_i = 0 its Q row keeps its bits through the step
            np.testing.assert_array_equal(Q[7].view(np.uint32), q7, err_msg="%s epoch %d: Q[7]" % (ds["name"], epoch))
            dq7 = obj.device_tensor("Q", (csr.num_items, vdim))[7].cpu().numpy()
            np.testing.assert_array_equal(dq7.view(np.uint32), q7)
    print("\n".join(report))


@pytest.mark.parametrize("max_trials,threshold", sc.WARP_TRIALS)
@pytest.mark.parametrize("presample", [0, 4, 8])
@pytest.mark.parametrize("score_func", ["dot", "l2"])
def test_warp_gradients_counts_and_statistics(oracle, score_func, presample, max_trials, threshold):
    from buffalo_amd.backend import CyWARP
    case = _case("warp_pattern")
    csr, d = case["csr"], sc.WARP_D
    vdim = sc.vdim_of(d)
    opt = warp_opt(**sc.warp_options(score_func, max_trials, threshold))
    P0, Q0, Qb = sc.init_state(csr, d, sc.SEEDS["warp"], sc.WARP_SCALE)
    P, Q = H.pad(P0, vdim), H.pad(Q0, vdim)
    obj = _prepare(CyWARP, opt, csr, P, Q, Qb, dict(chunk=64, warp_presample=presample), 2, False, None)
    report = []
    for epoch in range(2):
        obj.set_mode("epoch", epoch)
        obj.reset_stats()
        start = _device_state(obj, P, Q, Qb, d, False, epoch)
        e64 = rs.epoch_gradients(start.copy(np.float64), csr, opt, epoch, "warp")
        assert e64.unsafe == 0, (epoch, e64.unsafe)
        o, _ = _loaded_oracle(oracle.OracleWARP, opt, csr, None, start, False)
        _add_jobs(o, csr, 2)
        _add_jobs(obj, csr, 2)
        dev = _read_stage(obj, csr.num_users, csr.num_items, d, vdim)
        st, so = obj.stats(), o.stats()
        assert (st["scored_negatives"], st["accepted"]) == (e64.scored, e64.accepted) == (so["scored_negatives"], so["updates"])
        if threshold == -1e9:        # nothing violates: no gradient (the rows keep their bits: `untouched`), no count
            assert e64.accepted == 0 and not dev["countP"].any() and not dev["countQ"].any()
        if threshold == 1e9:
            assert e64.scored == csr.nnz and e64.accepted == (csr.nnz if 2 < max_trials else 0)
        _compare("warp-%s-S%d-T%d-%g epoch %d" % (score_func, presample, max_trials, threshold, epoch), dev, o, e64, start, report)
        o.join()
        obj.update_parameters()
    print("\n".join(report))
