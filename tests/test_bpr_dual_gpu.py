"""The two-triples item-major walk (bpr_item_major_dual_kernel, the kernel bench.py times) IS the sequential replay wherever a slice
is closed.

On the matrices of walk_cases.py every slice is a component no other slice shares a row with, so under many waves, any placement and
any path (plain stores, atomics, replica + delta merge, the drain launch) each component has ONE possible result: its own triples
replayed in walk order.  No test hook is set -- this is the throughput kernel as bench.py launches it, `im_dual` = 1 forced because
the size rule would pick the one-triple walk on so few users.  The bound, per row of P, of Q and per entry of Qb of every clean and
safe component (ref_walk.py):

    err(hip, f64) <= 2.5 x err(float32 replay, f64) + 4 x 2^-23 x max|f64 row|

What the designs are there for (walk_cases.DESIGNS): NK = 1 .. 4 and the guarded instantiation (`-generic`), nn = 3 (the carry of a
user over the slots of an entry), bias off, `update_i` off (the refresh branch of the mid-run flush), `update_j` off, flush intervals
1 / between / 64 on the `run` items (read back), nothing hot / everything on atomics / the heavy users alone (read back), three merge
segments, two epochs (cached regrouping, side-stream draw, "im_presample" 2 and 1), and the one-triple kernels with and without
prefetch at d = 128 / 200 under many waves.  Measured ratios, flag mixes and drained triples: profiles/bpr_dual_parity.txt.

Measured on one MI355X: worst ratio 0.33 .. 0.40 on all 30 designs -- the device rows are the float32 replay's almost bit for bit.
Two things the replay has to state as the walk does, or single entries of Qb that a step carries through zero miss the bound by up
to 564x (both in ref_walk.py): the sigmoid table is the reference's own (std::exp; numpy's differs in the last bit of 361 cells), and
a bias reaches memory as b + fl(sum of the steps since the last flush), in the flush intervals read back from the device."""
import numpy as np
import pytest

import helpers as H
import ref_walk as R
import walk_cases as W

pytestmark = pytest.mark.gpu


def _modes(design, case, num_cus):
    m = dict(W.BASE_MODES)
    m.update(design["modes"])
    if m.get("xcd_sync_updates") == "third":
        m["xcd_sync_updates"] = case.csr.nnz * case.nn // 3
    if m["xcd_hot_tau"] == "heavy":
        m["xcd_hot_tau"] = W.heavy_tau(case, num_cus)
    if design["expect"].get("hot") == "all":
        m["waves_per_cu"] = 64       # a uniform draw from this catalogue reaches the smallest tau (1 permille) only with more rows in flight
    return m


@pytest.mark.parametrize("design", W.DESIGNS, ids=lambda d: d["name"])
def test_closed_slices_are_the_sequential_replay(oracle, design):
    import torch
    from buffalo_amd.backend import CyBPR
    case, opt, negs, model, clean, refs = R.judge(oracle, design)
    us = R.usable(clean, refs)
    csr, d, nn, epochs = case.csr, design["d"], case.nn, design["epochs"]
    vdim, n = W.vdim_of(d), csr.nnz * nn
    P0, Q0, Qb0 = (np.zeros((csr.num_users, vdim), np.float32), np.zeros((csr.num_items, vdim), np.float32), model[2].copy())
    P0[:, :d], Q0[:, :d] = model[0], model[1]
    P, Q, Qb = P0.copy(), Q0.copy(), Qb0.copy()
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    modes = _modes(design, case, num_cus)
    obj = H.run_hip_sgd(CyBPR, opt, csr, P, Q, Qb, epochs=epochs, modes=modes, resident=True)
    assert obj.stats()["samples"] == epochs * n
    flush = obj.device_tensor("im_flush_every").cpu().numpy()
    hot_u = obj.device_tensor("im_hot_user").cpu().numpy()
    hot_i = obj.device_tensor("im_hot_item").cpu().numpy()
    drained = int(obj.device_tensor("im_drained", (1,)).cpu().numpy()[0])
    assert flush.shape == (csr.num_items,) and hot_i.shape == (csr.num_items,) and hot_u.shape == (csr.num_users,)
    del obj

    # ---- the bound, component by component ----
    worst, worst_kind = 0.0, {}
    for c in np.flatnonzero(us):
        r64 = refs[c][1]
        # the float32 replay with the bias steps of a run reaching memory in the device's own groups (the flush intervals read back)
        r32 = R.replay(case, negs, c, model, opt, R.ref_table(oracle), np.float32, flush=flush)
        got = (P[r32.users][:, :d], Q[r32.items][:, :d], Qb[r32.items])
        r = R.ratio(got, r32, r64)
        worst_kind[case.kind[c]] = max(worst_kind.get(case.kind[c], 0.0), r)
        assert not np.array_equal(got[0], P0[r32.users][:, :d])            # something moved
    worst = max(worst_kind.values())
    run_items = np.concatenate([case.items[c] for c in range(case.n_comp) if case.kind[c] == "run"])
    heavy = np.concatenate([case.users[c] for c in range(case.n_comp) if case.kind[c] == "heavy_user"])
    active = np.unique(csr.rows())
    print("%s: worst ratio %.3f %s; %d of %d components compared; drained %d of %d triples in the last call; flush_every on run items %s, "
          "distinct %s; hot users %d of %d (heavy %d of %d), hot items %d; modes %s"
          % (design["name"], worst, {k: round(v, 3) for k, v in sorted(worst_kind.items())}, us.sum(), case.n_comp, drained, n,
             sorted(set(flush[run_items].tolist())), sorted(set(flush[np.unique(csr.keys)].tolist())), int((hot_u[active] == 1).sum()), active.size,
             int((hot_u[heavy] == 1).sum()), heavy.size, int(hot_i.sum()), {k: v for k, v in modes.items() if k not in W.BASE_MODES or W.BASE_MODES[k] != v}))
    assert worst <= 1.0, (worst, worst_kind)

    # ---- rows nobody touches keep their bits, pad columns stay 0 ----
    touched_i = np.zeros(csr.num_items, bool)
    touched_i[csr.keys] = True
    touched_i[negs.reshape(-1)] = True
    touched_u = np.zeros(csr.num_users, bool)
    touched_u[active] = True
    assert np.array_equal(P[~touched_u], P0[~touched_u]) and (~touched_u).sum() >= 8
    assert np.array_equal(Q[~touched_i], Q0[~touched_i]) and np.array_equal(Qb[~touched_i], Qb0[~touched_i])
    assert np.all(P[:, d:] == 0) and np.all(Q[:, d:] == 0) and np.isfinite(P).all() and np.isfinite(Q[touched_i]).all()

    # ---- the drain launch is the exception, and the flags show the mix the design is there for ----
    assert drained <= 0.25 * n, (drained, n)
    assert set(hot_u.tolist()) <= {0, 1}
    want = design["expect"]
    if want.get("flush") == "one":
        assert set(flush[run_items].tolist()) == {1}
    if want.get("flush") == "mid":
        assert all(1 < f < 64 for f in flush[run_items].tolist()), flush[run_items]
    if want.get("flush") == "64":
        assert set(flush[run_items].tolist()) == {64}
    if want.get("hot", "none") == "none":
        assert not hot_u.any() and not hot_i.any()
    if want.get("hot") == "all":
        assert (hot_u[active] == 1).all() and hot_i.all()
    if want.get("hot") == "heavy":
        assert np.array_equal(np.flatnonzero(hot_u == 1), np.sort(heavy)) and not hot_i.any()
