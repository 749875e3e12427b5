"""The yardstick of test_bpr_dual_gpu.py, held on the CPU: the closed-slice matrices of walk_cases.py are what they claim to be under
the library's own plan, the float32 replay of ref_walk.py is the oracle's arithmetic, the reference alone meets the cap every design
needs (enough clean and safe components of every kind), and five planted defects of the walk sit far above the device bound."""
import numpy as np
import pytest

import ref_walk as R
import walk_cases as W

NNS = (1, 3)


@pytest.mark.parametrize("variant", sorted(W.VARIANTS))
@pytest.mark.parametrize("nn", NNS)
def test_every_slice_is_one_component(variant, nn):
    """For 1, 2, 4 and 8 queues: the slices the library's plan cuts (helpers.item_major_order over bfh_bpr_item_major_plan) are the
    components, entry for entry and in `walk_positions` order; the tail is the one partial slice."""
    case = W.case(variant, nn, 1 << 19)
    assert case.csr.num_items == 1 << 19 and case.E == 64 // nn
    for nq in (1, 2, 4, 8):
        sl = W.slices_of(case, nq)
        assert len(sl) == case.n_comp
        got = set()
        for x, _, pos in sl:
            c = int(case.comp[pos[0]])
            assert np.array_equal(pos, W.walk_positions(case, c)), (nq, c)
            assert x == case.residue[c] % nq
            assert len(pos) == case.E or case.kind[c] == "tail"
            got.add(c)
        assert len(got) == case.n_comp
    # what the kinds are there for
    csr = case.csr
    deg = np.bincount(csr.rows(), minlength=csr.num_users)
    cnt = np.bincount(csr.keys, minlength=csr.num_items)
    for c, kind in enumerate(case.kind):
        if kind == "run":
            assert cnt[case.items[c]].tolist() == [case.E] and set(deg[case.users[c]]) == {1}
        if kind == "heavy_user":
            assert deg[case.users[c]].tolist() == [case.E]
        if kind == "two_users":
            assert len(case.users[c]) == 2 and deg[case.users[c]].min() >= case.E // 2
    assert (deg == 0).sum() >= 8                      # users nobody touches


@pytest.mark.parametrize("nn", NNS)
def test_half_wave_pairings_over_the_designs(nn):
    """Over the variants and segment cuts the device file runs with the two-triples walk at 8 queues: a partial slice in half 0,
    one in half 1, an idle half 1 (odd ticket count) and two full slices."""
    seen = {}
    for dsg in W.DESIGNS:
        if dsg["nn"] != nn or dsg["modes"].get("im_dual", 1) != 1:
            continue
        case = R.design_case(dsg)
        n = case.csr.nnz * nn
        sync = n // 3 if dsg["modes"].get("xcd_sync_updates") == "third" else 1 << 23
        got, segments = W.pairings(case, 8, sync)
        assert segments == dsg["expect"].get("segments", 1)
        for k, v in got.items():
            seen[k] = seen.get(k, False) or v
    print(nn, seen)
    assert len(seen) == 4 and all(seen.values()), seen


@pytest.mark.parametrize("design", W.DESIGNS, ids=lambda d: d["name"])
def test_replay_is_the_oracle_and_the_cap_holds(oracle, design):
    """Every component replayed alone in float32 (`ref_numpy.bpr_sgd_step`, walk order) against the oracle applying the same
    triples to the whole model (`apply_triples`): bit for bit wherever the oracle's compiler contracts nothing, else to a few ulp
    (the measured distance is printed).  Then the cap: at least 3 clean and safe components of every kind, the tail, and 60 % of all."""
    case, opt, negs, model, clean, refs = R.judge(oracle, design)
    us = R.usable(clean, refs)
    csr, rows = case.csr, case.csr.rows()
    worst = 0.0
    for c in np.flatnonzero(clean):
        r32 = refs[c][0]
        o = oracle.OracleBPRMF()
        import helpers as H
        import os
        path = H.write_opt(opt)
        assert o.init(path)
        os.unlink(path)
        P, Q, Qb = (np.ascontiguousarray(model[0][r32.users]), np.ascontiguousarray(model[1][r32.items]), np.ascontiguousarray(model[2][r32.items]))
        o.initialize_model(P, Q, Qb, csr.nnz)
        pos = W.walk_positions(case, c)
        ul = np.searchsorted(r32.users, rows[pos]).astype(np.int32)
        il = np.searchsorted(r32.items, csr.keys[pos]).astype(np.int32)
        for e in range(negs.shape[0]):
            jl = np.searchsorted(r32.items, negs[e, pos]).astype(np.int32)
            o.apply_triples(np.repeat(ul, case.nn), np.repeat(il, case.nn), np.ascontiguousarray(jl.reshape(-1)), opt["lr"])
        for a, b in ((P, r32.P), (Q, r32.Q), (Qb, r32.Qb)):
            worst = max(worst, H.relerr(a, b))
    kinds = {k: int(sum(us[c] for c in range(case.n_comp) if case.kind[c] == k)) for k in sorted(set(case.kind))}
    margin = min(refs[c][1].worst for c in np.flatnonzero(us))
    print("%s: replay vs oracle %.2e; clean %d, clean and safe %d of %d %s; nearest table edge %.1f x the float32 dot bound"
          % (design["name"], worst, clean.sum(), us.sum(), case.n_comp, kinds, margin))
    assert worst <= 2e-6, worst
    assert all(v >= 3 for k, v in kinds.items() if k != "tail") and kinds["tail"] == 1, kinds
    assert us.mean() >= 0.60, us.mean()


@pytest.mark.parametrize("name", sorted(R.DEFECTS))
def test_planted_defects_sit_far_above_the_device_bound(oracle, name):
    """One arithmetic slip of the walk, planted in the float32 replay of one component: a step of a 64-run lost, a returning user
    given its row from before its last step, the step behind a flush missing from the item row, the bias of the other half's item,
    a flush applied twice -- each at least 10x over the bound the device rows are held to."""
    design = W.BY_NAME["d128"]
    case, opt, negs, model, clean, refs = R.judge(oracle, design)
    kind, step = R.DEFECTS[name]
    us = R.usable(clean, refs)
    c = next(c for c in range(case.n_comp) if us[c] and case.kind[c] == kind)
    bad = R.replay(case, negs, c, model, opt, R.ref_table(oracle), np.float32, defect=(name, step))
    r = R.ratio((bad.P, bad.Q, bad.Qb), *refs[c])
    own = R.ratio((refs[c][0].P, refs[c][0].Q, refs[c][0].Qb), *refs[c])
    print("%s: %.0f x the bound (the replay itself: %.2f)" % (name, r, own))
    assert own <= 0.4 and r >= 10.0, (r, own)
