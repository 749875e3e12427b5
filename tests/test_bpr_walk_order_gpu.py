"""BPRMF item-major walk: per-triple metadata in walk order ("im_presample" = 2).

The walk gets an entry's user from beside the entry and computes the first draw of its negative itself; the CSR-order presampler only
records, in walk order, the triples whose first draw was rejected.  The triples walked are bit for bit those of the two older sources of
negatives ("im_presample" = 1: all of them pre-drawn at their nnz positions; 0: drawn inside the walk), so wherever the run is
deterministic (one wave, test hook "im_single_wave") traces and models are compared for EQUALITY, not under a tolerance."""
import os

import numpy as np
import pytest

from conftest import bpr_opt
import helpers as H

pytestmark = pytest.mark.gpu

DET = dict(sampler="counter", pos_order="csr", inline=True)


def _dense_case():
    """96 users x 40 items, degrees 8 .. 36, user 0 with 39 of the 40 items (its draws take many attempts): about 2,000 entries -- more
    than one slice per queue at 8 queues, the last one partial."""
    from buffalo_amd.synth import CSR
    U, I = 96, 40
    rng = np.random.default_rng(17)
    deg = rng.integers(8, 37, size=U)
    deg[0] = 39
    keys = np.concatenate([np.sort(rng.permutation(I)[:k]) for k in deg]).astype(np.int32)
    return CSR(U, I, np.cumsum(deg, dtype=np.int64), keys, np.ones(keys.shape[0], np.float32))


def _factors(csr, vdim, seed=1):
    rng = np.random.default_rng(seed)
    P = rng.normal(scale=0.3, size=(csr.num_users, vdim)).astype(np.float32)
    Q = rng.normal(scale=0.3, size=(csr.num_items, vdim)).astype(np.float32)
    Qb = rng.normal(scale=0.1, size=(csr.num_items, 1)).astype(np.float32)
    return P, Q, Qb


_first_draws = {}


def _first_draw_rejected(oracle, csr, nn, seed):
    """Per triple of epoch 0 (CSR order, pos * nn + slot): was the first draw one of the user's own items?  The draw is replayed on the
    host with the oracle's counter sampler; the oracle's own epoch (same sampler) must agree with it wherever the first draw stands."""
    if (nn, seed) in _first_draws:
        return _first_draws[(nn, seed)]
    I = csr.num_items
    rows = csr.rows()
    beg = np.concatenate([[0], csr.indptr[:-1]])
    cand = np.empty(csr.nnz * nn, np.int64)
    rej = np.empty(csr.nnz * nn, bool)
    for pos in range(csr.nnz):
        u = rows[pos]
        own = csr.keys[beg[u]:csr.indptr[u]]
        for slot in range(nn):
            o0 = oracle.counter_draw(seed, 0, pos, slot, 0, 0)[0]
            cand[pos * nn + slot] = (o0 * I) >> 32
            rej[pos * nn + slot] = cand[pos * nn + slot] in own
    opt = bpr_opt(d=8, lr=0.01, min_lr=0.01, num_iters=1, random_seed=seed, num_negative_samples=nn)
    P, Q, Qb = _factors(csr, 8)
    tr = H.run_oracle_sgd(oracle.OracleBPRMF, opt, csr, P, Q, Qb, epochs=1, modes=DET, trace=True).get_trace()
    assert len(tr) == csr.nnz * nn
    assert np.array_equal(tr[~rej, 2], cand[~rej]) and not np.any(tr[rej, 2] == cand[rej])
    _first_draws[(nn, seed)] = rej
    return rej


def _single_wave_run(csr, opt, vdim, nq, presample, epochs=2):
    """`epochs` epochs of one wave draining every queue in ticket order; returns the per-epoch traces and the model."""
    import torch
    from buffalo_amd.backend import CyBPR
    n = csr.nnz * opt["num_negative_samples"]
    P, Q, Qb = _factors(csr, vdim)
    obj = CyBPR()
    path = H.write_opt(dict(opt, accelerator=True))
    assert obj.init(path)
    os.unlink(path)
    for k, v in dict(hogwild_atomic=3, im_single_wave=1, im_force_queues=nq, im_trace=n, im_presample=presample, im_presample_ahead=1).items():
        obj.set_mode(k, v)
    obj.initialize_model(P, Q, Qb, csr.nnz, True)
    obj.set_cumulative_table(H.cum_table(csr, opt), csr.num_items)
    obj.set_resident_csr(csr.indptr, csr.keys)
    traces = []
    for _ in range(epochs):
        obj.add_jobs(0, csr.num_users, csr.indptr, None)
        obj.update_parameters()
        traces.append(obj.device_tensor("im_trace", (n,), dtype="int32").cpu().numpy().copy())
        torch.cuda.synchronize()
    obj.synchronize(True)
    assert obj.stats()["samples"] == epochs * n
    return traces, (P, Q, Qb)


@pytest.mark.parametrize("schedule", ["constant", "decaying"])
@pytest.mark.parametrize("nq", [1, 4, 8])
@pytest.mark.parametrize("d,nn", [(32, 1), (32, 3), (128, 1), (128, 3)])
def test_three_negative_sources_walk_the_same_triples(oracle, d, nn, nq, schedule):
    """Two epochs of a single wave (deterministic) with the negatives from the walk-order exceptions (2), the CSR-order array (1) and the
    draw inside the walk (0): identical traces, identical models.  The second epoch is served from the side-stream draw of the first;
    on the decaying schedule (lr 0.05 -> 0.0001 over two epochs) the learning rate cuts the items' entries into another number of runs
    in the second epoch, the regrouping changes under the speculation, and a walk-order draw written against the old one must be thrown
    away.  The matrix is dense enough that well over 10 % of the first draws are rejected: the exception path carries the result."""
    csr = _dense_case()
    assert 1900 <= csr.nnz <= 2300 and csr.nnz * nn > 8 * 64 * 2
    rej = _first_draw_rejected(oracle, csr, nn, 5)
    print("first draw rejected: %.1f %% of %d triples" % (100.0 * rej.mean(), rej.size))
    assert rej.mean() >= 0.10
    lr, min_lr = (0.05, 0.05) if schedule == "constant" else (0.05, 0.0001)
    opt = bpr_opt(d=d, lr=lr, min_lr=min_lr, num_iters=2, random_seed=5, num_negative_samples=nn)
    runs = {ps: _single_wave_run(csr, opt, d, nq, ps) for ps in (2, 1, 0)}
    t2, m2 = runs[2]
    assert len(set(t2[0].tolist())) > 10 and not np.array_equal(t2[0], t2[1])      # the trace was written, by both epochs
    for ps in (1, 0):
        t, m = runs[ps]
        for e in range(2):
            assert np.array_equal(t2[e], t[e]), (ps, e, int((t2[e] != t[e]).sum()))
        for a, b in zip(m2, m):
            assert np.array_equal(a, b), ps


@pytest.mark.parametrize("d,nn,epochs", [(128, 1, 1), (128, 1, 2), (96, 3, 1)])
def test_dual_kernel_walk_order_conflict_free(oracle, d, nn, epochs):
    """The two-triples walk with many waves on the conflict-free matrix of test_bpr_gpu.py::test_item_major_conflict_free (every user one
    positive, the positives distinct): a triple whose three rows no other triple touches has one possible result.  "im_presample" = 2
    against the sequential oracle and against "im_presample" = 1, both under that test's tolerance (1e-5) on those rows; the library
    itself checks that the device processed exactly `total` triples (partial_update raises otherwise)."""
    from buffalo_amd import synth
    from buffalo_amd.backend import CyBPR
    U, I = 3000, 60000
    rng = np.random.default_rng(5)
    keys = rng.permutation(I)[:U].astype(np.int32)
    csr = synth.CSR(U, I, np.arange(1, U + 1, dtype=np.int64), keys, np.ones(U, np.float32))
    opt = bpr_opt(d=d, lr=0.05, min_lr=0.05, num_iters=epochs, random_seed=11, num_negative_samples=nn)
    vdim = ((d + 31) // 32) * 32
    P0, Q0, Qb0 = _factors(csr, vdim)
    P0[:, d:] = 0
    Q0[:, d:] = 0
    Po, Qo, Qbo = P0[:, :d].copy(), Q0[:, :d].copy(), Qb0.copy()
    tr = H.run_oracle_sgd(oracle.OracleBPRMF, opt, csr, Po, Qo, Qbo, epochs=epochs, modes=DET, trace=True).get_trace()
    assert len(tr) == epochs * U * nn
    out = {}
    for ps in (2, 1):
        P, Q, Qb = P0.copy(), Q0.copy(), Qb0.copy()
        obj = H.run_hip_sgd(CyBPR, opt, csr, P, Q, Qb, epochs=epochs, modes=dict(hogwild_atomic=3, im_dual=1, im_presample=ps), resident=True)
        assert obj.stats()["samples"] == epochs * U * nn      # ... and im_check_done found as many on the device
        out[ps] = (P, Q, Qb)
    negs = tr[:, 2].reshape(epochs, U, nn).transpose(1, 0, 2).reshape(U, epochs * nn)
    touch = np.zeros(I, np.int64)
    np.add.at(touch, keys, 1)
    np.add.at(touch, negs.reshape(-1), 1)
    clean = (touch[keys] == 1) & (touch[negs] == 1).all(axis=1)
    assert clean.sum() > U // 4
    cu = np.flatnonzero(clean)
    ci, cj = keys[cu], negs[cu].reshape(-1)
    P2, Q2, Qb2 = out[2]
    P1, Q1, Qb1 = out[1]
    for got, ref in ((P2[cu][:, :d], Po[cu]), (Q2[ci][:, :d], Qo[ci]), (Q2[cj][:, :d], Qo[cj]), (Qb2[ci], Qbo[ci]), (Qb2[cj], Qbo[cj]),
                     (P2[cu], P1[cu]), (Q2[ci], Q1[ci]), (Q2[cj], Q1[cj]), (Qb2[ci], Qb1[ci]), (Qb2[cj], Qb1[cj])):
        assert H.relerr(got, ref) < 1e-5, H.relerr(got, ref)
    assert not np.array_equal(P2[cu], P0[cu])
    assert np.isfinite(P2).all() and np.isfinite(Q2).all() and np.all(P2[:, d:] == 0) and np.all(Q2[:, d:] == 0)


def test_reupload_rebuilds_the_walk_order_arrays():
    """One epoch, set_resident_csr with other keys (same row lengths: every size the cached regrouping is keyed on stays what it was),
    one more epoch -- against a fresh handle that is given the second matrix and the model after the first epoch.  One wave, so the two
    must be equal: the entry users and the inverse of the sort follow the matrix's generation like the regrouping itself."""
    from buffalo_amd.backend import CyBPR
    from buffalo_amd.synth import CSR
    csr1 = _dense_case()
    U, I = csr1.num_users, csr1.num_items
    beg = np.concatenate([[0], csr1.indptr[:-1]])
    keys2 = np.concatenate([(I - 1 - csr1.keys[b:e])[::-1] for b, e in zip(beg, csr1.indptr)]).astype(np.int32)
    assert not np.array_equal(keys2, csr1.keys)
    csr2 = CSR(U, I, csr1.indptr.copy(), keys2, np.ones(keys2.shape[0], np.float32))
    d, nn = 32, 3
    opt = bpr_opt(d=d, lr=0.05, min_lr=0.05, num_iters=2, random_seed=9, num_negative_samples=nn, accelerator=True)
    modes = dict(hogwild_atomic=3, im_single_wave=1, im_force_queues=4, im_presample=2)

    def handle(P, Q, Qb, csr, epoch):
        obj = CyBPR()
        path = H.write_opt(opt)
        assert obj.init(path)
        os.unlink(path)
        for k, v in modes.items():
            obj.set_mode(k, v)
        obj.initialize_model(P, Q, Qb, csr.nnz, True)
        obj.set_mode("epoch", epoch)
        obj.set_cumulative_table(H.cum_table(csr, opt), I)
        obj.set_resident_csr(csr.indptr, csr.keys)
        return obj

    def epoch(obj, csr):
        obj.add_jobs(0, U, csr.indptr, None)
        obj.update_parameters()          # copies the model back to the host arrays

    P, Q, Qb = _factors(csr1, d)
    a = handle(P, Q, Qb, csr1, 0)
    epoch(a, csr1)
    P_mid = P.copy()
    P1, Q1, Qb1 = P.copy(), Q.copy(), Qb.copy()
    a.set_resident_csr(csr2.indptr, csr2.keys)
    epoch(a, csr2)
    b = handle(P1, Q1, Qb1, csr2, 1)
    epoch(b, csr2)
    assert not np.array_equal(P, P_mid)
    for x, y in ((P, P1), (Q, Q1), (Qb, Qb1)):
        assert np.array_equal(x, y)
