"""bfh_plsi_fold_in on the device (csrc/plsi_fold_kernels.hpp behind CyPLSI.fold_in) against the float64 restatement of its definition
(tests/plsi_fold_cases.py): one step inside the derived bound at every kernel dispatch and row-length edge, steps that compose bitwise, rows
that are the trainer's rows bit for bit and do not depend on their batch, free-running steps, the per-row loss, a training epoch that does not
notice the calls, host / device agreement, top-k straight from the folded rows, and every refusal of the ABI."""
import ctypes as C
import os

import numpy as np
import pytest

import als_cases as AC
import helpers as H
import plsi_fold_cases as FC
import ref_plsi as R

pytestmark = pytest.mark.gpu

BFH_ERR_INVALID = -1
TIMES = ("kernel_ms", "optimizer_ms", "aux_ms", "exchange_kernel_ms", "allreduce_ms")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def make(d, P, Q):
    """A CyPLSI whose model is the given arrays (keep_init); they are the caller's and are rewritten by swap."""
    from buffalo_amd.backend import CyPLSI
    g = CyPLSI()
    path = H.write_opt({"d": d, "random_seed": 0, "num_workers": 1, "num_iters": 10, "alpha1": 1.0, "alpha2": 1.0, "eps": 1e-10})
    assert g.init(path)
    os.unlink(path)
    g.set_mode("keep_init", 1)
    g.initialize_model(P, Q)
    return g


def model(d, n_rows):
    """(handle, start rows, Q): the model the histories are folded against; its P is the start rows (fold_in never reads it)."""
    P, Q = (x.copy() for x in FC.start(n_rows, d))
    return make(d, P, Q), P, Q


def fold(g, m, iters, alpha1, init=None, loss=False):
    L = np.full(m.num_users, np.nan) if loss else None
    out = g.fold_in(m.indptr, m.keys, m.vals, iters, alpha1, init=None if init is None else np.ascontiguousarray(init), loss=L)
    return (out, L) if loss else out


def _one_step(d, values, alpha1):
    m = FC.pattern(d, values, empty=alpha1 > 0)         # alpha1 = 0: a row without entries is 0 / 0, in the reference as well
    g, P, Q = model(d, m.num_users)
    assert FC.clamp_is_reached(P, Q, m)
    out = fold(g, m, 1, alpha1, P)
    f64, _ = FC.fold_ref(P, Q, m, 1, alpha1)
    r = FC.ratio(out, f64, FC.one_step_bound(m, d))
    per = ["%d: %.2f" % (n, FC.ratio(out[[i]], f64[[i]], FC.one_step_bound(m, d)[[i]])) for i, n in enumerate(FC.named_lengths(d, alpha1 > 0))]
    AC.record("plsi fold_in one step d=%d %s alpha1=%g" % (d, values, alpha1), ["error / bound %.3f; per row, entries: error / bound  %s" % (r, "  ".join(per))])
    assert r <= 1.0, r
    return out


@pytest.mark.parametrize("alpha1", [1.0, 0.0])
@pytest.mark.parametrize("d", [1, 7, 20, 32, 33, 128, 200, 300, 520])          # every (G, C) dispatch: 520 is the one with four chunks per lane
def test_one_step_against_float64(d, alpha1):
    out = _one_step(d, "ratings", alpha1)
    if alpha1 > 0:                                                               # the empty history: the smoothing alone
        a1 = np.float32(alpha1) / np.float32(d)
        s = np.float32(0)
        for _ in range(d):
            s = s + a1
        assert np.abs(out[0].astype(np.float64) - np.float64(a1 / s)).max() <= d * R.U24 * float(a1 / s)


@pytest.mark.parametrize("values", ["counts", "ones"])
@pytest.mark.parametrize("alpha1", [1.0, 0.0])
@pytest.mark.parametrize("d", [20, 200])
def test_alpha_and_value_kinds(d, alpha1, values):
    _one_step(d, values, alpha1)


@pytest.mark.parametrize("d", [20, 128, 300])
def test_steps_compose_bitwise(d):
    m = FC.pattern(d)
    g, P, _ = model(d, m.num_users)
    for t in (2, 10):
        whole, lw = fold(g, m, t, 1.0, P, loss=True)
        before = fold(g, m, t - 1, 1.0, P)
        last, ll = fold(g, m, 1, 1.0, before, loss=True)
        assert np.array_equal(bits(whole), bits(last)), t
        assert np.array_equal(bits(lw), bits(ll)), t                             # the loss is the last step's, from p(iters - 1)
    uni = fold(g, m, 2, 1.0)                                                     # the uniform start is the row of 1 / d
    assert np.array_equal(bits(uni), bits(fold(g, m, 2, 1.0, FC.uniform(m.num_users, d))))


@pytest.mark.parametrize("alpha1", [1.0, 0.0])
@pytest.mark.parametrize("d", [20, 128, 200])
def test_equals_the_trainer_bitwise(d, alpha1):
    """Three epochs of the trainer over the same rows with Q put back after every swap: the same bits, short rows, team rows and the rows the
    trainer cuts into slabs alike.  alpha1 = 0 makes the empty row NaN on both sides; NaN rows are left out of the comparison."""
    iters = 3
    m = FC.pattern(d)
    g, P0, Q0 = model(d, m.num_users)
    out = fold(g, m, iters, alpha1, P0)
    P, Q = P0.copy(), Q0.copy()
    t = make(d, P, Q)
    for _ in range(iters):
        t.reset()
        t.partial_update(0, m.num_users, m.indptr, m.keys, m.vals)
        t.normalize(alpha1, 1.0)
        t.swap()
        Q[:] = Q0
        t.synchronize(False)
    assert t.get_stats()["merges"] >= 2 * iters                                  # the rows of 2048 + 1 and 2 * 2048 + 1 entries: the trainer summed slabs
    nan = np.isnan(P).any(axis=1)
    assert np.array_equal(nan, np.isnan(out).any(axis=1)) and nan.sum() == (0 if alpha1 > 0 else 1)
    assert np.array_equal(bits(P[~nan]), bits(out[~nan]))
    assert not np.array_equal(bits(P[~nan]), bits(P0[~nan]))


@pytest.mark.parametrize("d", [20, 128])
def test_a_row_does_not_depend_on_its_batch(d):
    m = FC.pattern(d)
    n = m.num_users
    g, P, _ = model(d, n)
    whole, lw = fold(g, m, 3, 1.0, P, loss=True)

    def run(rows):
        rows = list(rows)
        return fold(g, FC.take(m, rows), 3, 1.0, P[rows], loss=True)

    back, lb = run(range(n - 1, -1, -1))
    assert np.array_equal(bits(whole), bits(back[::-1])) and np.array_equal(bits(lw), bits(lb[::-1]))
    cuts = [0, 5, n // 2, n]
    parts = [run(range(a, b)) for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(bits(whole), bits(np.concatenate([p[0] for p in parts])))
    assert np.array_equal(bits(lw), bits(np.concatenate([p[1] for p in parts])))
    alone = [run([r]) for r in range(n)]
    assert np.array_equal(bits(whole), bits(np.concatenate([p[0] for p in alone])))
    assert np.array_equal(bits(lw), bits(np.concatenate([p[1] for p in alone])))


@pytest.mark.parametrize("d", [20, 128])
def test_ten_free_steps_from_the_uniform_start(d):
    m = FC.pattern(d)
    g, _, Q = model(d, m.num_users)
    out = fold(g, m, 10, 1.0)
    assert np.array_equal(bits(out), bits(fold(g, m, 10, 1.0)))
    f64, _ = FC.fold_ref(None, Q, m, 10, 1.0, np.float64)
    f32, _ = FC.fold_ref(None, Q, m, 10, 1.0, np.float32)
    e32, e_hip, floor = R.relerr_elements(f32, f64), R.relerr_elements(out, f64), float(R.bound_normalized(FC.lengths_of(m).max(), d, d))
    AC.record("plsi fold_in 10 free steps d=%d" % d, ["e_hip %.3e  e32 %.3e  one-step bound %.3e" % (e_hip, e32, floor)])
    assert e_hip <= max(2.5 * e32, floor), (e_hip, e32, floor)


@pytest.mark.parametrize("d", [20, 200])
def test_loss_per_row(d):
    m = FC.pattern(d)
    g, P, Q = model(d, m.num_users)
    out, loss = fold(g, m, 1, 1.0, P, loss=True)
    assert np.array_equal(bits(out), bits(fold(g, m, 1, 1.0, P)))                # the build without the loss: the same rows
    l64, l32 = FC.fold_ref(P, Q, m, 1, 1.0, np.float64)[1], FC.fold_ref(P, Q, m, 1, 1.0, np.float32)[1]
    assert loss[0] == 0 and l64[0] == 0                                           # the empty history
    e32, e_hip = np.abs(l32[1:] - l64[1:]) / np.abs(l64[1:]), np.abs(loss[1:] - l64[1:]) / np.abs(l64[1:])
    AC.record("plsi fold_in loss d=%d" % d, ["largest relerr hip %.2e float32 %.2e floor %.2e" % (e_hip.max(), e32.max(), (d + 8) * R.U24)])
    worst = int(np.argmax(e_hip - np.maximum(e32, (d + 8) * R.U24)))
    assert (e_hip <= np.maximum(e32, (d + 8) * R.U24)).all(), (worst + 1, e_hip[worst], e32[worst])


def _epoch(with_folds):
    d = 20
    csr = R.skewed_case(600, 200, seed=9)
    P, Q = R.clamped_start(600, 200, d, seed=3)
    g = make(d, P, Q)
    folds, losses = [], []
    g.reset()
    for a, b in H.chunks_of(csr, 2):
        losses.append(g.partial_update(a, b, csr.indptr, *H.chunk_arrays(csr, a, b)))
        if with_folds:
            folds.append(g.fold_in(csr.indptr, csr.keys, csr.vals, 2, 1.0))
    times = {k: g.get_stats()[k] for k in TIMES}
    if with_folds:
        folds.append(g.fold_in(csr.indptr, csr.keys, csr.vals, 2, 1.0))
        assert {k: g.get_stats()[k] for k in TIMES} == times                     # the five timing fields belong to training
        assert g.fold_kernel_ms > 0
    g.normalize(1.0, 1.0)
    g.swap()
    if with_folds:
        folds.append(g.fold_in(csr.indptr, csr.keys, csr.vals, 2, 1.0))
    return P, Q, losses, folds, g.get_stats(), csr


def test_training_is_not_disturbed():
    P0, Q0, loss0, _, st0, _ = _epoch(False)
    P1, Q1, loss1, folds, st1, csr = _epoch(True)
    assert np.array_equal(bits(P0), bits(P1)) and np.array_equal(bits(Q0), bits(Q1)) and loss0 == loss1
    assert len(folds) == 4 and all(np.isfinite(f).all() for f in folds)
    assert np.array_equal(bits(folds[0]), bits(folds[2])) and not np.array_equal(bits(folds[0]), bits(folds[3]))     # Q changed at the swap only
    # the counters of the calls: exchanges = calls, accepted = rows, loaded_rows = rows of Q gathered (entries x steps), one launch each
    assert st1["exchanges"] - st0["exchanges"] == 4 and st1["accepted"] - st0["accepted"] == 4 * csr.num_users
    assert st1["loaded_rows"] - st0["loaded_rows"] == 4 * 2 * csr.nnz and st1["launches"] - st0["launches"] == 4
    assert st1["samples"] == st0["samples"] and st1["merges"] == st0["merges"]


def test_host_and_device_rows_agree():
    import torch
    d = 33
    m = FC.pattern(d)
    g, P, _ = model(d, m.num_users)
    vdim = g.get_vdim()
    assert vdim == 64
    for alpha1 in (1.0, 0.0):                                                    # alpha1 = 0: the empty row is NaN, its padding still 0
        out = np.full((m.num_users, d), np.nan, dtype=np.float32)
        assert g.fold_in(m.indptr, m.keys, m.vals, 2, alpha1, init=P, out=out) is out
        ptr, n = g.fold_in_device(m.indptr, m.keys, m.vals, 2, alpha1, init=P)
        assert ptr and n == m.num_users and g.device_buffer("fold") == (ptr, n * vdim * 4)
        dev = g.device_tensor("fold", (n, vdim)).cpu().numpy()
        torch.cuda.synchronize()
        assert np.array_equal(bits(out), bits(dev[:, :d]))
        assert not dev[:, d:].any()
        assert np.isnan(out[0]).all() == (alpha1 == 0) and np.isfinite(out[1:]).all()


def test_fold_in_recommend():
    from buffalo_amd.parallel import NO_BIAS, TopK, plsi_fold_in_recommend
    d, k = 20, 10
    csr = R.skewed_case(200, 300, seed=2)                                        # keys ascend inside a row
    P, Q = R.init_model(200, 300, d, seed=5)
    g = make(d, P, Q)
    pool = np.zeros(0, dtype=np.int32)
    keys, scores = np.zeros((csr.num_users, k), np.int32), np.zeros((csr.num_users, k), np.float32)
    plsi_fold_in_recommend(g, csr.indptr, csr.keys, csr.vals, 5, 1.0, keys, scores, pool, k)
    rows = g.fold_in(csr.indptr, csr.keys, csr.vals, 5, 1.0)
    eng = TopK()
    eng.set_seen(csr.indptr, csr.keys, csr.num_items)
    ek, es = np.zeros_like(keys), np.zeros_like(scores)
    eng.recommend_unseen(np.arange(csr.num_users, dtype=np.int32), rows, Q, NO_BIAS, ek, es, pool, k)
    assert np.array_equal(keys, ek) and np.array_equal(bits(scores), bits(es))
    beg = np.concatenate([[0], csr.indptr[:-1]])
    for u in range(csr.num_users):
        assert not np.intersect1d(keys[u], csr.keys[beg[u]:csr.indptr[u]]).size
    assert (keys >= 0).all() and len(set(keys[0].tolist())) == k


def _raw(g, n_rows, indptr, keys, vals, nnz, iters=2, alpha1=1.0, init=None, out=None):
    """bfh_plsi_fold_in as C sees it (None = NULL) -> (status, message)."""
    ptr = lambda a, ct: None if a is None else a.ctypes.data_as(C.POINTER(ct))   # noqa: E731
    st = g._L.bfh_plsi_fold_in(g._h, n_rows, ptr(indptr, C.c_int64), ptr(keys, C.c_int32), ptr(vals, C.c_float), nnz, iters, alpha1,
                               ptr(init, C.c_float), ptr(out, C.c_float), None, None)
    return st, (g._L.bfh_last_error(g._h) or b"").decode()


def test_refusals():
    from buffalo_amd.backend import CyPLSI
    d = 20
    csr = R.skewed_case(100, 40, seed=1)
    ip, ks, vs, n, nnz = csr.indptr, csr.keys, csr.vals, csr.num_users, csr.nnz
    P, Q = R.init_model(100, 40, d, seed=1)
    cold = CyPLSI()
    path = H.write_opt({"d": d, "random_seed": 0})
    assert cold.init(path)
    os.unlink(path)
    st, msg = _raw(cold, n, ip, ks, vs, nnz)
    assert st == BFH_ERR_INVALID and "initialize_model" in msg
    g = make(d, P, Q)
    good = g.fold_in(ip, ks, vs, 2, 1.0)
    f64, _ = FC.fold_ref(None, Q, csr, 2, 1.0)
    assert R.relerr_elements(good, f64) <= 1e-5

    def bad_key(pos, value):
        k = ks.copy()
        k[pos] = value
        return k

    dec = ip.copy()
    dec[5] = dec[4] - 1
    short = ip.copy()
    short[-1] -= 1
    cases = [("n_rows < 0", (-1, ip, ks, vs, nnz), "n_rows"),
             ("iters == 0", (n, ip, ks, vs, nnz, 0), "iters"), ("iters == -1", (n, ip, ks, vs, nnz, -1), "iters"),
             ("iters == 10001", (n, ip, ks, vs, nnz, 10001), "iters"),
             ("alpha1 < 0", (n, ip, ks, vs, nnz, 2, -0.5), "alpha1"), ("alpha1 nan", (n, ip, ks, vs, nnz, 2, float("nan")), "alpha1"),
             ("alpha1 inf", (n, ip, ks, vs, nnz, 2, float("inf")), "alpha1"),
             ("decreasing indptr", (n, dec, ks, vs, nnz), "decreases"),
             ("indptr[-1] != nnz", (n, ip, ks, vs, nnz - 1), "nnz"), ("indptr[-1] != nnz", (n, short, ks, vs, nnz), "nnz"),
             ("null keys", (n, ip, None, vs, nnz), "null"), ("null vals", (n, ip, ks, None, nnz), "null"), ("null indptr", (n, None, ks, vs, nnz), "null"),
             ("key == num_items", (n, ip, bad_key(nnz // 2, csr.num_items), vs, nnz), "outside"),
             ("key == -1", (n, ip, bad_key(nnz - 1, -1), vs, nnz), "outside")]
    for name, args, word in cases:
        before = g.get_stats()
        st, msg = _raw(g, *args)
        after = g.get_stats()
        assert st == BFH_ERR_INVALID and word in msg, (name, st, msg)
        # refused with the device untouched: nothing launched, nothing uploaded
        assert all(after[k] == before[k] for k in ("launches", "exchanges", "accepted", "loaded_rows", "h2d_bytes", "d2h_bytes")), name
        assert np.array_equal(bits(g.fold_in(ip, ks, vs, 2, 1.0)), bits(good)), name          # the handle still folds, to the same bits
    # no rows: status 0, nothing launched, an empty result
    before = g.get_stats()
    st, _ = _raw(g, 0, None, None, None, 0)
    assert st == 0 and all(g.get_stats()[k] == before[k] for k in ("launches", "exchanges", "h2d_bytes"))
    assert g.fold_in(ip[:0].copy(), ks[:0].copy(), vs[:0].copy(), 2, 1.0).shape == (0, d)
    assert g.device_buffer("fold") == (None, 0)
    assert np.array_equal(bits(g.fold_in(ip, ks, vs, 2, 1.0)), bits(good))
    # the Python mirror: dtype and shape checks in the file's _arr style
    with pytest.raises(ValueError):
        g.fold_in(ip.astype(np.int32), ks, vs, 2, 1.0)
    with pytest.raises(ValueError):
        g.fold_in(ip, ks.astype(np.int64), vs, 2, 1.0)
    with pytest.raises(ValueError):
        g.fold_in(ip, ks, vs[:-1].copy(), 2, 1.0)
    with pytest.raises(ValueError):
        g.fold_in(ip, ks, vs, 2, 1.0, out=np.zeros((n, g.get_vdim()), dtype=np.float32))
    with pytest.raises(ValueError):
        g.fold_in(ip, ks, vs, 2, 1.0, init=np.zeros((n, d), dtype=np.float64))
    with pytest.raises(ValueError):
        g.fold_in(ip, ks, vs, 2, 1.0, init=np.zeros((n - 1, d), dtype=np.float32))
    with pytest.raises(ValueError):
        g.fold_in(ip, ks, vs, 2, 1.0, loss=np.zeros(n, dtype=np.float32))
    with pytest.raises(TypeError):
        g.fold_in(ip, ks.tolist(), vs, 2, 1.0)
