"""bfh_als_fold_in on the device: the row-length edges of als_cases.pattern() inside the ALS envelope under both solve kernels, rows that do
not depend on their batch, a training run that does not notice the calls, a Gramian that follows the factor, host / device agreement,
top-k straight from the folded rows, and every refusal of the ABI."""
import ctypes as C

import numpy as np
import pytest

import als_cases as AC
import fold_in_cases as FC
import helpers as H
from ref_eals import bound, relerr

pytestmark = pytest.mark.gpu

BFH_ERR_INVALID, BFH_ERR_UNSUPPORTED = -1, -3


def fold(obj, m, axis, d, a=0, b=None):
    """Rows [a, b) of `m` as one fold_in call -> (rows [n, d], padding columns [n, vdim - d])."""
    b = m.num_users if b is None else b
    beg = 0 if a == 0 else int(m.indptr[a - 1])
    keys, vals = AC.chunk(m, a, b)
    X = obj.fold_in(axis, np.ascontiguousarray(m.indptr[a:b] - beg), keys, vals)
    assert X.shape == (b - a, AC.vdim_of(d)) and X.dtype == np.float32
    return X[:, :d], X[:, d:]


@pytest.mark.parametrize("knob", [1, 0])
@pytest.mark.parametrize("d, adaptive, axis", [(20, False, 0), (32, False, 0), (40, True, 0), (64, False, 0), (100, False, 0), (128, False, 0),
                                               (96, False, 1)])
def test_row_length_edges(d, adaptive, axis, knob):
    cmp_run, f64, Y, rows = FC.references(d, adaptive, axis)
    case = AC.pattern()
    obj = FC.make_hip(d, adaptive, {"als_fold_solve": knob})
    FC.bind(obj, case, d)
    X, pad = fold(obj, case.mat(axis), axis, d)
    assert np.isfinite(X).all()
    assert not X[0].any()                       # the empty history
    assert not pad.any()
    FC.hold("fold_in d=%d%s axis %d als_fold_solve=%d" % (d, " adaptive_reg" if adaptive else "", axis, knob), X, cmp_run, f64, rows)


def reversed_rows(m):
    """The same histories in reversed row order -> (indptr, keys, vals)."""
    bounds = FC.rows_of(m)[::-1]
    keys = np.concatenate([m.keys[b:e] for b, e in bounds])
    vals = np.concatenate([m.vals[b:e] for b, e in bounds])
    return np.cumsum([e - b for b, e in bounds], dtype=np.int64), np.ascontiguousarray(keys), np.ascontiguousarray(vals)


def test_a_row_does_not_depend_on_its_batch():
    d = 128
    cmp_run, f64, Y, rows = FC.references(d)
    case = AC.pattern()
    m = case.csr
    obj = FC.make_hip(d)
    FC.bind(obj, case, d)
    whole, _ = fold(obj, m, 0, d)
    calls = AC.chunked_calls(m.num_users)
    chunked = np.concatenate([fold(obj, m, 0, d, a, b)[0] for a, b in calls])
    back = obj.fold_in(0, *reversed_rows(m))[::-1, :d]
    slot_bytes = 4 * (128 * 128 + 2 * 128)
    obj.set_mode("als_fold_slot_bytes", 128 << 20)
    assert (m.num_users + 3) * slot_bytes >= 3 * (128 << 20)          # pattern() is cut at least three times
    cut, _ = fold(obj, m, 0, d)
    light = AC.lengths_of(m) <= AC.HEAVY
    assert (~light).sum() == 3
    for name, other in (("chunked calls", chunked), ("reversed order", back), ("smaller sub-batches", cut)):
        assert np.array_equal(whole[light].view(np.uint32), other[light].view(np.uint32)), name
        for r in np.flatnonzero(~light):         # chunks summed with atomics: the envelope, not the bits
            assert relerr(other[r], f64[r]) <= bound(relerr(cmp_run[r], f64[r])), (name, r)
    FC.hold("fold_in d=128 smaller sub-batches", cut, cmp_run, f64, rows)


def _training(d, optimizer, with_folds):
    """One user half-epoch, then the item half-epoch in two calls -- with fold_in calls after precompute and between the calls, or without."""
    case = AC.tiny(31)
    obj = FC.make_hip(d, optimizer=optimizer)
    P, Q = (H.pad(x.copy(), AC.vdim_of(d)) for x in AC.start(case, d))
    AC.bind(obj, case, P, Q, True)
    obj.precompute(0)
    loss = [obj.partial_update(0, case.users, case.csr.indptr, case.csr.keys, case.csr.vals, 0)]
    plans = [AC.plan_of(obj)]
    folds = []
    obj.precompute(1)
    mid = case.items // 2
    for a, b in ((0, mid), (mid, case.items)):
        if with_folds:
            folds.append(obj.fold_in(0, case.csr.indptr, case.csr.keys, case.csr.vals))
            folds.append(obj.fold_in(1, case.t.indptr, case.t.keys, case.t.vals))
        loss.append(obj.partial_update(a, b, case.t.indptr, *AC.chunk(case.t, a, b), 1))
        plans.append(AC.plan_of(obj))
    return P, Q, loss, plans, folds


@pytest.mark.parametrize("d, optimizer", [(128, None), (40, "llt")])
def test_training_is_not_disturbed(d, optimizer):
    P0, Q0, loss0, plans0, _ = _training(d, optimizer, False)
    P1, Q1, loss1, plans1, folds = _training(d, optimizer, True)
    assert np.array_equal(P0.view(np.uint32), P1.view(np.uint32)) and np.array_equal(Q0.view(np.uint32), Q1.view(np.uint32))
    assert loss0 == loss1 and plans0 == plans1
    assert len(folds) == 4 and all(np.isfinite(f).all() and f.any() for f in folds)
    assert not np.array_equal(folds[0], folds[2])     # the second user fold saw the item rows of the first call


def _tiny_references(case, Q, d):
    f64 = FC.fold_f64(case.csr, Q, 0)
    return FC.fold_f32(case.csr, Q, 0), f64


def test_gramian_follows_the_factor():
    d, case = 128, AC.tiny(47)
    obj = FC.make_hip(d)
    P, Q = (H.pad(x.copy(), 128) for x in AC.start(case, d))
    AC.bind(obj, case, P, Q, True)
    m = case.csr
    first = obj.fold_in(0, m.indptr, m.keys, m.vals)
    FC.hold("fold_in tiny d=128 first", first, *_tiny_references(case, Q.copy(), d), named=0)
    obj.precompute(1)
    obj.partial_update(0, case.items, case.t.indptr, case.t.keys, case.t.vals, 1)      # Q changes (and is written back to the host array)
    aux0 = obj.stats()["aux_ms"]
    second = obj.fold_in(0, m.indptr, m.keys, m.vals)
    aux1 = obj.stats()["aux_ms"]
    third = obj.fold_in(0, m.indptr, m.keys, m.vals)
    aux2 = obj.stats()["aux_ms"]
    assert not np.array_equal(first, second)
    FC.hold("fold_in tiny d=128 after the item half-epoch", second, *_tiny_references(case, Q.copy(), d), named=0)
    assert np.array_equal(second.view(np.uint32), third.view(np.uint32))
    assert aux1 > aux0 and aux2 == aux1            # the Gramian kernels are timed into aux_ms: run for the second call, not for the third


def test_host_and_device_rows_agree():
    import torch
    d, case = 100, AC.tiny(31)
    obj = FC.make_hip(d)
    FC.bind(obj, case, d)
    m = case.csr
    out = np.full((m.num_users, 128), np.nan, dtype=np.float32)
    assert obj.fold_in(0, m.indptr, m.keys, m.vals, out) is out
    ptr, n = obj.fold_in_device(0, m.indptr, m.keys, m.vals)
    assert ptr and n == m.num_users and obj.device_buffer("fold") == (ptr, n * 128 * 4)
    dev = obj.device_tensor("fold", (n, 128)).cpu().numpy()
    torch.cuda.synchronize()
    assert np.array_equal(out.view(np.uint32), dev.view(np.uint32))


def test_fold_in_recommend():
    from buffalo_amd.parallel import NO_BIAS, TopK, fold_in_recommend
    d, k, case = 128, 10, AC.tiny(31)
    m = case.csr
    assert AC.lengths_of(m).max() <= AC.HEAVY
    obj = FC.make_hip(d)
    _, Q = FC.bind(obj, case, d)
    pool = np.zeros(0, dtype=np.int32)
    keys, scores = np.zeros((m.num_users, k), np.int32), np.zeros((m.num_users, k), np.float32)
    fold_in_recommend(obj, m.indptr, m.keys, m.vals, keys, scores, pool, k)
    rows = obj.fold_in(0, m.indptr, m.keys, m.vals)
    eng = TopK()
    eng.set_seen(m.indptr, m.keys, m.num_items)
    ek, es = np.zeros_like(keys), np.zeros_like(scores)
    eng.recommend_unseen(np.arange(m.num_users, dtype=np.int32), rows, Q, NO_BIAS, ek, es, pool, k)
    assert np.array_equal(keys, ek) and np.array_equal(scores.view(np.uint32), es.view(np.uint32))
    for u in range(m.num_users):
        assert not np.intersect1d(keys[u], m.row(u)[0]).size
    assert (keys >= 0).all() and len(set(keys[0].tolist())) == k


def _raw(obj, axis, n_rows, indptr, keys, vals, nnz, out=None):
    """bfh_als_fold_in as C sees it (None = NULL) -> (status, message)."""
    ptr = lambda a, ct: None if a is None else a.ctypes.data_as(C.POINTER(ct))   # noqa: E731
    st = obj._L.bfh_als_fold_in(obj._h, axis, n_rows, ptr(indptr, C.c_int64), ptr(keys, C.c_int32), ptr(vals, C.c_float), nnz, ptr(out, C.c_float))
    return st, (obj._L.bfh_last_error(obj._h) or b"").decode()


def test_refusals():
    from buffalo_amd.backend import CyALS
    d, case = 40, AC.tiny(31)
    m = case.csr
    ip, ks, vs, n, nnz = m.indptr, m.keys, m.vals, m.num_users, m.nnz
    cold = FC.make_hip(d)
    st, msg = _raw(cold, 0, n, ip, ks, vs, nnz)
    assert st == BFH_ERR_INVALID and "initialize_model" in msg
    obj = FC.make_hip(d)
    FC.bind(obj, case, d)
    good = obj.fold_in(0, ip, ks, vs)
    f64 = FC.fold_f64(m, AC.start(case, d)[1], 0)
    assert relerr(good[:, :d], f64) <= 1e-5

    def bad_key(pos, value):
        k = ks.copy()
        k[pos] = value
        return k

    dec = ip.copy()
    dec[5] = dec[4] - 1
    short = ip.copy()
    short[-1] -= 1
    cases = [("axis", (2, n, ip, ks, vs, nnz), "axis"), ("axis", (-1, n, ip, ks, vs, nnz), "axis"),
             ("n_rows < 0", (0, -1, ip, ks, vs, nnz), "n_rows"),
             ("decreasing indptr", (0, n, dec, ks, vs, nnz), "decreases"),
             ("indptr[-1] != nnz", (0, n, ip, ks, vs, nnz - 1), "nnz"), ("indptr[-1] != nnz", (0, n, short, ks, vs, nnz), "nnz"),
             ("null keys", (0, n, ip, None, vs, nnz), "null"), ("null vals", (0, n, ip, ks, None, nnz), "null"),
             ("null indptr", (0, n, None, ks, vs, nnz), "null"),
             ("key == num_items", (0, n, ip, bad_key(nnz // 2, m.num_items), vs, nnz), "outside"),
             ("key == -1", (0, n, ip, bad_key(nnz - 1, -1), vs, nnz), "outside"),
             ("axis 1: key == num_users", (1, case.items, case.t.indptr, np.where(np.arange(nnz) == 3, m.num_users, 0).astype(np.int32), vs, nnz), "outside")]
    for name, args, word in cases:
        before = obj.stats()
        st, msg = _raw(obj, *args)
        after = obj.stats()
        assert st == BFH_ERR_INVALID and word in msg, (name, st, msg)
        # refused with the device untouched: nothing timed, nothing uploaded
        assert after["kernel_ms"] == before["kernel_ms"] and after["aux_ms"] == before["aux_ms"] and after["h2d_bytes"] == before["h2d_bytes"], name
        again = obj.fold_in(0, ip, ks, vs)          # the handle still folds, to the same bits
        assert np.array_equal(again.view(np.uint32), good.view(np.uint32)), name
    assert case.t.indptr[-1] == nnz
    # no rows: status 0, nothing launched, an empty result
    before = obj.stats()
    st, _ = _raw(obj, 0, 0, None, None, None, 0)
    assert st == 0 and obj.stats()["kernel_ms"] == before["kernel_ms"] and obj.stats()["launches"] == before["launches"]
    assert obj.fold_in(0, ip[:0].copy(), ks[:0].copy(), vs[:0].copy()).shape == (0, AC.vdim_of(d))
    assert np.array_equal(obj.fold_in(0, ip, ks, vs).view(np.uint32), good.view(np.uint32))
    # above vdim 128: there is no dense solve
    wide = FC.make_hip(160)
    FC.bind(wide, case, 160)
    st, msg = _raw(wide, 0, n, ip, ks, vs, nnz)
    assert st == BFH_ERR_UNSUPPORTED and "128" in msg, (st, msg)
    with pytest.raises(ValueError):
        CyALS.fold_in(obj, 0, ip.astype(np.int32), ks, vs)      # dtype checks in the file's _arr style
    with pytest.raises(ValueError):
        obj.fold_in(0, ip, ks, vs, out=np.zeros((n, d), dtype=np.float32))
