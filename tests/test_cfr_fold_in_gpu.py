"""bfh_cfr_fold_in on the device against the float64 statement of its rule (tests/cfr_fold_cases.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import cfr_cases as CC
import cfr_fold_cases as FC
import helpers as H
from ref_cfr import ARRAYS, F64CFR, bound, relerr

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make(d, arrs=None, names=ARRAYS, optimizer="manual_cg"):
    """A CyCFR at d (manual_cg: fold_in solves exactly whatever the optimizer is) with copies of `arrs` bound -> (object, the bound copies)."""
    from buffalo_amd.backend import CyCFR
    g = FC.init_of(CyCFR(), d, optimizer)
    mine = {k: v.copy() for k, v in (arrs or {}).items() if k in names}
    for k, v in mine.items():
        g.set_embedding(v, k)
    return g, mine


def run(g, kind, iters, init, rows=None):
    """fold_in of the case's rows (`rows`: those, in that order) -> (x, b)"""
    a, c = FC.case().parts(kind, rows)
    if init is not None and rows is not None:
        init = init[list(rows)].copy()
    return g.fold_in(kind, *a, *c, iters=iters, init_bias=init)


@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("d", [1, 33, 64, 65, 96, 128])
@pytest.mark.parametrize("kind", ["user", "item", "context"])
def test_length_edges_inside_the_envelope(kind, d, iters):
    arrs, init, cmp_run, f64 = FC.references(kind, d, iters)
    g, _ = make(d, arrs, [n for n in FC.KINDS[kind][:3] if n])          # only the arrays the kind reads; no precompute
    X, b = run(g, kind, iters, init)
    FC.hold("fold_in %s d=%d iters=%d" % (kind, d, iters), X, b, cmp_run, f64)
    assert not X[0].any() and (kind == "user" or b[0] == init[0])      # the (0, 0) row
    if kind == "item":
        nc0 = np.array([l[0] > 0 and l[1] == 0 for l in FC.case().lens])
        assert nc0.any() and not b[nc0].any()                           # solved from part a alone: 0 / 1e-10 (a context without part c is an empty row)
    vd = g.get_vdim()
    dev = g.device_tensor("fold", (X.shape[0], vd)).cpu().numpy()
    assert g.dim() == d and np.array_equal(bits(dev[:, :d]), bits(X)) and not dev[:, d:].any()
    assert g.device_buffer("fold_bias")[1] == (0 if kind == "user" else 4 * X.shape[0])


@pytest.mark.parametrize("d", [64, 128])
def test_one_iteration_is_the_trainer_step(d):
    cs = FC.case()
    arrs = FC.references("item", d, 1)[0]
    g, mine = make(d, arrs)
    for kind, args in (("item", (cs.a.indptr, cs.a.keys, cs.a.vals, cs.c.indptr, cs.c.keys, cs.c.vals)), ("context", (cs.c.indptr, cs.c.keys, cs.c.vals))):
        init = arrs[kind + "_bias"][:cs.n, 0].copy()
        X, b = run(g, kind, 1, init)
        # the same rows as rows 0 .. n of the model: one trainer step on a second handle (exact solve) and in float64, from the same start
        tr, theirs = make(d, arrs, optimizer="llt")
        ref = FC.init_of(F64CFR(), d, "llt")
        CC.bind(ref, {k: v.copy() for k, v in arrs.items()})
        for o in (tr, ref):
            o.precompute(b"user")
            getattr(o, "partial_update_" + kind)(0, cs.n, *args)
        live = np.array([(l[0] if kind == "item" else 0) + l[1] > 0 for l in cs.lens])
        want = np.where(live[:, None], ref.F[kind][:cs.n], 0.0), np.where(live, ref.F[kind + "_bias"][:cs.n, 0], init)
        cmp_run = FC.fold(kind, arrs, cs, 1, init, np.float32)
        FC.hold("fold_in %s d=%d iters=1 against the float64 trainer step" % (kind, d), X, b, cmp_run, want)
        step = theirs[kind][:cs.n][live]
        assert relerr(X[live], step) <= bound(relerr(cmp_run[0], want[0])) + relerr(step, want[0][live])      # ... and beside the device's own step
    assert all(np.array_equal(bits(mine[k]), bits(arrs[k])) for k in ARRAYS)      # the folding handle's five arrays are untouched


def test_a_row_does_not_depend_on_its_batch():
    d, kind, n = 96, "item", FC.case().n
    arrs, init, _, _ = FC.references(kind, d, 3)
    g, _ = make(d, arrs)
    whole = run(g, kind, 3, init)
    parts = [run(g, kind, 3, init, rows) for rows in (range(0, 5), range(5, 5), range(5, n))]
    back = run(g, kind, 3, init, range(n - 1, -1, -1))
    again = run(make(d, arrs)[0], kind, 3, init)
    for i in (0, 1):
        assert np.array_equal(bits(whole[i]), bits(np.concatenate([p[i] for p in parts])))
        assert np.array_equal(bits(whole[i]), bits(back[i][::-1])) and np.array_equal(bits(whole[i]), bits(again[i]))


def test_training_does_not_notice():
    d, case, runs = 33, CC.tiny(3), []
    csr = lambda m: (m.indptr, m.keys, m.vals)                           # noqa: E731
    none = (None,) * 3
    folds = (("user", csr(case.csr), none), ("item", csr(case.t), csr(case.ctx)), ("context", none, csr(case.ctx)))
    for with_folds in (False, True):
        arrs = CC.arrays(case, d)
        g, _ = make(d)
        CC.bind(g, arrs)
        losses = []
        for upd in (CC.update_user, CC.update_item, CC.update_context):   # one epoch, the model's own rows folded in before every call
            for kind, a, c in folds if with_folds else ():
                g.fold_in(kind, *a, *c, iters=2)
            losses.append(upd(g, case))
        runs.append((arrs, losses))
    (a0, l0), (a1, l1) = runs
    assert all(np.array_equal(bits(a0[k]), bits(a1[k])) for k in ARRAYS)
    # the losses: the trainer's loss kernels add their doubles with atomics, in an order that changes from run to run without any fold-in;
    # at most 1e4 terms of one sign pattern, each addition rounded to 2^-53: 1e4 x 2^-53 = 1.1e-12
    assert all(abs(x - y) <= 1.1e-12 * abs(x) for x, y in zip(l0, l1)), (l0, l1)


def test_refusals_launch_nothing_and_recommend():
    from buffalo_amd import parallel as par
    from buffalo_amd.backend import BuffaloHipError, CyCFR
    d, cs = 20, FC.case()
    arrs = FC.references("item", d, 1)[0]
    g, _ = make(d, arrs, ("item",))
    (ip, k, v), _ = cs.parts("user")
    with pytest.raises(BuffaloHipError, match="before set_embedding"):
        g.fold_in("item", ip, k, v, ip, k, v)
    g, _ = make(d, arrs)
    X, _ = g.fold_in("user", ip, k, v)
    n, nnz = ip.shape[0], k.shape[0]
    bad_ip, bad_k, one = ip.copy(), k.copy(), np.zeros(n, np.float32)
    bad_ip[1], bad_k[-1] = -1, FC.N
    P = lambda x, t: None if x is None else x.ctypes.data_as(C.POINTER(t))      # noqa: E731
    A, NO = (P(ip, C.c_int64), P(k, C.c_int32), P(v, C.c_float), nnz), (None, None, None, 0)
    table = [("unknown obj_type", (b"users", n, *A, *NO, 1, None, None, None)), ("n_rows is negative", (b"user", -1, *A, *NO, 1, None, None, None)),
             ("iters must be at least 1", (b"user", n, *A, *NO, 0, None, None, None)),
             ("indptr decreases at row 1", (b"user", n, P(bad_ip, C.c_int64), *A[1:], *NO, 1, None, None, None)),
             (r"indptr\[n_rows - 1\] != nnz", (b"user", n, *A[:3], nnz - 1, *NO, 1, None, None, None)),
             ("null keys / vals", (b"user", n, A[0], None, None, nnz, *NO, 1, None, None, None)),
             ("part c given, but this obj_type has none", (b"user", n, *A, *A, 1, None, None, None)),
             ("part a given, but this obj_type has none", (b"context", n, *A, *A, 1, None, None, None)),
             ("part a is missing", (b"user", n, *NO, *NO, 1, None, None, None)),
             ("a user has no bias", (b"user", n, *A, *NO, 1, P(one, C.c_float), None, None)),
             ("a user has no bias", (b"user", n, *A, *NO, 1, None, None, P(one, C.c_float))),
             (r"part c: key %d at position %d is outside \[0, %d\)" % (FC.N, nnz - 1, FC.N), (b"item", n, *A, A[0], P(bad_k, C.c_int32), A[2], nnz, 1, None, None, None))]
    launches = g.stats()["launches"]
    for msg, args in table:
        with pytest.raises(BuffaloHipError, match=msg):
            g._call("fold_in", *args)
    assert np.array_equal(bits(g.device_tensor("fold", (n, g.get_vdim())).cpu().numpy()[:, :d]), bits(X))      # the earlier call's rows are still there
    empty = g.fold_in("user", np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32))
    assert g.stats()["launches"] == launches and empty[0].shape == (0, d) and g.device_buffer("fold") == (None, 0)
    bad, path = CyCFR(), H.write_opt(CC.opt(129, "llt"))
    try:
        with pytest.raises(BuffaloHipError, match="d > 128 is not supported"):
            bad.init(path)
    finally:
        os.unlink(path)
    # recommend: ascending unique keys per row (rows 0 .. 9 of the case and the short rows behind DUP), against TopK on the folded rows
    rows = [r for r in range(n) if r != 10]
    (ip, k, v), _ = cs.parts("user", rows)
    top = 10
    keys, scores = np.zeros((len(rows), top), np.int32), np.zeros((len(rows), top), np.float32)
    par.cfr_fold_in_recommend(g, ip, k, v, keys, scores, np.zeros(0, np.int32), top)
    X, _ = g.fold_in("user", ip, k, v)
    wk, ws = np.zeros_like(keys), np.zeros_like(scores)
    eng = par.TopK()
    eng.set_seen(ip, k, FC.N)
    eng.recommend_unseen(np.arange(len(rows), dtype=np.int32), X, arrs["item"], par.NO_BIAS, wk, ws, np.zeros(0, np.int32), top)
    assert np.array_equal(keys, wk) and np.array_equal(bits(scores), bits(ws))
