"""bfh_eals_fold_in on the device against the float64 restatement of its rule (tests/eals_fold_cases.py); the measured figures are in
profiles/eals_fold_in_parity.txt."""
import ctypes as C

import numpy as np
import pytest

import eals_cases as EC
import eals_fold_cases as FC
import helpers as H
from ref_eals import bound, relerr

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("with_init", [False, True])
@pytest.mark.parametrize("d", [20, 64, 128])
def test_class_edges_inside_the_envelope(d, with_init):
    init, cmp_run, f64 = FC.references(d, with_init)
    g, _, _ = FC.make_hip(d, *FC.model(d))
    ip, k, v = FC.pattern(d)
    X = g.fold_in(ip, k, v, 3, init=init)
    assert X.shape == (ip.shape[0], d) and (with_init or not X[0].any())          # the empty history stays the zero row from a zero start
    FC.hold("fold_in d=%d init=%s iters=3" % (d, "random" if with_init else "none"), X, cmp_run, f64, FC.named_lengths(d))
    rows, n = g.device_buffer("fold")
    assert rows and n == ip.shape[0] * FC.vdim_of(d) * 4
    dev = g.device_tensor("fold", (ip.shape[0], FC.vdim_of(d))).cpu().numpy()
    assert np.array_equal(bits(dev[:, :d]), bits(X)) and not dev[:, d:].any()
    assert np.array_equal(bits(g.fold_in(ip, k, v, 0, init=init)), bits(np.zeros_like(X) if init is None else init))      # iters == 0


def test_fixed_point_is_the_closed_form_solve():
    d, (_, Q, Cw) = 20, FC.model(20)
    ip, k, v = FC.csr_of([257, 1025], 3)
    g, _, _ = FC.make_hip(d, *FC.model(d))
    X = g.fold_in(ip, k, v, 30)
    want = np.stack([FC.solve(Q, Cw, k[b:e], v[b:e]) for b, e in FC.rows_of(ip)])
    FC.hold("fold_in d=20 iters=30 against the closed form", X, FC.fold(Q, Cw, ip, k, v, 30, None, np.float32), want, (257, 1025))


def test_a_row_does_not_depend_on_its_batch():
    d = 64
    ip, k, v = FC.pattern(d)
    bounds = FC.rows_of(ip)
    g, _, _ = FC.make_hip(d, *FC.model(d))
    whole = g.fold_in(ip, k, v, 2)
    single = np.concatenate([g.fold_in(np.array([e - b], np.int64), k[b:e].copy(), v[b:e].copy(), 2) for b, e in bounds])
    assert np.array_equal(bits(whole), bits(single))
    # reversed, and with a scratch bound of 4,000 entries: the 256-thread streamed class (4,096 and 244 entries, one launch above) is cut in two
    g2, _, _ = FC.make_hip(d, *FC.model(d), fold_scratch_bytes=18 * 4 * 4000)
    rk, rv = (np.concatenate([a[b:e] for b, e in bounds[::-1]]) for a in (k, v))
    back = g2.fold_in(np.cumsum([e - b for b, e in bounds[::-1]], dtype=np.int64), rk, rv, 2)[::-1]
    assert np.array_equal(bits(whole), bits(back))


def test_sweeps_compose():
    d = 20
    _, cmp_run, f64 = FC.references(d, False, 2)
    g, _, _ = FC.make_hip(d, *FC.model(d))
    ip, k, v = FC.pattern(d)
    FC.hold("fold_in d=20 iters=2", g.fold_in(ip, k, v, 2), cmp_run, f64, FC.named_lengths(d))
    FC.hold("fold_in d=20 iters=1 twice", g.fold_in(ip, k, v, 1, init=g.fold_in(ip, k, v, 1)), cmp_run, f64, FC.named_lengths(d))


def test_training_does_not_notice_and_the_gramian_follows_Q():
    from buffalo_amd.backend import CyEALS
    d = 20
    prob = EC.problem("tiny", d)
    csr, runs = prob[0], []
    for with_folds in (False, True):
        g = CyEALS()
        assert g.init(H.write_opt(EC.opt(d)))
        P, Q = EC.bind(g, prob)
        fold = (lambda: g.fold_in(csr.indptr, csr.keys, csr.vals, 2)) if with_folds else (lambda: None)
        fold()
        s0 = EC.step(g, prob, 0, P, Q)
        fold()
        s1 = EC.step(g, prob, 1, P, Q)
        runs.append((s0, s1))
    for a, b in zip(*runs):
        assert np.array_equal(bits(a.P), bits(b.P)) and np.array_equal(bits(a.Q), bits(b.Q)) and a.loss == b.loss
    # the handle of the second run has folded before update(1): the next call must see the new Q
    X = g.fold_in(csr.indptr, csr.keys, csr.vals, 2)
    args = (Q, prob[3], csr.indptr, csr.keys, csr.vals, 2, None)
    f64 = FC.fold(*args, np.float64)
    FC.hold("fold_in d=20 after update(1)", X, FC.fold(*args, np.float32), f64)
    assert relerr(X, FC.fold(prob[2], *args[1:], np.float64)) > 100 * bound(0.0)      # ... and not the Q it started from


def test_refusals_launch_nothing():
    from buffalo_amd.backend import BuffaloHipError, CyEALS
    d = 20
    ip, k, v = FC.csr_of([3, 0, 2], 1)
    g = CyEALS()
    assert g.init(H.write_opt(EC.opt(d)))
    with pytest.raises(BuffaloHipError, match="before initialize_model"):
        g.fold_in(ip, k, v, 1)
    g, n = FC.make_hip(d, *FC.model(d))[0], ip.shape[0]
    table = [("n_rows is negative", (-1, ip, k, v, 5, 1)), ("iters is negative", (n, ip, k, v, 5, -1)),
             ("indptr decreases at row 1", (n, np.array([3, 2, 5], np.int64), k, v, 5, 1)), (r"indptr\[n_rows - 1\] != nnz", (n, ip, k, v, 4, 1)),
             ("null keys / vals", (n, ip, None, None, 5, 1)), (r"key 6000 at position 4 is outside \[0, 6000\)", (n, ip, np.array([0, 1, 2, 3, 6000], np.int32), v, 5, 1)),
             (r"key -1 at position 0", (n, ip, np.array([-1, 1, 2, 3, 4], np.int32), v, 5, 1))]
    launches = g.stats()["launches"]
    for msg, (rows, a, b, c, nnz, iters) in table:
        ptr = [None if x is None else x.ctypes.data_as(C.POINTER(t)) for x, t in zip((a, b, c), (C.c_int64, C.c_int32, C.c_float))]
        with pytest.raises(BuffaloHipError, match=msg):
            g._call("fold_in", rows, ptr[0], ptr[1], ptr[2], nnz, iters, None, None)
    assert g.fold_in(np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32), 1).shape == (0, d)
    assert g.stats()["launches"] == launches and g.device_buffer("fold") == (None, 0)
    with pytest.raises(BuffaloHipError, match="unknown device buffer"):
        g.device_buffer("P")
    assert g.get_vdim() == 32 and g.dim() == d and g.device_buffer("Q")[1] == FC.ITEMS * 32 * 4


def test_recommend_from_the_folded_rows():
    from buffalo_amd import parallel as par
    d, k = 20, 10
    rng = np.random.default_rng(7)
    P, Q = (rng.normal(scale=0.3, size=(r, d)).astype(np.float32) for r in (2, 300))
    Cw = np.full(300, 0.5 / 300, np.float32)
    lens = rng.integers(0, 40, size=200)
    keys = np.concatenate([np.sort(rng.choice(300, size=n, replace=False)) for n in lens]).astype(np.int32)
    vals = (1 + rng.poisson(1.0, size=keys.shape[0])).astype(np.float32)
    ip = np.cumsum(lens, dtype=np.int64)
    g, _, _ = FC.make_hip(d, P, Q, Cw)
    out_keys, out_scores = np.zeros((200, k), np.int32), np.zeros((200, k), np.float32)
    par.eals_fold_in_recommend(g, ip, keys, vals, 3, out_keys, out_scores, np.zeros(0, np.int32), k)
    X = g.fold_in(ip, keys, vals, 3)
    for b, (beg, end) in enumerate(FC.rows_of(ip)):
        pool = np.setdiff1d(np.arange(300, dtype=np.int32), keys[beg:end]).astype(np.int32)
        wk, ws = np.zeros((1, k), np.int32), np.zeros((1, k), np.float32)
        par.dot_topn(np.array([b], np.int32), X, Q, par.NO_BIAS, wk, ws, pool, k)
        assert np.array_equal(out_keys[b], wk[0]), b
