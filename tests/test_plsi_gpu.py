"""pLSI on the device (csrc/plsi.hip behind bfh_plsi_* / CyPLSI) against the float64 restatement of the reference's epoch (tests/ref_plsi.py).

Bounds are derived, not tuned.  One epoch from identical inputs: every accumulator element within (n + d + 6) 2^-24 relative of float64, n = entries
of that row (P) or column (Q) -- the forward error of a sum of n non-negative terms of d + 5 roundings each, valid for ANY summation order; after
normalize + swap (n + d + m + 10) 2^-24, m = d for P and rows of Q for Q.  Loss: relative error no larger than max(e32, (d + 8) 2^-24), e32 = the
error of the reference's own one-worker float32 arithmetic on the same case.  Free-running epochs: e_hip <= max(2.5 e32, the one-epoch bound).
With alpha1 = 0 a row without entries is 0 / 0 in the reference and NaN on the device as well, so alpha = 0 is run on matrices without empty rows."""
import os

import numpy as np
import pytest

import helpers as H
import ref_plsi as R

pytestmark = pytest.mark.gpu


def _opt(d, seed=0):
    return H.write_opt({"d": d, "random_seed": seed, "num_workers": 1, "num_iters": 10, "alpha1": 1.0, "alpha2": 1.0, "eps": 1e-10})


def _obj(d, P=None, Q=None, seed=0):
    from buffalo_amd.backend import CyPLSI
    g = CyPLSI()
    path = _opt(d, seed)
    assert g.init(path)
    os.unlink(path)
    if P is not None:
        g.set_mode("keep_init", 1)
        g.initialize_model(P, Q)
    return g


def _feed(g, csr, n_batches=1):
    """reset + the batches of one epoch; returns the per-batch losses."""
    g.reset()
    losses = []
    for a, b in H.chunks_of(csr, n_batches):
        keys, vals = H.chunk_arrays(csr, a, b)
        losses.append(g.partial_update(a, b, csr.indptr, keys, vals))
    return losses


def _uneven(csr, n):
    """n uneven consecutive row ranges."""
    if n <= 1:
        return [(0, csr.num_users)]
    w = np.arange(1, n + 1, dtype=np.float64) ** 2
    edges = np.concatenate([[0], np.round(np.cumsum(w) / w.sum() * csr.num_users)]).astype(int)
    return [(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:]) if b > a]


def _raw(g, d, shape_p, shape_q):
    vdim = g.get_vdim()
    Pn = g.device_tensor("P_new", (shape_p[0], vdim)).cpu().numpy()[:, :d].copy()
    Qn = g.device_tensor("Q_new", (shape_q[0], vdim)).cpu().numpy()[:, :d].copy()
    return Pn, Qn


def _ratio(a, ref, bound):
    """Largest elementwise |a - ref| / (|ref| * bound); 0 / 0 counts as 0, a non-finite device value as inf."""
    a, ref = a.astype(np.float64), ref.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(a - ref) / (np.abs(ref) * bound)
    r[a == ref] = 0.0
    r[~np.isfinite(r)] = np.inf
    return float(r.max())


def _one_epoch_checks(csr, d, P0, Q0, alpha=(1.0, 1.0), n_batches=1, label=""):
    P, Q = P0.copy(), Q0.copy()
    g = _obj(d, P, Q)
    g.set_mode("raw_accumulators", 1)
    losses = _feed(g, csr, n_batches)
    g.normalize(*alpha)
    Pn, Qn = _raw(g, d, P.shape, Q.shape)
    P64, Q64, l64 = R.accumulate(P0, Q0, csr, np.float64)
    _, _, l32 = R.accumulate(P0, Q0, csr, np.float32)
    n_row, n_col = R.entry_counts(csr)
    rp = _ratio(Pn, P64, R.bound_raw(n_row, d)[:, None])
    rq = _ratio(Qn, Q64, R.bound_raw(n_col, d)[:, None])
    e32, e_hip = abs(l32 - l64) / abs(l64), abs(float(np.sum(np.array(losses, dtype=np.float64))) - l64) / abs(l64)
    print("%s d=%d raw: error / bound P %.3f Q %.3f; loss relerr hip %.2e float32 %.2e" % (label, d, rp, rq, e_hip, e32))
    assert rp <= 1.0 and rq <= 1.0, (rp, rq)
    assert (Pn[n_row == 0] == 0).all() and (Qn[n_col == 0] == 0).all()      # empty owners: a zero accumulator
    assert e_hip <= max(e32, (d + 8) * R.U24), (e_hip, e32)
    g.set_mode("raw_accumulators", 0)
    g.normalize(*alpha)
    g.swap()
    N64, M64 = R.normalize(P64, Q64, alpha[0], alpha[1], np.float64)
    np_, nq = _ratio(P, N64, R.bound_normalized(n_row, d, d)[:, None]), _ratio(Q, M64, R.bound_normalized(n_col, d, Q.shape[0])[:, None])
    print("%s d=%d normalised: error / bound P %.3f Q %.3f" % (label, d, np_, nq))
    assert np_ <= 1.0 and nq <= 1.0, (np_, nq)
    return P, Q, losses, g


@pytest.mark.parametrize("d", [1, 7, 20, 32, 33, 128, 200])
def test_one_epoch_against_float64(d):
    csr = R.skewed_case(empty=True)
    P0, Q0 = R.clamped_start(1500, 300, d, seed=11)
    if d > 1:
        assert (P0[R.entry_rows(csr)].astype(np.float64) * Q0[csr.keys] < 1e-10).any()     # the clamp is exercised
    _one_epoch_checks(csr, d, P0, Q0, label="skewed+empty")


@pytest.mark.parametrize("values", ["counts", "ones"])
@pytest.mark.parametrize("alpha", [(0.0, 0.0), (1.0, 1.0), (0.0, 1.0)])
def test_alpha_and_value_kinds(values, alpha):
    csr = R.skewed_case(600, 200, seed=9, values=values)          # no empty rows: alpha1 = 0 would be 0 / 0 there
    P0, Q0 = R.clamped_start(600, 200, 20, seed=3)
    _one_epoch_checks(csr, 20, P0, Q0, alpha=alpha, label="%s alpha=%s" % (values, alpha))


def test_empty_row_with_alpha1_zero_is_nan_as_in_the_reference():
    csr = R.skewed_case(200, 60, seed=2, empty=True)
    P, Q = R.init_model(200, 60, 20, seed=1)
    g = _obj(20, P, Q)
    _feed(g, csr)
    g.normalize(0.0, 1.0)
    g.swap()
    assert np.isnan(P[3]).all() and np.isnan(P[4]).all() and np.isfinite(np.delete(P, [3, 4], axis=0)).all()
    assert np.isfinite(Q).all()


@pytest.mark.parametrize("d", [20, 128])
def test_batches_and_resident_give_the_same_bits(d):
    csr = R.skewed_case(empty=True)
    P0, Q0 = R.clamped_start(1500, 300, d, seed=11)
    P1, Q1, l1, _ = _one_epoch_checks(csr, d, P0, Q0, label="one batch")
    l64 = R.accumulate(P0, Q0, csr, np.float64)[2]
    e32 = abs(R.accumulate(P0, Q0, csr, np.float32)[2] - l64) / abs(l64)
    for n in (3, 7):
        P, Q = P0.copy(), Q0.copy()
        g = _obj(d, P, Q)
        g.reset()
        losses = []
        for a, b in _uneven(csr, n):
            keys, vals = H.chunk_arrays(csr, a, b)
            losses.append(g.partial_update(a, b, csr.indptr, keys, vals))
        assert len(losses) == n
        g.normalize(1.0, 1.0)
        g.swap()
        assert P.tobytes() == P1.tobytes() and Q.tobytes() == Q1.tobytes(), n
        e = abs(float(np.sum(np.array(losses, dtype=np.float64))) - l64) / abs(l64)
        assert e <= max(e32, (d + 8) * R.U24), (n, e, e32)
    P, Q = P0.copy(), Q0.copy()
    g = _obj(d, P, Q)
    g.set_resident_csr(csr.indptr, csr.keys, csr.vals)
    g.reset()
    loss = g.update_resident()
    g.normalize(1.0, 1.0)
    g.swap()
    assert P.tobytes() == P1.tobytes() and Q.tobytes() == Q1.tobytes()
    assert loss == l1[0]
    from buffalo_amd._lib import BuffaloHipError
    with pytest.raises(BuffaloHipError, match="resident"):
        g.reset()
        g.partial_update(0, csr.num_users, csr.indptr, csr.keys, csr.vals)


def test_long_column_and_long_row_take_the_split_path():
    """A column of > 50 000 entries and a row of > 4 000: owners cut into segments over several waves, summed from partial rows in segment order."""
    from buffalo_amd.synth import CSR
    U, I, d = 52000, 4200, 20
    rng = np.random.default_rng(4)
    r = [np.arange(U), np.zeros(4100, dtype=np.int64), np.repeat(np.arange(U), 2)]
    c = [np.zeros(U, dtype=np.int64), np.arange(1, 4101), rng.integers(1, I, size=2 * U)]
    key = np.unique(np.concatenate(r) * I + np.concatenate(c))
    rows, cols = key // I, (key % I).astype(np.int32)
    vals = rng.integers(1, 6, size=key.shape[0]).astype(np.float32)
    csr = CSR(U, I, np.cumsum(np.bincount(rows, minlength=U), dtype=np.int64), cols, vals)
    n_row, n_col = R.entry_counts(csr)
    assert n_col.max() > 50000 and n_row.max() > 4000
    P0, Q0 = R.clamped_start(U, I, d, seed=8)
    _, _, _, g = _one_epoch_checks(csr, d, P0, Q0, label="split", n_batches=3)
    st = g.get_stats()
    # per epoch: the long row in the P half-step, the long column in the Q half-step -- each run twice here (raw + normalised pass of the Q side)
    assert st["merges"] >= 2, st
    assert st["samples"] == csr.nnz


def test_five_free_epochs_reproducible_and_close_to_float64():
    d = 20
    csr = R.skewed_case()
    P0, Q0 = R.clamped_start(1500, 300, d, seed=11)
    runs = []
    for _ in range(2):
        P, Q = P0.copy(), Q0.copy()
        g = _obj(d, P, Q)
        for _ in range(5):
            _feed(g, csr, 2)
            g.normalize(1.0, 1.0)
            g.swap()
        runs.append((P.copy(), Q.copy()))
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()
    P64, Q64 = P0.astype(np.float64), Q0.astype(np.float64)
    P32, Q32 = P0.copy(), Q0.copy()
    for _ in range(5):
        P64, Q64, _ = R.epoch(P64, Q64, csr, 1.0, 1.0, np.float64)
        P32, Q32, _ = R.epoch(P32, Q32, csr, 1.0, 1.0, np.float32)
    n_row, n_col = R.entry_counts(csr)
    for name, hip, f32, f64, floor in (("P", runs[0][0], P32, P64, float(R.bound_normalized(n_row.max(), d, d))),
                                       ("Q", runs[0][1], Q32, Q64, float(R.bound_normalized(n_col.max(), d, 300)))):
        e32, e_hip = R.relerr_elements(f32, f64), R.relerr_elements(hip, f64)
        print("%s after 5 free epochs (1500 x 300, d = 20): e_hip %.3e  e32 %.3e  one-epoch bound %.3e" % (name, e_hip, e32, floor))   # first run: profiles/plsi_first_contact.txt
        assert e_hip <= max(2.5 * e32, floor), (name, e_hip, e32, floor)


def test_initialize_model_fills_a_seeded_random_start():
    d, U, I = 20, 400, 150

    def start(seed):
        P, Q = np.zeros((U, d), dtype=np.float32), np.zeros((I, d), dtype=np.float32)
        g = _obj(d, seed=seed)
        g.initialize_model(P, Q)
        vdim = g.get_vdim()
        assert (g.device_tensor("P", (U, vdim)).cpu().numpy()[:, :d] == P).all()       # uploaded what it wrote
        assert (g.device_tensor("Q", (I, vdim)).cpu().numpy()[:, :d] == Q).all()
        return P, Q
    P, Q = start(5)
    assert (P >= 0).all() and (Q >= 0).all()
    assert np.abs(P.sum(axis=1, dtype=np.float64) - 1).max() <= d * R.U24
    assert np.abs(Q.sum(axis=0, dtype=np.float64) - 1).max() <= I * R.U24
    assert (P.max(axis=1) > P.min(axis=1)).all() and (Q.max(axis=0) > Q.min(axis=0)).all()    # random, not 1 / d
    P2, Q2 = start(5)
    assert P.tobytes() == P2.tobytes() and Q.tobytes() == Q2.tobytes()
    P3, Q3 = start(6)
    assert P.tobytes() != P3.tobytes() and Q.tobytes() != Q3.tobytes()


def test_errors_have_a_status_and_a_message():
    from buffalo_amd._lib import BuffaloHipError
    from buffalo_amd.backend import CyPLSI
    csr = R.skewed_case(100, 40, seed=1)
    P, Q = R.init_model(100, 40, 8, seed=1)
    for bad_d in (0, -3):
        path = _opt(bad_d)
        with pytest.raises(BuffaloHipError, match="d must be"):
            CyPLSI().init(path)
    assert CyPLSI().init("/nonexistent/opt.json") is False
    g = _obj(8)
    with pytest.raises(BuffaloHipError, match="before initialize_model"):
        g.partial_update(0, 100, csr.indptr, csr.keys, csr.vals)
    with pytest.raises(BuffaloHipError, match="before initialize_model"):
        g.normalize(1.0, 1.0)
    g.set_mode("keep_init", 1)
    g.initialize_model(P, Q)
    with pytest.raises(BuffaloHipError, match="reset"):
        g.partial_update(0, 100, csr.indptr, csr.keys, csr.vals)
    g.reset()
    with pytest.raises(BuffaloHipError, match="no batch seen"):
        g.normalize(1.0, 1.0)
    with pytest.raises(BuffaloHipError, match="bad row range"):
        g.partial_update(0, 101, csr.indptr, csr.keys, csr.vals)
    bad = csr.keys.copy()
    bad[5] = 40
    with pytest.raises(BuffaloHipError, match="keys outside"):
        g.partial_update(0, 100, csr.indptr, bad, csr.vals)
    with pytest.raises(BuffaloHipError, match="before set_resident_csr"):
        g.update_resident()
    with pytest.raises(BuffaloHipError, match="unknown mode"):
        g.set_mode("no_such_mode", 1)
    with pytest.raises(BuffaloHipError, match="unknown device buffer"):
        g.device_buffer("R")
    # the handle is still usable: a clean epoch equals the restatement
    g.reset()
    a, b = H.chunks_of(csr, 2)
    g.partial_update(a[0], a[1], csr.indptr, *H.chunk_arrays(csr, *a))
    with pytest.raises(BuffaloHipError, match="consecutive"):
        g.partial_update(a[0], a[1], csr.indptr, *H.chunk_arrays(csr, *a))
    g.partial_update(b[0], b[1], csr.indptr, *H.chunk_arrays(csr, *b))
    g.normalize(1.0, 1.0)
    g.swap()
    P64, Q64, _ = R.epoch(R.init_model(100, 40, 8, seed=1)[0], R.init_model(100, 40, 8, seed=1)[1], csr, 1.0, 1.0, np.float64)
    np.testing.assert_allclose(P, P64, rtol=1e-4)
    np.testing.assert_allclose(Q, Q64, rtol=1e-4)
