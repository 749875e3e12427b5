"""Pins tests/ref_plsi.py, the numpy restatement of the reference's pLSI epoch that the device tests are measured against (no GPU):
a closed form on a 3 x 2 example, the normalisation, EM's monotone loss, and the float32 one-worker arithmetic against float64."""
import math

import numpy as np

import ref_plsi as R
from buffalo_amd.synth import CSR


def _hand():
    # users x items = 3 x 2, d = 2; entries (0,0,2) (0,1,1) (1,1,3) (2,0,1)
    csr = CSR(3, 2, np.array([2, 3, 4]), np.array([0, 1, 1, 0]), np.array([2.0, 1.0, 3.0, 1.0]))
    P = np.array([[0.25, 0.75], [0.5, 0.5], [0.125, 0.875]], dtype=np.float32)
    Q = np.array([[0.5, 0.25], [0.5, 0.75]], dtype=np.float32)
    return csr, P, Q


def test_float64_epoch_equals_the_closed_form_on_a_hand_example():
    csr, P, Q = _hand()
    Pn = [[0.0, 0.0] for _ in range(3)]
    Qn = [[0.0, 0.0] for _ in range(2)]
    loss = 0.0
    for x, c, v in ((0, 0, 2.0), (0, 1, 1.0), (1, 1, 3.0), (2, 0, 1.0)):
        lat = [float(P[x, k]) * float(Q[c, k]) for k in range(2)]     # all far above the clamp
        norm = lat[0] + lat[1]
        loss -= math.log(norm) * v
        for k in range(2):
            Pn[x][k] += lat[k] / norm * v
            Qn[c][k] += lat[k] / norm * v
    a1, a2 = 1.0 / 2, 1.0 / 2                                          # alpha / d, alpha / num_items
    Pe = [[(p + a1) / (row[0] + row[1] + 2 * a1) for p in row] for row in Pn]
    col = [Qn[0][k] + Qn[1][k] + 2 * a2 for k in range(2)]
    Qe = [[(row[k] + a2) / col[k] for k in range(2)] for row in Qn]
    raw = R.accumulate(P, Q, csr, np.float64)
    np.testing.assert_allclose(raw[0], Pn, rtol=1e-14)
    np.testing.assert_allclose(raw[1], Qn, rtol=1e-14)
    # spot values by hand: entry (0,0,2): lat = (1/8, 3/16), norm = 5/16 -> P[0] gets (0.8, 1.2); entry (0,1,1): lat = (1/8, 9/16) -> (2/11, 9/11)
    np.testing.assert_allclose(raw[0][0], [0.8 + 2 / 11, 1.2 + 9 / 11], rtol=1e-14)
    P1, Q1, l1 = R.epoch(P, Q, csr, 1.0, 1.0, np.float64)
    np.testing.assert_allclose(P1, Pe, rtol=1e-14)
    np.testing.assert_allclose(Q1, Qe, rtol=1e-14)
    assert abs(l1 - loss) <= 1e-14 * abs(loss)


def test_the_clamp_is_applied_per_factor_and_enters_the_norm():
    csr = CSR(1, 1, np.array([1]), np.array([0]), np.array([1.0]))
    P = np.array([[1e-7, 1.0]], dtype=np.float32)
    Q = np.array([[1e-6, 0.5]], dtype=np.float32)
    Pn, _, loss = R.accumulate(P, Q, csr, np.float64)
    c = float(R.CLAMP)
    np.testing.assert_allclose(Pn[0], [c / (c + 0.5), 0.5 / (c + 0.5)], rtol=1e-14)
    assert abs(loss + math.log(c + 0.5)) < 1e-14


def test_rows_of_p_and_columns_of_q_sum_to_one_after_normalize():
    csr = R.skewed_case(200, 60, seed=2, empty=True)
    P, Q = R.init_model(200, 60, 7, seed=1)
    for dtype, tol in ((np.float64, 1e-13), (np.float32, 60 * R.U24)):
        P1, Q1, _ = R.epoch(P, Q, csr, 1.0, 1.0, dtype)
        assert np.abs(P1.sum(axis=1, dtype=np.float64) - 1).max() <= tol
        assert np.abs(Q1.sum(axis=0, dtype=np.float64) - 1).max() <= tol
        np.testing.assert_allclose(P1[3], 1.0 / 7, rtol=1e-6)     # a user without entries: alpha1 / d over alpha1


def test_training_loss_does_not_increase_without_smoothing():
    """EM's guarantee (alpha1 = alpha2 = 0, no empty rows); with smoothing the update is no longer the exact M-step, so nothing is asserted there."""
    csr = R.skewed_case(120, 40, seed=3)
    P, Q = R.init_model(120, 40, 5, seed=4)
    P, Q = P.astype(np.float64), Q.astype(np.float64)
    losses = []
    for _ in range(10):
        P, Q, loss = R.epoch(P, Q, csr, 0.0, 0.0, np.float64)
        losses.append(loss)
    assert all(b <= a * (1 + 1e-12) for a, b in zip(losses, losses[1:])), losses
    assert losses[-1] < losses[0]


def test_float32_one_worker_arithmetic_stays_inside_the_bound():
    """The bound the device is held to, (n + d + 6) 2^-24, holds for the reference's own sequential float32 arithmetic with room to spare
    (1500 x 300, 15 % dense, five 90 %-dense columns, d = 20, values 1..5, a start with products below the clamp)."""
    d = 20
    csr = R.skewed_case()
    P, Q = R.clamped_start(1500, 300, d, seed=11)
    rows = R.entry_rows(csr)
    assert (P[rows].astype(np.float64) * Q[csr.keys] < 1e-10).any()
    n_row, n_col = R.entry_counts(csr)
    for ep in range(3):
        P64, Q64, l64 = R.accumulate(P, Q, csr, np.float64)
        P32, Q32, l32 = R.accumulate(P, Q, csr, np.float32)
        with np.errstate(invalid="ignore", divide="ignore"):
            rp = np.nan_to_num(np.abs(P32 - P64) / P64) / R.bound_raw(n_row, d)[:, None]
            rq = np.nan_to_num(np.abs(Q32 - Q64) / Q64) / R.bound_raw(n_col, d)[:, None]
        print("epoch %d: float32 / bound  P %.3f  Q %.3f  loss relerr %.2e" % (ep, rp.max(), rq.max(), abs(l32 - l64) / abs(l64)))
        assert rp.max() <= 1.0 and rq.max() <= 1.0
        assert abs(l32 - l64) / abs(l64) < 1e-4
        N64, M64 = R.normalize(P64, Q64, 1.0, 1.0, np.float64)
        N32, M32 = R.normalize(P32, Q32, 1.0, 1.0, np.float32)
        assert (np.abs(N32 - N64) / N64 <= R.bound_normalized(n_row, d, d)[:, None]).all()
        assert (np.abs(M32 - M64) / M64 <= R.bound_normalized(n_col, d, 300)[:, None]).all()
        P, Q = N32, M32
