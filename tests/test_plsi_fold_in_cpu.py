"""The yardstick of the pLSI fold-in tests (plsi_fold_cases.fold_ref) checked without a GPU and without the library: against closed forms, its
float32 form against its float64 form inside the one-step bound over ten steps, and the same bound rejecting a float32 restatement with one
planted defect -- a bound that let those through would prove nothing on the device."""
import numpy as np
import pytest

import plsi_fold_cases as FC
import ref_plsi as R
from buffalo_amd.synth import CSR


def _one(keys, vals, items=FC.ITEMS):
    return CSR(1, items, np.array([len(keys)], dtype=np.int64), np.array(keys, dtype=np.int32), np.array(vals, dtype=np.float32))


def test_named_lengths_sit_on_the_kernel_paths():
    assert [FC.layout(d) for d in (1, 20, 32, 33, 128, 200, 300, 520)] == [(8, 1, 4), (8, 1, 4), (8, 1, 4), (16, 1, 4), (32, 1, 4), (64, 1, 4),
                                                                            (64, 2, 2), (64, 4, 2)]
    assert FC.named_lengths(20) == [0, 1, 16, 17, 3, 4, 5, 24, 32, 40, 2047, 2048, 2049, 4097]
    assert FC.named_lengths(200, empty=False) == [1, 3, 4, 5, 2047, 2048, 2049, 4097]          # G = 64: no short rows but the empty one
    m = FC.pattern(20)
    assert FC.lengths_of(m)[:14].tolist() == FC.named_lengths(20) and m.num_users <= 2000 and m.num_items == 300
    assert np.unique(m.keys[slice(*FC.rows_of(m)[13])]).shape[0] < 4097                          # keys repeat in the long rows


def test_d_one_gives_exactly_one():
    m = FC.pattern(1)
    P, Q = FC.start(m.num_users, 1)
    for dtype in (np.float64, np.float32):
        out, _ = FC.fold_ref(P, Q, m, 3, 1.0, dtype)
        assert (out == 1.0).all()


def test_one_entry_matches_the_two_line_formula():
    d, c, v, alpha1 = 7, 41, 3.0, 1.0
    P, Q = FC.start(5, d)
    p, q = P[2].astype(np.float64), Q[c].astype(np.float64)
    lat = np.maximum(p * q, np.float64(np.float32(1e-10)))
    acc = lat / lat.sum() * v + np.float64(np.float32(alpha1) / np.float32(d))
    out, loss = FC.fold_ref(P[[2]], Q, _one([c], [v]), 1, alpha1)
    np.testing.assert_allclose(out[0], acc / acc.sum(), rtol=1e-14)
    np.testing.assert_allclose(loss[0], -np.log(lat.sum()) * v, rtol=1e-14)


@pytest.mark.parametrize("alpha1", [1.0, 0.25, 0.0])
def test_empty_row_is_the_smoothing_alone(alpha1):
    d = 20
    _, Q = FC.start(5, d)
    for dtype in (np.float64, np.float32):
        out, loss = FC.fold_ref(None, Q, _one([], []), 4, alpha1, dtype)
        assert loss[0] == 0
        if alpha1 == 0:
            assert np.isnan(out).all()
        else:
            a1 = np.dtype(dtype).type(np.float32(alpha1) / np.float32(d))
            s = np.dtype(dtype).type(0)
            for _ in range(d):
                s = s + a1
            assert (out[0] == a1 / s).all()


def _ten_steps(d, alpha1=1.0, empty=True):
    """(float32 input, float32 step, float64 step) for ten steps of the float64 run over the pattern of d."""
    m = FC.pattern(d, empty=empty)
    P, Q = FC.start(m.num_users, d)
    P64 = P.astype(np.float64)
    for _ in range(10):
        x = P64.astype(np.float32)
        P64 = FC.step(x, Q, m, alpha1, np.float64)
        yield m, Q, x, P64


@pytest.mark.parametrize("d", [7, 20, 128])
def test_float32_restatement_is_inside_the_one_step_bound(d):
    worst = 0.0
    for m, Q, x, f64 in _ten_steps(d):
        worst = max(worst, FC.ratio(FC.step(x, Q, m, 1.0, np.float32), f64, FC.one_step_bound(m, d)))
    print("d=%d: float32 restatement uses %.3f of bound_normalized(n_b, d, d) over 10 steps" % (d, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("defect", FC.DEFECTS)
def test_the_bound_rejects_a_planted_defect(defect):
    """Each defect sits in ONE named row (the 17-entry team row, or for the clamp a row whose start holds a tiny factor) and must push exactly
    that row out of the bound.  The clamp moves a sum by 1e-10 / norm per entry, far below a smoothing term of 1 / d: it is planted under alpha1 = 0."""
    d = 20
    alpha1, empty = (0.0, False) if defect == "skip_clamp" else (1.0, True)
    m, Q, x, f64 = next(iter(_ten_steps(d, alpha1, empty)))
    lengths = FC.lengths_of(m)
    if defect == "skip_clamp":
        hit = (x[R.entry_rows(m)].astype(np.float64) * Q[m.keys] < 1e-10).any(axis=1)
        row = int(np.flatnonzero(np.bincount(R.entry_rows(m), weights=hit, minlength=m.num_users))[0])
    else:
        row = int(np.flatnonzero(lengths == 17)[0])
    bound = FC.one_step_bound(m, d)
    good = FC.step(x, Q, m, alpha1, np.float32)
    bad = FC.step(x, Q, m, alpha1, np.float32, defect, row)
    others = np.arange(m.num_users) != row
    assert FC.ratio(good, f64, bound) <= 1.0
    assert FC.ratio(bad[others], f64[others], bound[others]) <= 1.0
    assert FC.ratio(bad[[row]], f64[[row]], bound[[row]]) > 1.0, defect


def test_clamp_is_reached_from_the_clamped_start_and_never_from_the_uniform_one():
    for d in (1, 7, 20, 32, 33, 128, 200, 300):
        m = FC.pattern(d)
        P, Q = FC.start(m.num_users, d)
        assert FC.clamp_is_reached(P, Q, m), d
        assert not FC.clamp_is_reached(FC.uniform(m.num_users, d), Q, m), d
