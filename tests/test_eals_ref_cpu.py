"""The float64 eALS yardstick (tests/ref_eals.py) held to the oracle and to the objective, and proof that the device bound built on
it has teeth.  The oracle is itself held to the reference's compiled eals.cc by test_oracle_vs_reference_sources.py, so this
chains the yardstick to the reference.

Measured (relerr of the oracle's factors against the yardstick, per step; profiles/eals_parity.txt): 1e-7 .. 3e-6 after a
half-epoch or one epoch on every case (`many`: 3.0e-6); after the second free-running epoch the largest are 6.8e-6 (pattern("user"),
d = 17: the 4,000 .. 6,000-entry rows summed in one running float) and 5.9e-6 (`many`), inside the bound 1e-5."""
import numpy as np
import pytest

import eals_cases as EC
import helpers as H
from ref_eals import DEFECTS, F64EALS, bound, relerr

YARDSTICK_CASES = [("pattern_user", 1), ("pattern_user", 17), ("pattern_user", 72), ("pattern_item", 1), ("pattern_item", 17), ("pattern_item", 72),
                   ("tiny", 20), ("empty_rows", 20), ("many", 16)]


@pytest.mark.parametrize("name,d", YARDSTICK_CASES)
def test_yardstick_follows_the_oracle(name, d):
    orc, f64 = EC.references(name, d, EC.HALVES_THEN_2_EPOCHS)
    lines, worst = [], 0.0
    for o, f in zip(orc, f64):
        eP, eQ = relerr(o.P, f.P), relerr(o.Q, f.Q)
        worst = max(worst, eP, eQ)
        lines.append("step %d update(%d): err(oracle, f64) P %.3g Q %.3g; loss oracle %.9g f64 %.12g" % (o.step, o.axis, eP, eQ, o.loss[o.axis], f.loss[f.axis]))
    EC.record("cpu yardstick vs oracle, %s d=%d" % (name, d), lines + ["largest %.3g (bound 1e-5)" % worst])
    assert worst <= 1e-5, lines


def test_yardstick_loss_is_the_objective_and_falls():
    d = 20
    csr, P, Q, Cw = prob = EC.problem("tiny", d)
    t = csr.transpose()
    f = F64EALS()
    assert f.init(H.write_opt(EC.opt(d)))
    assert not f.update(csr.indptr, csr.keys, csr.vals, 0) and f.estimate_loss(csr.nnz, csr.indptr, csr.keys, csr.vals, 0) == (0.0, 0.0)
    EC.bind(f, prob)
    losses = [f.estimate_loss(csr.nnz, csr.indptr, csr.keys, csr.vals, 0)[1]]
    assert abs(losses[0] - f.dense_loss(csr.indptr, csr.keys, csr.vals)) <= 1e-12 * losses[0]
    for _ in range(5):
        for axis, m in ((0, csr), (1, t)):
            assert f.update(m.indptr, m.keys, m.vals, axis)
            l0, l1 = f.estimate_loss(csr.nnz, csr.indptr, csr.keys, csr.vals, 0)[1], f.estimate_loss(csr.nnz, t.indptr, t.keys, t.vals, 1)[1]
            want = f.dense_loss(csr.indptr, csr.keys, csr.vals)
            assert abs(l0 - want) <= 1e-12 * want and abs(l1 - want) <= 1e-12 * want, (l0, l1, want)
            assert l0 <= losses[-1], (losses, l0)       # exact coordinate minimisation never goes up
            losses.append(l0)
            scale = np.abs(f.vhat[0]).max()
            assert np.abs(f.vhat[1][f.map[0]] - f.vhat[0]).max() <= 1e-12 * scale
            assert np.abs(f.vhat[0][f.map[1]] - f.vhat[1]).max() <= 1e-12 * scale
    assert losses[-1] < 0.5 * losses[0]


@pytest.mark.parametrize("d", [24, 17])
def test_the_device_bound_has_teeth(d):
    """One wrong entry in one dimension of a 4,300-entry row moves the factors by far more than the envelope allows."""
    orc, f64 = EC.references("heavy", d, EC.ONE_EPOCH)
    prob = EC.problem("heavy", d)
    allowed = bound(relerr(orc[1].Q, f64[1].Q))        # the device bound on Q after update(0), update(1)
    lines = ["err(oracle, f64) %.3g -> device bound %.3g" % (relerr(orc[1].Q, f64[1].Q), allowed)]
    moved = {}
    for defect in DEFECTS:
        bad = EC.run(lambda: F64EALS(defect=defect), d, prob, EC.ONE_EPOCH, losses=False)
        assert np.array_equal(bad[0].P, f64[0].P)      # the 12-entry user rows are below the defect's row length
        moved[defect] = relerr(bad[1].Q, f64[1].Q)
        lines.append("%s moves Q by %.3g = %.0f x bound" % (defect, moved[defect], moved[defect] / allowed))
    EC.record("cpu teeth, heavy d=%d" % d, lines)
    assert all(m > 10 * allowed for m in moved.values()), lines
