"""The float64 CFR yardstick (tests/ref_cfr.py) held to the oracle and to a dense restatement of the item update, and proof that
the device bound built on it has teeth.  The oracle is itself held to the reference's compiled cfr.cc by
test_oracle_vs_reference_sources.py, so this chains the yardstick to the reference.

Measured (relerr of the oracle's arrays against the yardstick, every array of every step; profiles/cfr_parity.txt): single steps
from a shared float32 state 1e-7 .. 2.6e-6 on `pattern` (d = 1 .. 128, all three solvers), at most 8.8e-6 on `tiny_a` (`user`,
d = 96, llt: 150 users and 90 items leave the Gramians rank-deficient); after one free-running epoch at most 2.8e-5 (`context_bias`,
pattern, d = 33).  CAP is the largest of them with 2x headroom, rounded up to the next power of ten."""
import numpy as np
import pytest

import cfr_cases as CC
import helpers as H
from ref_cfr import ARRAYS, DEFECTS, F64CFR, bound, relerr

CAP = 1e-4      # set from 2.83e-5 (free epoch) and 8.83e-6 (single step); a case above it does not belong in the envelope tests

# every (case, d, optimizer) the device tests run: test_cfr_rows_gpu.py on `pattern`, its used-handle test and test_cfr_gpu.py on `tiny_a`
YARDSTICK_CASES = [("pattern", 1, "llt"), ("pattern", 33, "manual_cg"), ("pattern", 64, "ldlt"), ("pattern", 65, "llt"), ("pattern", 96, "manual_cg"),
                   ("pattern", 128, "llt"), ("tiny_a", 8, "llt"), ("tiny_a", 20, "llt"), ("tiny_a", 20, "manual_cg"),
                   ("tiny_a", 40, "ldlt"), ("tiny_a", 96, "llt"), ("tiny_b", 20, "llt"), ("gaps", 8, "llt")]


def schedule_of(d):
    return CC.STEPS_THEN_EPOCH if d <= 33 else CC.SINGLE_STEPS


@pytest.mark.parametrize("name,d,optimizer", YARDSTICK_CASES)
def test_yardstick_follows_the_oracle(name, d, optimizer):
    orc, f64 = CC.references(name, d, optimizer, schedule_of(d))
    lines, worst = [], 0.0
    for o, f in zip(orc, f64):
        errs = {n: relerr(o.arrs[n], f.arrs[n]) for n in ARRAYS}
        worst = max(worst, *errs.values())
        lines.append("step %s: err(oracle, f64) %s; loss oracle %s f64 %s" % (
            o.step, " ".join("%s %.3g" % kv for kv in errs.items() if kv[1]), " ".join("%.9g" % x for x in o.loss), " ".join("%.12g" % x for x in f.loss)))
        for lo, lf in zip(o.loss, f.loss):      # the oracle's float per-row sums against the float64 ones
            assert abs(lo - lf) <= 1e-6 * abs(lf), lines
    CC.record("cpu yardstick vs oracle, %s d=%d %s" % (name, d, optimizer), lines + ["largest %.3g (cap %g)" % (worst, CAP)])
    assert worst <= CAP, lines


CAP_EPOCH = 1e-3    # set from 6.49e-5, the largest free-epoch distance over the six neighbouring starts (2x headroom passes 1e-4)


@pytest.mark.parametrize("d,optimizer", [(1, "llt"), (33, "manual_cg")])
def test_the_oracle_s_epoch_distance_is_a_cloud(d, optimizer):
    """What cfr_cases.epoch_distance rests on: starts one ulp apart leave the float64 epoch where it is and move the oracle's
    distance to it by a large factor at d = 33 (measured 2.8 for `context_bias`); the envelope of the epoch takes the largest."""
    worst, draws, moved = CC.epoch_distance("pattern", d, optimizer)
    orc, f64 = CC.references("pattern", d, optimizer, CC.STEPS_THEN_EPOCH)
    lines = ["start %d: err(oracle, f64) %s" % (k, " ".join("%s %.3g" % kv for kv in e.items())) for k, e in enumerate(draws)]
    lines.append("the float64 epoch moved by at most %.3g between the starts" % max(max(m.values()) for m in moved))
    lines.append("largest / smallest: " + " ".join("%s %.2f" % (n, worst[n] / min(e[n] for e in draws)) for n in ARRAYS))
    CC.record("cpu epoch distance over %d starts, pattern d=%d %s" % (len(draws), d, optimizer), lines)
    assert draws[0] == {n: relerr(orc[3].arrs[n], f64[3].arrs[n]) for n in ARRAYS}       # start 0 is the case's own state
    assert max(max(m.values()) for m in moved) <= 1e-6, lines        # a start one ulp away is the same problem
    assert max(worst.values()) <= CAP_EPOCH, lines


def test_pattern_has_the_rows_it_promises():
    case = CC.pattern()
    for m in (case.csr, case.t, case.ctx):
        assert tuple(CC.lengths_of(m)[:len(CC.NAMED_LENGTHS)]) == CC.NAMED_LENGTHS
    CC.assert_second_tickets(case, 256)         # the MI355X has 256 CUs: 4,096 waves per launch
    # gaps: the rows of the existing 6 x 5 case that have entries in one matrix only
    g = CC.gaps()
    assert CC.lengths_of(g.t)[1] > 0 and CC.lengths_of(g.ctx)[1] == 0 and CC.lengths_of(g.csr)[1] == 0
    orc, f64 = CC.references("gaps", 8, "llt", CC.STEPS_THEN_EPOCH)
    start = CC.arrays(g, 8)
    for s in (orc[1], f64[1]):
        assert s.arrs["item_bias"][1, 0] == 0.0 and not np.array_equal(s.arrs["item"][1], start["item"][1])     # user entries only: solved, bias 0 / 1e-10
    for s in (orc[0], f64[0]):
        assert np.array_equal(s.arrs["user"][1], start["user"][1]) and np.array_equal(s.arrs["user"][3], start["user"][3])
    for s in (orc[2], f64[2]):
        assert np.array_equal(s.arrs["context"][1], start["context"][1]) and np.array_equal(s.arrs["context_bias"][4], start["context_bias"][4])


def test_item_update_is_the_dense_system_and_its_loss_the_objective():
    """A, y and the loss of every item row of `tiny_a` rebuilt from the dense U x I and I x I matrices, the loss without the FF
    trick: l [sum_{u not in row} (i.u)^2 + sum_{u in row} (1 + alpha v)(i.u - 1)^2] + sum err^2 + reg_i |i|^2."""
    d = 8
    case = CC.tiny(3)
    o = CC.opt(d, "llt")
    f = F64CFR()
    assert f.init(H.write_opt(o))
    arrs = CC.arrays(case, d)
    CC.bind(f, arrs)
    f.precompute(b"user")
    U, I, Cx, Ib, Cb = (arrs[n].astype(np.float64) for n in ARRAYS)
    alpha, l, reg_i = (float(np.float32(o[k])) for k in ("alpha", "l", "reg_i"))
    R, M = np.zeros((case.users, case.items)), np.zeros((case.users, case.items), bool)
    R[case.csr.rows(), case.csr.keys], M[case.csr.rows(), case.csr.keys] = case.csr.vals, True
    S, Ms = np.zeros((case.items, case.items)), np.zeros((case.items, case.items), bool)
    S[case.ctx.rows(), case.ctx.keys], Ms[case.ctx.rows(), case.ctx.keys] = case.ctx.vals, True
    total = 0.0
    for x in range(case.items):
        ku, vu = case.t.row(x)
        kc, vc = case.ctx.row(x)
        A, y = f.item_system(x, ku, vu.astype(np.float64), kc, vc.astype(np.float64))
        w = 1.0 + alpha * R[:, x]                       # 1 where the user has no entry
        Ad = l * (U.T * w) @ U + (Cx.T * Ms[x]) @ Cx + reg_i * np.eye(d)
        yd = l * ((w * M[:, x]) @ U) + (Ms[x] * (S[x] - Ib[x, 0] - Cb[:, 0])) @ Cx
        assert np.abs(A - Ad).max() <= 1e-12 * np.abs(Ad).max() and np.abs(y - yd).max() <= 1e-12 * np.abs(yd).max(), x
        dot = U @ I[x]
        err = (S[x] - Cx @ I[x] - Ib[x, 0] - Cb[:, 0])[Ms[x]]
        want = l * ((dot[~M[:, x]] ** 2).sum() + (w * (dot - 1.0) ** 2)[M[:, x]].sum()) + (err ** 2).sum() + reg_i * (I[x] ** 2).sum()
        got = f.item_loss(x, ku, vu.astype(np.float64), kc, vc.astype(np.float64))
        assert abs(got - want) <= 1e-12 * want, (x, got, want)
        total += want
    got = CC.update_item(f, case)
    assert abs(got - total) <= 1e-12 * total
    for x in range(case.items):                         # ... and the rows it wrote are the solutions of those systems
        ku, vu = case.t.row(x)
        w = 1.0 + alpha * R[:, x]
        Ad = l * (U.T * w) @ U + (Cx.T * Ms[x]) @ Cx + reg_i * np.eye(d)
        yd = l * ((w * M[:, x]) @ U) + (Ms[x] * (S[x] - Ib[x, 0] - Cb[:, 0])) @ Cx
        sol = np.linalg.solve(Ad, yd)
        assert np.abs(f.F["item"][x] - sol).max() <= 1e-12 * np.abs(sol).max()


TOUCHES = {"ctx_pad_lane": (("I", "item"), ("I", "item_bias"), ("C", "context"), ("C", "context_bias")),
           "drop_chunk_tail": (("I", "item"), ("C", "context")),
           "y_not_scaled": (("U", "user"), ("I", "item"))}


@pytest.mark.parametrize("defect", DEFECTS)
def test_the_device_bound_has_teeth(defect):
    """Each planted single-point mistake moves the arrays it touches by far more than the envelope allows a device run."""
    d, optimizer = 33, "manual_cg"
    case = CC.pattern()
    orc, f64 = CC.references("pattern", d, optimizer, CC.STEPS_THEN_EPOCH)
    bad = CC.run(lambda: F64CFR(defect=defect), case, d, optimizer, CC.SINGLE_STEPS)
    by_step = {s.step: k for k, s in enumerate(bad)}
    lines, ratios = [], []
    for s, name in TOUCHES[defect]:
        k = by_step[s]
        allowed = bound(relerr(orc[k].arrs[name], f64[k].arrs[name]))
        moved = relerr(bad[k].arrs[name], f64[k].arrs[name])
        ratios.append(moved / allowed)
        lines.append("%s, step %s: moves %s by %.3g = %.0f x the device bound %.3g" % (defect, s, name, moved, moved / allowed, allowed))
    CC.record("cpu teeth, pattern d=%d %s" % (d, optimizer), lines)
    assert all(r >= 10 for r in ratios), lines
