"""eALS on the device against the float64 yardstick (tests/ref_eals.py): the three row classes of csrc/eals_handle.hpp and their
edges, the block-per-row kernel end to end, ticket / slot reuse, a handle initialised again, refusals.

The bound everywhere: err(hip, f64) <= 2.5 x err(oracle, f64) + 4 x 2^-23 (ref_eals.bound), all three sides from the same float32
state.  The loss: |loss_hip - loss_f64| <= |loss_oracle - loss_f64| + 8 x 2^-24 |loss_f64| (ref_eals.loss_bound).  What was
measured (ratios per case) is in profiles/eals_parity.txt.

Which test runs which part of `eals_update_long_kernel<1024>` (rows above 4,096 entries):
  the row's own scratch slot (`row_off`, `heavy_off`)   pattern rows 4097 / 4160 / 4161 / 6000: four slots of 4160, 4160, 4224 and 6016 entries in
                                          one launch (test_row_classes_and_their_edges); 520 slots in test_tickets_and_slots_are_reused
  the ticket broadcast through red[0]     every heavy row; a SECOND ticket per block only where rows outnumber blocks: `many` (520 rows, 512 blocks)
  the 16-wave combination through red[]   every heavy row: 4,097 entries already spread over all 16 waves
  the deferred fold (dd > 0)              every d > 1; d = 1 runs the block close alone
  the block close with nd < 16            d = 1, 17 (a one-wide tail block), 24, 72, 200; nd = 16 exactly: d = 16
  the mirror write other[map[..]]         the NEXT half-epoch reads it (free-running epochs), and estimate_loss through either
                                          orientation must agree to one float ulp (test_heavy_rows_end_to_end)
Class bounds: 256 / 257 and 4096 / 4097 and the slot rounding 4160 / 4161 (also 63 / 64 / 65, 319 / 320 / 321) are rows of `pattern`.
A second ticket in the mid loop: `many` (4,200 mid rows, 4,096 waves)."""
import numpy as np
import pytest

import eals_cases as EC
import helpers as H
from ref_eals import bound, loss_bound, relerr

pytestmark = pytest.mark.gpu


def _hip():
    from buffalo_amd.backend import CyEALS
    return CyEALS()


def _hold(section, hip, orc, f64, losses=False, named_rows=None):
    """Every snapshot of the device run inside the envelope of the oracle's; -> the lines that were recorded."""
    lines, bad = [], []
    for h, o, f in zip(hip, orc, f64):
        eo, eh = relerr(o.X(), f.X()), relerr(h.X(), f.X())
        ln = "step %d update(%d): err(oracle, f64) %.3g err(hip, f64) %.3g ratio %.2f bound %.3g" % (h.step, h.axis, eo, eh, eh / max(eo, 1e-30), bound(eo))
        ok = eh <= bound(eo)
        if losses:
            lo, lh, lf = o.loss[h.axis], h.loss[h.axis], f.loss[h.axis]
            ln += "; loss f64 %.12g |oracle - f64| %.3g |hip - f64| %.3g allowed %.3g; hip axis 0 / 1 %.9g / %.9g" % (
                lf, abs(lo - lf), abs(lh - lf), loss_bound(lo, lf), h.loss[0], h.loss[1])
            ok = ok and abs(lh - lf) <= loss_bound(lo, lf) and abs(h.loss[0] - h.loss[1]) <= 2.0 ** -23 * abs(h.loss[0])
        lines.append(ln)
        if named_rows is not None and h.axis == named_rows:     # a failure names the row class
            scale = np.abs(f.X()).max()
            per = ["%d: %.2g / %.2g" % (n, np.abs(o.X()[i] - f.X()[i]).max() / scale, np.abs(h.X()[i] - f.X()[i]).max() / scale)
                   for i, n in enumerate(EC.NAMED_LENGTHS)]
            lines.append("  per row, entries: err(oracle) / err(hip)  " + "  ".join(per))
        if not ok:
            bad.append(ln)
        assert np.isfinite(h.P).all() and np.isfinite(h.Q).all()
    EC.record(section, lines)
    assert not bad, "\n".join(lines)
    return lines


@pytest.mark.parametrize("d", [1, 16, 17, 72, 200])
@pytest.mark.parametrize("side", ["user", "item"])
def test_row_classes_and_their_edges(side, d):
    name = "pattern_" + side
    axis = 0 if side == "user" else 1
    prob = EC.problem(name, d)
    lens = EC.lengths_of(prob[0] if axis == 0 else prob[0].transpose())
    assert tuple(lens[:len(EC.NAMED_LENGTHS)]) == EC.NAMED_LENGTHS
    orc, f64 = EC.references(name, d, EC.HALVES_THEN_EPOCH)
    hip = EC.run(_hip, d, prob, EC.HALVES_THEN_EPOCH, losses=False)
    _hold("rows %s d=%d" % (name, d), hip, orc, f64, named_rows=axis)
    # the row without entries moves by the regulariser alone (eals.cc:193-216, 261-262), like the oracle's
    X0 = prob[1 + axis]
    for h, o in zip(hip, orc):
        if h.axis == axis:
            assert np.array_equal(h.X()[0] == X0[0], o.X()[0] == X0[0])
            if axis == 1:   # an item nobody touched has c_i = 0: numerator 0, denominator reg_i -> exactly 0 on both sides
                assert prob[3][0] == 0.0 and np.array_equal(h.X()[0], o.X()[0]) and not h.X()[0].any()


@pytest.mark.parametrize("d", [24, 17])
def test_heavy_rows_end_to_end(d):
    prob = EC.problem("heavy", d)
    orc, f64 = EC.references("heavy", d, EC.TWO_EPOCHS)
    hip = EC.run(_hip, d, prob, EC.TWO_EPOCHS)
    _hold("heavy 4500 x 12 d=%d" % d, hip, orc, f64, losses=True)


def test_tickets_and_slots_are_reused():
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    csr = EC.many()
    # the mid launch has min(n_mid, 16 CUs) waves, the heavy launch min(n_heavy, 2 CUs) blocks: both loops must hand some group a second row
    assert csr.num_users > 16 * cus and csr.num_items > 2 * cus, cus
    prob = EC.problem("many", 16)
    orc, f64 = EC.references("many", 16, EC.ONE_EPOCH)
    hip = EC.run(_hip, 16, prob, EC.ONE_EPOCH)
    _hold("many 4200 x 520 d=16 (%d CUs)" % cus, hip, orc, f64, losses=True)


def test_initialize_again_on_a_used_handle():
    """One handle: `tiny` (the scratch and the side buffers then grow from small to large), `many`, then pattern("item") (a 6,000-entry
    row, longer than anything the scratch saw; other side lengths, other nnz), then `tiny` again.  The caches of the previous model must
    not survive initialize_model."""
    d = 16
    g = _hip()
    assert g.init(H.write_opt(EC.opt(d)))
    for name in ("tiny", "many", "pattern_item", "tiny"):
        prob = csr, P0, Q0, Cw = EC.problem(name, d)
        t = csr.transpose()
        P, Q = P0.copy(), Q0.copy()
        g.initialize_model(P, Q, Cw)
        assert not g.update(csr.indptr, csr.keys, csr.vals, 0)                      # eals.cc:106-114: no cache yet
        assert g.estimate_loss(csr.nnz, csr.indptr, csr.keys, csr.vals, 0) == (0.0, 0.0)
        g.precompute_cache(csr.nnz, csr.indptr, csr.keys, 0)
        assert not g.update(t.indptr, t.keys, t.vals, 1) and not g.update(csr.indptr, csr.keys, csr.vals, 0)
        assert np.array_equal(P, P0) and np.array_equal(Q, Q0)
        g.precompute_cache(csr.nnz, t.indptr, t.keys, 1)
        hip = [EC.step(g, prob, 0, P, Q, 1, losses=False), EC.step(g, prob, 1, P, Q, 2, losses=False)]
        orc, f64 = EC.references(name, d, EC.ONE_EPOCH)
        _hold("reinit %s d=%d" % (name, d), hip, orc, f64)


def test_refusals_launch_nothing():
    from buffalo_amd.backend import BuffaloHipError, CyEALS
    d = 16
    prob = csr, P0, Q0, Cw = EC.problem("tiny", d)
    t = csr.transpose()
    g = CyEALS()
    with pytest.raises(BuffaloHipError, match="1024"):
        g.init(H.write_opt(EC.opt(1025)))
    g = CyEALS()
    assert g.init(H.write_opt(EC.opt(d)))
    with pytest.raises(BuffaloHipError, match="before initialize_model"):
        g.update(csr.indptr, csr.keys, csr.vals, 0)
    P, Q = P0.copy(), Q0.copy()
    g.initialize_model(P, Q, Cw)
    with pytest.raises(BuffaloHipError, match="does not end at nnz"):
        g.precompute_cache(csr.nnz - 1, csr.indptr, csr.keys, 0)
    with pytest.raises(BuffaloHipError, match="axis"):
        g.precompute_cache(csr.nnz, csr.indptr, csr.keys, 2)
    assert not g.update(csr.indptr, csr.keys, csr.vals, 0)          # the refused calls bound nothing
    g.precompute_cache(csr.nnz, csr.indptr, csr.keys, 0)
    g.precompute_cache(csr.nnz, t.indptr, t.keys, 1)
    with pytest.raises(BuffaloHipError, match="nnz differs"):
        g.estimate_loss(csr.nnz - 1, csr.indptr, csr.keys, csr.vals, 0)
    assert np.array_equal(P, P0) and np.array_equal(Q, Q0)
    # ... and the handle is whole: the epoch that follows is the one a fresh handle computes
    hip = [EC.step(g, prob, 0, P, Q, 1, losses=False), EC.step(g, prob, 1, P, Q, 2, losses=False)]
    orc, f64 = EC.references("tiny", d, EC.ONE_EPOCH)
    _hold("after refusals tiny d=%d" % d, hip, orc, f64)
