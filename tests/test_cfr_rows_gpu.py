"""CoFactor on the device against the float64 yardstick (tests/ref_cfr.py): the row lengths at which the Gramian passes of
csrc/als_kernels.hpp change course, run through the four switches only CFR sets (`ctx`, `accumulate`, `out_scale`, `ff_scale`).

The bound everywhere: err(hip, f64) <= 2.5 x err(oracle, f64) + 4 x 2^-23 (ref_eals.bound), per array, biases included, all three
sides from the same float32 state.  The loss: |loss_hip - loss_f64| <= |loss_oracle - loss_f64| + 8 x 2^-24 |loss_f64|
(ref_eals.loss_bound).  What was measured (ratios per case) is in profiles/cfr_parity.txt.

Which row of `pattern` (cfr_cases.py) runs what, in each of the four passes (user, item <- users, item <- contexts, context):
  0                     skipped: the row keeps its bits
  1, 2, 3               one leftover pair, half padding at 1 and 3 -- in `ctx` mode the padding lane's weight is the `one` argument
  63 / 64 / 65          one 64-entry chunk less a lane, full, and a second chunk of one entry
  127 / 128 / 129       the same one chunk on
  4095 / 4096           the longest rows that stay one work item
  4097                  two work items of 2050 + 2047 entries adding into one slot, `bias_self` taken off in both
  8193                  three: 2732 + 2732 + 2729, the tail odd
Every pass of a whole-matrix call has about 8,300 work items for the 4,096 waves of a 256-CU launch: second tickets in the `ctx`
and in the `accumulate` passes.  Items 54 .. 63 have no user entries: solved from one context entry each."""
import numpy as np
import pytest

import cfr_cases as CC
import helpers as H
from ref_cfr import ARRAYS, loss_bound

pytestmark = pytest.mark.gpu

NAMED = len(CC.NAMED_LENGTHS)


def _hip():
    from buffalo_amd.backend import CyCFR
    return CyCFR()


def _schedule(d):
    return CC.STEPS_THEN_EPOCH if d <= 33 else CC.SINGLE_STEPS


@pytest.mark.parametrize("d,optimizer", [(1, "llt"), (33, "manual_cg"), (64, "ldlt"), (65, "llt"), (96, "manual_cg"), (128, "llt")])
def test_row_lengths_and_their_edges(d, optimizer):
    """The three single steps, and at d <= 33 one free-running epoch.  The epoch is held to 2.5 x the LARGEST distance of the oracle
    over six start states one ulp apart (cfr_cases.epoch_distance, where the reason is written down): against the single oracle run
    its `context_bias` came out at 1.76, 1.76 and 2.80 times the oracle's distance in three runs of one library (d = 33), while the
    oracle's own distance moves by a factor 2.8 between those neighbours."""
    import torch
    case = CC.pattern()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    CC.assert_second_tickets(case, cus)
    orc, f64 = CC.references("pattern", d, optimizer, _schedule(d))
    hip = CC.run(_hip, case, d, optimizer, _schedule(d))
    epoch = CC.epoch_distance("pattern", d, optimizer)[0] if d <= 33 else None
    CC.hold("rows pattern d=%d %s (%d CUs)" % (d, optimizer, cus), hip, orc, f64, named=NAMED, epoch=epoch)
    start = CC.arrays(case, d)
    u, i, c = hip[0].arrs, hip[1].arrs, hip[2].arrs
    # rows without entries keep their bits (cfr.cc:116-119, 184-187, 281-284)
    assert np.array_equal(u["user"][0], start["user"][0])
    assert np.array_equal(i["item"][0], start["item"][0]) and np.array_equal(i["item_bias"][0], start["item_bias"][0])
    assert np.array_equal(c["context"][0], start["context"][0]) and np.array_equal(c["context_bias"][0], start["context_bias"][0])
    # items with context entries only are solved, as the oracle solves them (inside the envelope: held above)
    rows = slice(CC.N_LONG, CC.FIRST_FREE)
    assert not CC.lengths_of(case.t)[rows].any() and CC.lengths_of(case.ctx)[rows].all()
    for s in (hip[1], orc[1]):
        assert (s.arrs["item"][rows] != start["item"][rows]).any(axis=1).all()


def _hold_losses(section, hip, orc, f64):
    lines, bad = [], []
    for h, o, f in zip(hip, orc, f64):
        for lh, lo, lf in zip(h.loss, o.loss, f.loss):
            ln = "step %s: loss f64 %.12g |oracle - f64| %.3g |hip - f64| %.3g allowed %.3g" % (h.step, lf, abs(lo - lf), abs(lh - lf), loss_bound(lo, lf))
            lines.append(ln)
            if not abs(lh - lf) <= loss_bound(lo, lf):
                bad.append(ln)
    CC.record(section, lines)
    assert not bad, "\n".join(lines)


def test_losses_against_float64():
    d, optimizer = 33, "manual_cg"
    case = CC.pattern()
    orc, f64 = CC.references("pattern", d, optimizer, _schedule(d))
    hip = CC.run(_hip, case, d, optimizer, CC.SINGLE_STEPS)
    _hold_losses("losses pattern d=%d %s" % (d, optimizer), hip, orc, f64)
    off = CC.run(_hip, case, d, optimizer, CC.SINGLE_STEPS, compute_loss=False)
    assert [s.loss for s in off] == [[0.0], [0.0], [0.0]]
    CC.hold("losses off pattern d=%d %s" % (d, optimizer), off, orc, f64)       # the rows do not depend on the switch


def _light_rows(case, s):
    """Rows whose every Gramian pass of step `s` is one work item: at most 4,096 entries in either matrix."""
    lu, lt, lc = (CC.lengths_of(m) for m in (case.csr, case.t, case.ctx))
    return {"U": lu <= 4096, "I": (lt <= 4096) & (lc <= 4096), "C": lc <= 4096}[s]


def test_chunked_calls():
    """Every update made in the calls [0, 14) [14, 14) [14, 54) [54, 5000) [5000, N): an empty call, shift_u != shift_c in every
    item call after the first.  A row of one work item per pass adds one value per slot element per pass, and two passes make a
    commutative sum, so such rows must come out bit-identical to the one-call run; the chunks of a longer row add in ticket order."""
    d, optimizer = 33, "manual_cg"
    case = CC.pattern()
    orc, f64 = CC.references("pattern", d, optimizer, _schedule(d))
    one = CC.run(_hip, case, d, optimizer, CC.SINGLE_STEPS)
    cut = CC.run(_hip, case, d, optimizer, CC.SINGLE_STEPS, ranges=list(CC.CHUNKED_CALLS))
    CC.hold("chunked calls pattern d=%d %s" % (d, optimizer), cut, orc, f64, named=NAMED)
    _hold_losses("chunked calls pattern d=%d %s" % (d, optimizer), cut, orc, f64)
    # in `pattern` every call of that list holds rows with user entries; [54, 64) is the call whose rows have none at all
    ctx_only = CC.run(_hip, case, d, optimizer, ("I",), ranges=[(0, CC.N_LONG), (CC.N_LONG, CC.FIRST_FREE), (CC.FIRST_FREE, case.items)])
    CC.hold("item calls [0, 54) [54, 64) [64, N) pattern d=%d %s" % (d, optimizer), ctx_only, orc[1:2], f64[1:2])
    lines = []
    for a, b in zip(one + one[1:2], cut + ctx_only):
        light = _light_rows(case, a.step)
        for name in ARRAYS:
            diff = np.flatnonzero((a.arrs[name] != b.arrs[name]).any(axis=1))
            lines.append("step %s %s: %d rows differ from the one-call run, %d of them light%s" % (
                a.step, name, diff.shape[0], int(light[diff].sum()), (" (rows %s)" % diff[:8].tolist()) if diff.shape[0] else ""))
            assert not light[diff].any(), lines
    CC.record("chunked calls pattern d=%d %s" % (d, optimizer), lines)


def _same_bits(a, b):
    return {name: int((a.arrs[name] != b.arrs[name]).any(axis=1).sum()) for name in ARRAYS}


def test_a_used_handle_follows_the_matrix_it_is_handed():
    """The reference's front keeps one CyCFR per model and accepts set_data with a new matrix (cfr.py:68); CCFR holds no data
    state.  `tiny_a` and `tiny_b` have one shape and different row bounds: whatever a handle remembers of the first must not
    reach the second."""
    d, optimizer = 20, "llt"
    a, b = CC.tiny(3), CC.tiny(13)
    assert (a.users, a.items) == (b.users, b.items) and not np.array_equal(a.csr.indptr, b.csr.indptr)
    assert not np.array_equal(a.t.indptr, b.t.indptr) and not np.array_equal(a.ctx.indptr, b.ctx.indptr)
    start = CC.arrays(b, d)
    g = _hip()
    assert g.init(H.write_opt(CC.opt(d, optimizer)))
    CC.step(g, a, "E", CC.arrays(a, d))
    used = [CC.step(g, b, s, start) for s in CC.SINGLE_STEPS]
    fresh = CC.run(_hip, b, d, optimizer, CC.SINGLE_STEPS)
    orc, f64 = CC.references("tiny_b", d, optimizer, CC.STEPS_THEN_EPOCH)
    CC.record("used handle: tiny_a then tiny_b d=%d %s" % (d, optimizer),
              ["step %s: rows that differ from a fresh handle's %s" % (u.step, _same_bits(u, f)) for u, f in zip(used, fresh)])
    CC.hold("used handle: tiny_a then tiny_b d=%d %s" % (d, optimizer), used, orc, f64)
    for u, f in zip(used, fresh):
        assert not any(_same_bits(u, f).values()), (u.step, _same_bits(u, f))
    # init again with another d and another solver, back on tiny_a with the row ranges the handle has seen
    d, optimizer = 40, "ldlt"
    assert g.init(H.write_opt(CC.opt(d, optimizer)))
    start = CC.arrays(a, d)
    used = [CC.step(g, a, s, start) for s in CC.SINGLE_STEPS]
    fresh = CC.run(_hip, a, d, optimizer, CC.SINGLE_STEPS)
    orc, f64 = CC.references("tiny_a", d, optimizer, CC.SINGLE_STEPS)
    CC.hold("used handle: init again, tiny_a d=%d %s" % (d, optimizer), used, orc, f64)
    for u, f in zip(used, fresh):
        assert not any(_same_bits(u, f).values()), (u.step, _same_bits(u, f))
    # set_embedding with fewer rows, then a call: a user row depends on its own entries and the items alone
    n = 100
    arrs = {k: v.copy() for k, v in start.items()}
    CC.bind(g, arrs)
    fewer = arrs["user"][:n].copy()
    g.set_embedding(fewer, b"user")
    CC.update_user(g, a, [(0, n)])
    assert np.array_equal(fewer, fresh[0].arrs["user"][:n]) and np.array_equal(arrs["user"], start["user"])
    from buffalo_amd.backend import BuffaloHipError
    with pytest.raises(BuffaloHipError, match="bad row range"):
        CC.update_user(g, a, [(0, n + 1)])


def test_refusals():
    from buffalo_amd.backend import BuffaloHipError
    d = 20
    case = CC.tiny(3)
    with pytest.raises(BuffaloHipError, match="d > 128"):
        _hip().init(H.write_opt(CC.opt(129, "llt")))
    g = _hip()
    assert g.init(H.write_opt(CC.opt(d, "llt")))
    arrs = CC.arrays(case, d)
    for name in ARRAYS[:4]:
        g.set_embedding(arrs[name], name.encode("utf8"))
    g.precompute(b"user")
    with pytest.raises(BuffaloHipError, match="all five"):
        CC.update_item(g, case)
    g.set_embedding(arrs["context_bias"], b"context_bias")
    with pytest.raises(BuffaloHipError, match="user or item"):
        g.precompute(b"context")
    for a, b in ((5, 4), (0, case.users + 1)):
        with pytest.raises(BuffaloHipError, match="bad row range"):
            g.partial_update_user(a, b, case.csr.indptr, case.csr.keys, case.csr.vals)
    for a, b in ((5, 4), (0, case.items + 1)):
        with pytest.raises(BuffaloHipError, match="bad row range"):
            g.partial_update_item(a, b, case.t.indptr, case.t.keys, case.t.vals, case.ctx.indptr, case.ctx.keys, case.ctx.vals)
        with pytest.raises(BuffaloHipError, match="bad row range"):
            g.partial_update_context(a, b, case.ctx.indptr, case.ctx.keys, case.ctx.vals)
    start = CC.arrays(case, d)
    assert all(np.array_equal(arrs[k], start[k]) for k in ARRAYS)        # the refused calls wrote nothing
    # ... and the handle is whole: the steps that follow are inside the envelope
    hip = [CC.step(g, case, s, start) for s in CC.SINGLE_STEPS]
    orc, f64 = CC.references("tiny_a", d, "llt", CC.STEPS_THEN_EPOCH)
    CC.hold("after refusals tiny_a d=%d llt" % d, hip, orc, f64)
