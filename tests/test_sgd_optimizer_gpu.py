"""The epoch-end optimizer step alone (sgd_update_rows_kernel, sgd_update_bias_kernel; csrc/sgd_kernels.hpp) against the float64 run of
ref_sgd.optimizer_step: X, grad, mom, vel and the counts are WRITTEN into the handle's device tensors, `update_parameters` is called
twice (the second call has the bias-correction exponent 2 and a non-zero mom / vel), and everything is read back.  Every output
element is held to  |dev - f64| / |f64| <= ref_eals.bound(worst element of the float32 restatement)  -- the oracle cannot be the
envelope here, its counts cannot be written from outside; tests/test_sgd_ref_cpu.py holds the restatement to the oracle.  An element
whose float64 value is 0 must be 0.  Measured: the worst element of any case at 0.23 x its bound (profiles/sgd_accumulate_parity.txt).

Inputs are drawn, not trained (`sgd_cases.draw_step_inputs`: no output element is a difference of nearly equal numbers), and hold what training never
produces:
  row 0            a count of 0 beside a non-zero gradient (Q-9: not divided)
  columns 0 ... 3  X = 0 with gradients 1e-12, 1e-10, 1, 1e6: FEPS outside the square root decides the first two (Q-5)
  padding columns  grad = 0, vel = 0 (and X = 0): the step is 0, not NaN
  WARP rows 1 ... 4  gradient 0 and reg 0, norms 0.5, exactly 1, 1 + 2^-20 and 30 on either side of the projection's max(1, |x|)
Shapes: vdim 32 ... 544 = every lane group G of the rows kernel (8, 16, 32, 64 lanes), vdim 96 / 160 / 288 with idle lanes in the group,
288 and 544 on the two-pass projection; P has 4 rpw + 1 rows (one past a full workgroup), Q has rpw - 1 (at least 1: the one-row call).
Both optimizers, BPRMF and WARP; WARP has no bias, so its gradQb column is divided by the count and otherwise left (Q-9), as is
BPRMF's with use_bias off."""
import numpy as np
import pytest

from conftest import bpr_opt, warp_opt
import helpers as H
import ref_sgd as rs
import sgd_cases as sc

pytestmark = pytest.mark.gpu

VDIMS = [32, 64, 96, 128, 160, 256, 288, 544]

def _options(kind, optimizer, d, use_bias):
    if kind == "warp":
        return warp_opt(d=d, optimizer=optimizer, per_coordinate_normalize=True, lr=0.05)
    return bpr_opt(d=d, optimizer=optimizer, per_coordinate_normalize=True, lr=0.05, use_bias=use_bias, reg_b=0.03)


def _check(tag, dev, inputs, cnt, reg, opt, iters, project, bias, report):
    """One array family (X, grad, mom, vel) of one call against the float64 and the float32 run from the same float32 inputs."""
    adam = opt["optimizer"] == "adam"
    outs = {}
    for dt in (np.float64, np.float32):
        X, g, m, v = (a.astype(dt) for a in inputs)
        outs[dt] = rs.optimizer_step(X, g, m if adam else None, v, cnt, reg, opt, iters, project=project, bias=bias)
    for name, got, w64, w32 in zip(("X", "grad", "mom", "vel"), dev, outs[np.float64], outs[np.float32]):
        if w64 is None:
            continue
        assert np.isfinite(got).all(), (tag, name)
        e_dev, e_ref = rs.elem_err(got, w64), rs.elem_err(w32, w64)
        report.append("%-28s %-4s dev %.3e  f32 %.3e  ratio %.2f" % (tag, name, e_dev.max(), e_ref.max(), e_dev.max() / max(e_ref.max(), rs.ULP32)))
        assert e_dev.max() <= rs.bound(e_ref.max()), (tag, name, float(e_dev.max()), float(e_ref.max()), np.unravel_index(e_dev.argmax(), e_dev.shape))


@pytest.mark.parametrize("vdim", VDIMS)
@pytest.mark.parametrize("kind,optimizer,use_bias", [("bpr", "adagrad", True), ("bpr", "adam", True), ("bpr", "adam", False),
                                                      ("warp", "adagrad", False), ("warp", "adam", False)])
def test_step_against_float64(kind, optimizer, use_bias, vdim):
    import torch
    from buffalo_amd.backend import CyBPR, CyWARP
    d, rows = vdim - 5, sc.step_rows(vdim)
    warp, adam = kind == "warp", optimizer == "adam"
    opt = _options(kind, optimizer, d, use_bias)
    rng = sc.step_rng(kind, optimizer, vdim)
    first = {s: sc.draw_step_inputs(rng, rows[s], d, warp) for s in "PQ"}
    P, Q = H.pad(first["P"][0], vdim), H.pad(first["Q"][0], vdim)
    Qb = first["Q"][1].reshape(-1, 1).copy()
    obj = (CyWARP if warp else CyBPR)()
    assert obj.init(H.write_opt(dict(opt, accelerator=True)))
    assert obj.get_vdim() == vdim
    obj.initialize_model(P, Q, Qb, 100, True)

    def tensor(name, side):
        if name.endswith("Qb"):
            return obj.device_tensor(name, (rows["Q"],))
        if name.startswith("count"):
            return obj.device_tensor(name, (rows[side],), dtype="int32")
        return obj.device_tensor(name, (rows[side], vdim))

    def read(name, side):
        a = tensor(name, side).cpu().numpy().copy()
        if a.ndim == 2:
            assert np.all(a[:, d:] == 0), (name, "padding columns")
            a = a[:, :d]
        return a
    report = []
    for call in range(2):
        drawn = first if call == 0 else {s: sc.draw_step_inputs(rng, rows[s], d, warp, first[s][5]) for s in "PQ"}
        cnts = {}
        for s in "PQ":
            _, _, g, gb, cnt, _ = drawn[s]
            tensor("grad" + s, s).copy_(torch.from_numpy(H.pad(g, vdim)))
            tensor("count" + s, s).copy_(torch.from_numpy(cnt))
            cnts[s] = cnt
            if s == "Q":
                tensor("gradQb", s).copy_(torch.from_numpy(gb))
        torch.cuda.synchronize()
        names = ("", "grad", "mom", "vel")
        before = {s: [read(n + s if n else s, s) if (n != "mom" or adam) else np.zeros((rows[s], d), np.float32) for n in names] for s in "PQ"}
        before["Qb"] = [read(n + "Qb" if n else "Qb", "Q") if (n != "mom" or adam) else np.zeros(rows["Q"], np.float32) for n in names]
        obj.update_parameters()
        after = {s: [read(n + s if n else s, s) if (n != "mom" or adam) else None for n in names] for s in "PQ"}
        after["Qb"] = [read(n + "Qb" if n else "Qb", "Q") if (n != "mom" or adam) else None for n in names]
        np.testing.assert_array_equal(P[:, :d], after["P"][0])          # update_parameters copies the model back
        np.testing.assert_array_equal(Qb.reshape(-1), after["Qb"][0])
        tag = "%s-%s-%d call %d" % (kind, optimizer, vdim, call)
        o = dict(opt, use_bias=bool(opt.get("use_bias", False)))
        _check(tag + " P", after["P"], before["P"], cnts["P"], opt["reg_u"], o, call, warp, False, report)
        _check(tag + " Q", after["Q"], before["Q"], cnts["Q"], opt["reg_i"], o, call, warp, False, report)
        _check(tag + " Qb", after["Qb"], before["Qb"], cnts["Q"], opt.get("reg_b", 0.0), o, call, False, True, report)
        if not o["use_bias"]:                                            # Q-9: divided by the count, nothing else
            nz = cnts["Q"] != 0
            want = before["Qb"][1].copy()
            want[nz] = want[nz] / cnts["Q"][nz].astype(np.float32)
            np.testing.assert_array_equal(after["Qb"][1], want)
            np.testing.assert_array_equal(after["Qb"][0], before["Qb"][0])
        for s in "PQ":                                                   # the counts are spent
            assert not tensor("count" + s, s).cpu().numpy().any()
    print("\n".join(report))
