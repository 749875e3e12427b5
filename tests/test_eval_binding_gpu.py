"""The upper layers of the validation evaluator on the device: the compiled Cython class (integration/buffalo/algo/hip/_evaluate.pyx)
against the ctypes mirror, the mixin reading a training handle's factors straight from HBM, and the one-device contract of a handle."""
import os
import sys

import numpy as np
import pytest

import eval_cases as ec
import helpers as H

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
RANK = ("ndcg", "map", "accuracy", "auc")


def _trained_bpr(train, P0, Q0, Qb0, d, vdim):
    from conftest import bpr_opt
    from buffalo_amd.backend import CyBPR
    P, Q = H.pad(0.1 * P0, vdim), H.pad(0.1 * Q0, vdim)
    Qb = np.ascontiguousarray(0.1 * Qb0)
    obj = H.run_hip_sgd(CyBPR, bpr_opt(d=d, lr=0.05, num_iters=3), train, P, Q, Qb, epochs=3)
    return obj, P, Q, Qb


def test_compiled_binding_equals_the_ctypes_mirror():
    """CyEvaluator and Evaluator drive one library: the same dicts and lists, host forms and device forms, with and without bias,
    all rows and a subset; a None where an array belongs is a TypeError, a refused call a RuntimeError with the library's message."""
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "integration"))
    import build_binding
    build_binding.build()
    CyEvaluator = build_binding.import_evaluator()
    from buffalo_amd.evaluate import Evaluator
    train, vali, P0, Q0, Qb0 = ec.planted(U=200, I=300, d=20, bias=True, seed=14)
    d, vdim = 20, 32
    obj, P, Q, Qb = _trained_bpr(train, P0, Q0, Qb0, d, vdim)
    hP, hQ, qb = np.ascontiguousarray(P[:, :d]), np.ascontiguousarray(Q[:, :d]), np.ascontiguousarray(Qb.reshape(-1))
    no_bias = np.zeros(0, np.float32)
    data = (200, 300, train.indptr, train.keys, vali["row"], vali["col"], vali["val"])
    cy, ct = CyEvaluator(), Evaluator()
    cy.set_data(*data)
    ct.set_data(*data)
    assert cy.num_rows() == ct.num_rows() > 100
    subset = np.unique(vali["row"])[::4].astype(np.int32)
    dP, dQ, dQb = (obj.device_buffer(n)[0] for n in ("P", "Q", "Qb"))
    for rows in (None, subset):
        for bias in (True, False):
            want, want_keys = ct.ranking(hP, hQ, qb if bias else None, rows=rows, topk=10, return_keys=True)
            got, keys = cy.ranking(hP, hQ, qb if bias else no_bias, rows, 10, return_keys=True)
            assert got == want and np.array_equal(keys, want_keys) and want["N"] > 0
            got, keys = cy.ranking_device(dP, 200, dQ, 300, d, vdim, dQb if bias else 0, rows, 10, return_keys=True)
            assert got == want and np.array_equal(keys, want_keys)
            assert cy.ranking(hP, hQ, qb if bias else no_bias, rows, 10) == want
    for bias in (True, False):
        want = ct.scores(hP, hQ, qb if bias else None)
        assert cy.scores(hP, hQ, qb if bias else no_bias) == want and want["rmse"] > 0
        assert cy.scores_device(dP, 200, dQ, 300, d, vdim, dQb if bias else 0) == want
    with pytest.raises(TypeError):
        cy.ranking(hP, hQ, None, None, 10)
    with pytest.raises(TypeError):
        cy.scores(hP, hQ, None)
    with pytest.raises(RuntimeError, match="topk must be in"):
        cy.ranking(hP, hQ, no_bias, None, 0)
    with pytest.raises(RuntimeError, match="unknown mode"):
        cy.set_mode("no_such_knob", 1)
    cy.set_mode("batch", 64)
    assert cy.ranking(hP, hQ, qb, None, 10) == ct.ranking(hP, hQ, qb, topk=10)


def test_mixin_reads_the_factors_of_a_training_handle_from_hbm():
    """DeviceEvaluable with validation_on_device = True: device_buffer("P" / "Q" / "Qb") with get_vdim() as the leading dimension gives
    the dict of the host branch on the synchronised arrays, bit for bit."""
    from buffalo_amd.evaluate import DeviceEvaluable
    from buffalo_amd.serialize import Option
    train, vali, P0, Q0, Qb0 = ec.planted(U=200, I=300, d=20, bias=True, seed=15)
    obj, P, Q, Qb = _trained_bpr(train, P0, Q0, Qb0, 20, 32)

    class Data:
        groups = {"rowwise": {"indptr": train.indptr, "key": train.keys, "val": train.vals}, "vali": vali}

        def get_header(self):
            return {"num_users": 200, "num_items": 300, "num_nnz": train.nnz}

        def get_group(self, name):
            return self.groups[name]

        def has_group(self, name):
            return name in self.groups

    class Front(DeviceEvaluable):
        pass
    out = {}
    for on_device in (False, True):
        f = Front()
        f.validation_on_device = on_device
        f.data, f.obj, f.P, f.Q, f.Qb = Data(), obj, P, Q, Qb
        f.opt = Option({"d": 20, "use_bias": True, "validation": {"topk": 10}})
        assert obj.get_vdim() == 32
        out[on_device] = f.get_validation_results()
        f.opt["use_bias"] = False
        out[on_device, "no bias"] = f.get_validation_results()
    assert list(out[True]) == ["ndcg", "map", "accuracy", "auc", "rmse", "error"]
    assert out[True] == out[False] and out[True, "no bias"] == out[False, "no bias"]
    assert out[True] != out[True, "no bias"] and out[True]["ndcg"] > 0


def test_a_handle_stays_on_the_device_of_first_use():
    from buffalo_amd._lib import BuffaloHipError
    from buffalo_amd.evaluate import Evaluator
    train, vali, P, Q, _ = ec.planted(d=20, seed=16)
    ev = Evaluator()
    ev.set_device(0)                                  # a fresh handle may be placed
    ev.set_data(train.num_users, train.num_items, train.indptr, train.keys, vali["row"], vali["col"], vali["val"])
    before = ev.ranking(P, Q, topk=10)
    ev.set_device(0)                                  # the device it lives on: nothing to move
    with pytest.raises(BuffaloHipError, match="create a new handle"):
        ev.set_device(1)
    assert ev.ranking(P, Q, topk=10) == before        # the refused call left the handle as it was
