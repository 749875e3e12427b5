"""Validation on the GPU -- the surface of ``buffalo.evaluate`` (/root/reference/buffalo/evaluate/base.py:44-148).

* ``Evaluator`` mirrors ``bfh_eval_*``: the training matrix and the ``vali`` group go to HBM once (``set_data``); ``ranking`` /
  ``scores`` then take factor matrices from numpy arrays, ``ranking_device`` / ``scores_device`` straight from the HBM buffers of a
  training handle (``obj.device_buffer("P")``), which is what validation right after an epoch wants.
* ``DeviceEvaluable`` is the mixin for a front: the three methods of ``Evaluable`` a buffalo maintainer overrides
  (``get_validation_results``, ``_evaluate_ranking_metrics``, ``_evaluate_score_metrics``), returning the reference's keys
  ``ndcg`` / ``map`` / ``accuracy`` / ``auc`` / ``rmse`` / ``error``.

The ranking excludes every user's training items inside the selection, so exactly ``topk`` entries per user are selected -- not
``topk + max_seen`` -- and the lists never leave the device.  Everything runs in ``libbuffalo_hip.so``; there is no CPU fallback.
"""
import ctypes as C

import numpy as np

from .backend import _arr, _Base, _ptr
from .parallel import _score_func_value

RANKING_KEYS = ("ndcg", "map", "accuracy", "auc")


class Evaluator(_Base):
    _PFX = "bfh_eval_"

    def set_score_func(self, name):
        """``"dot"`` (default) or ``"l2"``: the ranking by squared distance and the predictions ``1 - |p - q|^2`` of ``scores``
        (warp.py:94-107, :147); under ``"l2"`` a bias is refused (``bfh_eval_set_mode(h, "score_func", 1)``)."""
        self.set_mode("score_func", _score_func_value(name))

    def set_data(self, num_users, num_items, indptr, keys, vali_row, vali_col, vali_val):
        """indptr: int64 END offsets [num_users] (no leading 0) of the rowwise training matrix, keys ascending inside a row."""
        _arr(indptr, np.int64, 1, "indptr"), _arr(keys, np.int32, 1, "keys")
        _arr(vali_row, np.int32, 1, "vali_row"), _arr(vali_col, np.int32, 1, "vali_col"), _arr(vali_val, np.float32, 1, "vali_val")
        if indptr.shape[0] != int(num_users):
            raise ValueError("indptr must have one END offset per user")
        if not vali_row.shape == vali_col.shape == vali_val.shape:
            raise ValueError("vali_row / vali_col / vali_val must have the same length")
        self._call("set_data", int(num_users), int(num_items), _ptr(indptr, C.c_int64), _ptr(keys, C.c_int32), keys.shape[0],
                   _ptr(vali_row, C.c_int32), _ptr(vali_col, C.c_int32), _ptr(vali_val, C.c_float), vali_row.shape[0])

    def num_rows(self):
        """Users with validation entries: what ``rows=None`` ranks."""
        return self._call("num_rows")

    @staticmethod
    def _bias(Qb, q_rows):
        if Qb is None or Qb.size == 0:
            return None, 0
        Qb = np.ascontiguousarray(Qb, dtype=np.float32).reshape(-1)
        if Qb.shape[0] != q_rows:
            raise ValueError("Qb must have one entry per row of Q")
        return Qb, q_rows

    def _rows_and_keys(self, rows, topk, return_keys):
        if rows is not None:
            rows = _arr(np.ascontiguousarray(rows, dtype=np.int32), np.int32, 1, "rows")
        n = self.num_rows() if rows is None else rows.shape[0]
        keys = np.empty((n, int(topk)), dtype=np.int32) if return_keys else None
        return rows, n, keys

    @staticmethod
    def _ranking_result(out, keys, return_keys):
        res = dict(zip(RANKING_KEYS, out[:4].tolist()))
        res["N"] = float(out[4])
        return (res, keys) if return_keys else res

    def ranking(self, P, Q, Qb=None, rows=None, topk=10, return_keys=False):
        """{ndcg, map, accuracy, auc, N} of evaluate/base.py:44-128 (N == 0: all zeros) [, the filtered lists int32[n_rows, topk]]."""
        _arr(P, np.float32, 2, "P"), _arr(Q, np.float32, 2, "Q")
        Qb, qb_rows = self._bias(Qb, Q.shape[0])
        rows, n, keys = self._rows_and_keys(rows, topk, return_keys)
        out = np.zeros(5, dtype=np.float64)
        self._call("ranking", _ptr(P, C.c_float), P.shape[0], P.shape[1], _ptr(Q, C.c_float), Q.shape[0], Q.shape[1],
                   _ptr(Qb, C.c_float) if qb_rows else None, qb_rows, _ptr(rows, C.c_int32) if rows is not None else None, n, int(topk),
                   _ptr(out, C.c_double), _ptr(keys, C.c_int32) if return_keys else None)
        return self._ranking_result(out, keys, return_keys)

    def ranking_device(self, dP, p_rows, dQ, q_rows, d, ld, dQb=None, rows=None, topk=10, return_keys=False):
        """dP / dQ / dQb: device addresses (ints) of row-major [rows, ld] factors, e.g. ``obj.device_buffer("Q")[0]``."""
        rows, n, keys = self._rows_and_keys(rows, topk, return_keys)
        out = np.zeros(5, dtype=np.float64)
        self._call("ranking_device", C.c_void_p(dP), int(p_rows), C.c_void_p(dQ), int(q_rows), int(d), int(ld), C.c_void_p(dQb or 0),
                   int(q_rows) if dQb else 0, _ptr(rows, C.c_int32) if rows is not None else None, n, int(topk), _ptr(out, C.c_double),
                   _ptr(keys, C.c_int32) if return_keys else None)
        return self._ranking_result(out, keys, return_keys)

    def scores(self, P, Q, Qb=None):
        """{rmse, error} of evaluate/base.py:130-148."""
        _arr(P, np.float32, 2, "P"), _arr(Q, np.float32, 2, "Q")
        Qb, qb_rows = self._bias(Qb, Q.shape[0])
        out = np.zeros(2, dtype=np.float64)
        self._call("scores", _ptr(P, C.c_float), P.shape[0], P.shape[1], _ptr(Q, C.c_float), Q.shape[0], Q.shape[1],
                   _ptr(Qb, C.c_float) if qb_rows else None, qb_rows, _ptr(out, C.c_double))
        return {"rmse": out[0].item(), "error": out[1].item()}

    def scores_device(self, dP, p_rows, dQ, q_rows, d, ld, dQb=None):
        out = np.zeros(2, dtype=np.float64)
        self._call("scores_device", C.c_void_p(dP), int(p_rows), C.c_void_p(dQ), int(q_rows), int(d), int(ld), C.c_void_p(dQb or 0),
                   int(q_rows) if dQb else 0, _ptr(out, C.c_double))
        return {"rmse": out[0].item(), "error": out[1].item()}


def sample_rows(rows, eval_samples):
    """validation.eval_samples (evaluate/base.py:58-60): the random draw stays in Python, the evaluator takes the subset."""
    rows = np.asarray(rows)
    if not eval_samples:
        return rows
    return np.random.choice(rows, size=min(int(eval_samples), len(rows)), replace=False)


class DeviceEvaluable:
    """Mixin for a front with ``self.data`` (groups ``rowwise`` and ``vali``), ``self.opt`` and the factors ``self.P`` / ``self.Q``
    [/ ``self.Qb`` with ``opt.use_bias``]: put it in front of ``Evaluable`` in the bases.  The evaluator is bound to the data set on first
    use.  A front whose backend keeps the current factors in HBM sets ``validation_on_device = True``: the factors are then read
    through ``self.obj.device_buffer`` and nothing but the result crosses PCIe.

    ``validation_score_func`` is ``"dot"`` unless the front sets ``"l2"`` itself; it is NOT derived from ``opt.score_func``: the
    reference's own front validates an ``"l2"`` model by dot product (its option is lower-cased, its comparisons read ``"L2"``), and a
    drop-in must not silently differ.  Under ``"l2"`` the lists are ranked by squared distance, the predictions are ``1 - distance`` and
    no bias is passed."""

    validation_on_device = False
    validation_score_func = "dot"

    def _evaluator(self):
        cached = getattr(self, "_device_evaluator", None)
        if cached is not None and cached[0] is self.data:
            return cached[1]
        header = self.data.get_header()
        tr, va = self.data.get_group("rowwise"), self.data.get_group("vali")
        ev = Evaluator()
        if self.validation_score_func != "dot":      # "dot" is the handle's default: nothing to set
            ev.set_score_func(self.validation_score_func)
        ev.set_data(header["num_users"], header["num_items"], np.ascontiguousarray(tr["indptr"], dtype=np.int64),
                    np.ascontiguousarray(tr["key"], dtype=np.int32), np.ascontiguousarray(va["row"], dtype=np.int32),
                    np.ascontiguousarray(va["col"], dtype=np.int32), np.ascontiguousarray(va["val"], dtype=np.float32))
        self._vali_rows = np.unique(np.asarray(va["row"], dtype=np.int32))
        self._device_evaluator = (self.data, ev)
        return ev

    def _validation_factors(self):
        """(device?, arguments of Evaluator.ranking[_device] / scores[_device])."""
        d = self.opt.d
        bias = bool(getattr(self.opt, "use_bias", False)) and getattr(self, "Qb", None) is not None and self.validation_score_func != "l2"
        if self.validation_on_device:
            header = self.data.get_header()
            dQb = self.obj.device_buffer("Qb")[0] if bias else None
            return True, (self.obj.device_buffer("P")[0], header["num_users"], self.obj.device_buffer("Q")[0], header["num_items"], d,
                          self.obj.get_vdim(), dQb)
        P = np.ascontiguousarray(self.P[:, :d], dtype=np.float32)
        Q = np.ascontiguousarray(self.Q[:, :d], dtype=np.float32)
        return False, (P, Q, np.asarray(self.Qb, dtype=np.float32) if bias else None)

    def get_validation_results(self, topk=None):
        if not self.data.has_group("vali"):
            return {}
        factors = self._validation_factors()       # once for both passes: the host branch copies P and Q
        results = {}
        results.update(self._evaluate_ranking_metrics(topk, factors))
        results.update(self._evaluate_score_metrics(factors))
        return results

    def _evaluate_ranking_metrics(self, topk=None, factors=None):
        validation = self.opt.validation or {}
        topk = int(topk or validation.get("topk", 10))
        ev = self._evaluator()
        samples = validation.get("eval_samples", 0)
        rows = sample_rows(self._vali_rows, samples) if samples else None
        on_device, args = factors or self._validation_factors()
        res = (ev.ranking_device if on_device else ev.ranking)(*args, rows=rows, topk=topk)
        if res.pop("N") == 0:
            return {}
        return res

    def _evaluate_score_metrics(self, factors=None):
        ev = self._evaluator()
        on_device, args = factors or self._validation_factors()
        return (ev.scores_device if on_device else ev.scores)(*args)


__all__ = ["Evaluator", "DeviceEvaluable", "sample_rows", "RANKING_KEYS"]
