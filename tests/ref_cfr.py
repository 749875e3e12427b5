"""Float64 run of the CoFactor row updates (CCFR, lib/algo_impl/cfr/cfr.cc:92-313, as restated in the header of csrc/cfr_impl.hpp)
-- the yardstick of the CFR envelope tests, what tests/f64_backend.py is for ALS and tests/ref_eals.py for eALS.

  user     A = l (FF_I + sum alpha v i i^T) + reg_u I                  y = l sum (1 + alpha v) i
  item     A = l (FF_U + sum alpha v u u^T) + sum c c^T + reg_i I      y = l sum (1 + alpha v) u + sum (v - Ib_x - Cb_c) c
  context  A = sum i i^T + reg_c I                                     y = sum (v - Cb_x - Ib_i) i
followed, for item and context rows, by the bias refresh from the UPDATED row: b = sum (v - x . other_c - bias_other_c) / (n + 1e-10)
(cfr.cc:242-249, 303-310; an item solved because of its user entries alone gets 0 / 1e-10 = 0).  Rows without entries are skipped.

`F64CFR` has CyCFR's surface (init, set_embedding, precompute, the three partial_update_* calls, each returning its loss).  It copies
the caller's float32 arrays ONCE per set_embedding and keeps all five in float64 from then on; after an update the rows of the call
are written back to the bound float32 arrays, as the other backends do.  llt / ldlt are np.linalg.solve; manual_cg is
ref_numpy.manual_cg_f64 from the row before the update with tolerance 0 (`cg_tolerance_`, cfr.cc:40: the key nobody sets).  The
losses are the reference's terms (cfr.cc:145-149, 193-205, 219-233, 300-301, 313) summed in float64.

A backend's distance from this run is its own rounding, amplified by the conditioning of the case, so a HIP run is held to
`err(hip, f64) <= 2.5 x err(oracle, f64) + 4 ulp` (`ref_eals.bound`), per array, biases included.

`defect=` (tests/test_cfr_ref_cpu.py only) plants one single-point mistake, to show that the envelope bound would catch it:
  ctx_pad_lane      a context row with an odd entry count also consumes row 0 of the other factor at weight 1, with coefficient
                    -bias_self (the padding lane of the row's last pair taken at weight 1 instead of 0)
  drop_chunk_tail   the last entry of a row above 4,096 entries is left out of A and y in the context pass
  y_not_scaled      `l` is applied to A of the user-item pass but not to y
"""
import json

import numpy as np

import ref_numpy as rn
from ref_eals import bound, loss_bound, relerr  # noqa: F401  (the envelope is eALS's: imported, not copied)

DEFECTS = ("ctx_pad_lane", "drop_chunk_tail", "y_not_scaled")
ARRAYS = ("user", "item", "context", "item_bias", "context_bias")
HEAVY = 4096        # csrc/als_core.hpp: rows above this are cut into chunks that add into one slot


def _f32(x):
    return float(np.float32(x))


class F64CFR:
    def __init__(self, defect=None):
        assert defect is None or defect in DEFECTS, defect
        self.defect = defect
        self.F, self.host, self.FF = {}, {}, None

    def init(self, opt_path):
        path = opt_path.decode("utf-8") if isinstance(opt_path, bytes) else opt_path
        with open(path) as f:
            o = json.load(f)
        assert o["optimizer"] in ("llt", "ldlt", "manual_cg"), "float64 stand-in: dense solves only"
        self.d, self.optimizer, self.iters = int(o["d"]), o["optimizer"], int(o["num_cg_max_iters"])
        self.alpha, self.l, self.eps = _f32(o["alpha"]), _f32(o["l"]), _f32(o.get("eps", 1e-10))
        self.reg = {"user": _f32(o["reg_u"]), "item": _f32(o["reg_i"]), "context": _f32(o["reg_c"])}
        self.compute_loss = bool(o.get("compute_loss", False))
        self.F, self.host, self.FF = {}, {}, None
        return True

    def set_embedding(self, F, obj_type):
        t = obj_type.decode("utf-8") if isinstance(obj_type, bytes) else obj_type
        assert t in ARRAYS and F.dtype == np.float32 and F.shape[1] == (1 if t.endswith("bias") else self.d), (t, F.shape)
        self.host[t], self.F[t] = F, F.astype(np.float64)

    def precompute(self, obj_type):
        t = obj_type.decode("utf-8") if isinstance(obj_type, bytes) else obj_type
        assert t in ("user", "item"), t
        self.FF = self.F[t].T @ self.F[t]

    # ---- pieces -------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _row(indptr, keys, vals, x, shift):
        b = (0 if x == 0 else int(indptr[x - 1])) - shift
        e = int(indptr[x]) - shift
        return keys[b:e], vals[b:e].astype(np.float64)

    def _solve(self, x0, A, y):
        if self.optimizer == "manual_cg":
            return rn.manual_cg_f64(x0, A, y, iters=self.iters, tol=0.0, eps=self.eps)
        return np.linalg.solve(A, y)

    def _weighted_part(self, Y, k, v):
        """l (FF + sum alpha v q q^T), l sum (1 + alpha v) q  (cfr.cc:126-140, 190-214)."""
        Ys = Y[k]
        A = self.l * (self.FF + (Ys * (self.alpha * v)[:, None]).T @ Ys)
        y = ((1.0 + self.alpha * v)[:, None] * Ys).sum(axis=0)
        return A, (y if self.defect == "y_not_scaled" else self.l * y)

    def _context_part(self, Y, k, v, b_self, b_other):
        """sum q q^T, sum (v - b_self - b_other[key]) q  (cfr.cc:216-235, 289-296)."""
        Ys, coeff = Y[k], v - b_self - b_other[k, 0]
        if self.defect == "drop_chunk_tail" and k.shape[0] > HEAVY:
            Ys, coeff = Ys[:-1], coeff[:-1]
        A, y = Ys.T @ Ys, coeff @ Ys
        if self.defect == "ctx_pad_lane" and k.shape[0] % 2 == 1:
            A, y = A + np.outer(Y[0], Y[0]), y - b_self * Y[0]
        return A, y

    def item_system(self, x, ku, vu, kc, vc):
        """A and y of item row x from its user entries (ku, vu) and its context entries (kc, vc), before the solve."""
        A, y = self._weighted_part(self.F["user"], ku, vu)
        Ac, yc = self._context_part(self.F["context"], kc, vc, self.F["item_bias"][x, 0], self.F["context_bias"])
        return A + Ac + self.reg["item"] * np.eye(self.d), y + yc

    def item_loss(self, x, ku, vu, kc, vc):
        """cfr.cc:193-205, 219-233 on the row BEFORE its update, with the FF trick of the reference."""
        ix = self.F["item"][x]
        dot = self.F["user"][ku] @ ix
        loss = self.l * (float(ix @ self.FF @ ix) + float((-dot * dot + (1.0 + self.alpha * vu) * (dot - 1.0) ** 2).sum()))
        err = vc - self.F["context"][kc] @ ix - self.F["item_bias"][x, 0] - self.F["context_bias"][kc, 0]
        return loss + float(err @ err) + self.reg["item"] * float(ix @ ix)

    def _write_back(self, names, start_x, next_x):
        for t in names:
            self.host[t][start_x:next_x] = self.F[t][start_x:next_x].astype(np.float32)

    # ---- cfr.cc:92-150 ------------------------------------------------------------------------------------------------------
    def partial_update_user(self, start_x, next_x, indptr, keys, vals):
        if next_x == start_x:
            return 0.0
        Uf, If = self.F["user"], self.F["item"]
        shift = 0 if start_x == 0 else int(indptr[start_x - 1])
        loss = 0.0
        for x in range(start_x, next_x):
            k, v = self._row(indptr, keys, vals, x, shift)
            if k.shape[0] == 0:
                continue
            A, y = self._weighted_part(If, k, v)
            Uf[x] = self._solve(Uf[x], A + self.reg["user"] * np.eye(self.d), y)
            loss += float(Uf[x] @ Uf[x])
        self._write_back(("user",), start_x, next_x)
        return self.reg["user"] * loss if self.compute_loss else 0.0

    # ---- cfr.cc:152-253 -----------------------------------------------------------------------------------------------------
    def partial_update_item(self, start_x, next_x, indptr_u, keys_u, vals_u, indptr_c, keys_c, vals_c):
        if next_x == start_x:
            return 0.0
        If, Cf, Ib, Cb = self.F["item"], self.F["context"], self.F["item_bias"], self.F["context_bias"]
        shift_u = 0 if start_x == 0 else int(indptr_u[start_x - 1])
        shift_c = 0 if start_x == 0 else int(indptr_c[start_x - 1])
        loss = 0.0
        for x in range(start_x, next_x):
            ku, vu = self._row(indptr_u, keys_u, vals_u, x, shift_u)
            kc, vc = self._row(indptr_c, keys_c, vals_c, x, shift_c)
            if ku.shape[0] == 0 and kc.shape[0] == 0:
                continue
            if self.compute_loss:
                loss += self.item_loss(x, ku, vu, kc, vc)
            A, y = self.item_system(x, ku, vu, kc, vc)
            If[x] = self._solve(If[x], A, y)
            Ib[x, 0] = float((vc - Cf[kc] @ If[x] - Cb[kc, 0]).sum()) / (kc.shape[0] + 1e-10)
        self._write_back(("item", "item_bias"), start_x, next_x)
        return loss

    # ---- cfr.cc:255-314 -----------------------------------------------------------------------------------------------------
    def partial_update_context(self, start_x, next_x, indptr, keys, vals):
        if next_x == start_x:
            return 0.0
        If, Cf, Ib, Cb = self.F["item"], self.F["context"], self.F["item_bias"], self.F["context_bias"]
        shift = 0 if start_x == 0 else int(indptr[start_x - 1])
        loss = 0.0
        for x in range(start_x, next_x):
            k, v = self._row(indptr, keys, vals, x, shift)
            if k.shape[0] == 0:
                continue
            A, y = self._context_part(If, k, v, Cb[x, 0], Ib)
            loss += float(Cf[x] @ Cf[x])                    # the row BEFORE the update (cfr.cc:300-301)
            Cf[x] = self._solve(Cf[x], A + self.reg["context"] * np.eye(self.d), y)
            Cb[x, 0] = float((v - If[k] @ Cf[x] - Ib[k, 0]).sum()) / (k.shape[0] + 1e-10)
        self._write_back(("context", "context_bias"), start_x, next_x)
        return self.reg["context"] * loss if self.compute_loss else 0.0
