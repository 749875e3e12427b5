"""Float64 run of the eALS recurrence (He et al., SIGIR'16, as CEALS drives it: lib/algo_impl/eals/eals.cc) -- the yardstick of the
eALS envelope tests, what tests/f64_backend.py is for ALS.  Written from the oracle's `EALS` class (oracle/buffalo_oracle.cc) and the
formulas quoted in csrc/eals_kernels.hpp (eals.cc:196-216, 261-262, 122-150); no float32 anywhere between the calls.

`F64EALS` has CyEALS's surface (init, initialize_model, precompute_cache, update, estimate_loss).  It copies the caller's float32
factors ONCE (initialize_model) and keeps P, Q, both vhat caches and the index maps in float64 from then on; `factors()` hands out
its P and Q.  A backend's distance from this run is its own rounding, amplified by the conditioning of the case, so a HIP run is
held to `err(hip, f64) <= 2.5 x err(oracle, f64) + 4 ulp` (`bound`).

The rows of a half-epoch are independent (a row reads and writes its own entries of the cache of ITS orientation; the mirror is
only read by the other half-epoch), so one coordinate step is done for all rows at once: np.bincount over the row index forms the
numerator and the denominator, `X @ S[d]` the Gramian term with the current X, then the new coordinate is folded into vhat.

`defect=` (tests/test_eals_ref_cpu.py only) plants one single-point mistake into the rows above `defect_min_len` entries, to show
that the envelope bound would catch it:
  drop_last_entry_one_dim   the row's last entry is left out of the numerator and denominator in the last dimension
  skip_block_close          the vhat fold of dimension 15 is lost (the close of the first 16-dimension block)
  stale_vhat_last_entry     the fold into the row's last entry is skipped in dimension 0
"""
import json

import numpy as np

DEFECTS = ("drop_last_entry_one_dim", "skip_block_close", "stale_vhat_last_entry")
ULP32 = 2.0 ** -23


def relerr(a, b):
    """helpers.relerr: max abs difference over the largest entry of b (b = the float64 side)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def bound(err_oracle):
    """The envelope of a device run: 2.5 x the oracle's own distance (the ALS envelope of f64_backend.py) + four float32 ulps of
    the largest entry (the final rounding to float32, the division and the last reduction, where both errors sit at 1e-7)."""
    return 2.5 * err_oracle + 4 * ULP32


def loss_bound(loss_oracle, loss_f64):
    """The device loss accumulates in double, so it gets no margin over the oracle's float accumulators; the additive term is the
    rounding of the float return value."""
    return abs(loss_oracle - loss_f64) + 8 * 2.0 ** -24 * abs(loss_f64)


class F64EALS:
    def __init__(self, defect=None, defect_min_len=4096):
        assert defect is None or defect in DEFECTS, defect
        self.defect, self.defect_min_len = defect, defect_min_len
        self.P = self.Q = self.C = None
        self.cached = [False, False]
        self.vhat, self.map, self.rows, self.keys, self.indptr = [None, None], [None, None], [None, None], [None, None], [None, None]

    def init(self, opt_path):
        with open(opt_path) as f:
            opt = json.load(f)
        self.d, self.alpha, self.reg = int(opt["d"]), float(np.float32(opt["alpha"])), (float(np.float32(opt["reg_u"])), float(np.float32(opt["reg_i"])))
        return True

    def initialize_model(self, P, Q, Cw):
        assert P.shape[1] == self.d and Q.shape[1] == self.d and Cw.shape[0] == Q.shape[0]
        self.P, self.Q, self.C = P.astype(np.float64), Q.astype(np.float64), Cw.astype(np.float64)
        self.cached = [False, False]

    def factors(self):
        return self.P, self.Q

    def _sides(self, axis):
        return (self.P, self.Q) if axis == 0 else (self.Q, self.P)

    # eals.cc:49-100
    def precompute_cache(self, nnz, indptr, keys, axis):
        if self.cached[axis]:
            return
        X, Y = self._sides(axis)
        assert indptr.shape[0] == X.shape[0] and int(indptr[-1]) == nnz == keys.shape[0]
        cnt = np.diff(np.concatenate([[0], indptr]))
        rows = np.repeat(np.arange(X.shape[0]), cnt)
        self.vhat[axis] = np.einsum("nd,nd->n", X[rows], Y[keys])
        order = np.lexsort((rows, keys))            # position r of the other orientation holds own position order[r]
        mp = np.empty(nnz, np.int64)
        mp[order] = np.arange(nnz)
        self.map[axis], self.rows[axis], self.keys[axis], self.indptr[axis] = mp, rows, keys.astype(np.int64), indptr.astype(np.int64)
        self.cached[axis] = True

    def _gram(self, axis):
        """S of the update of `axis`: 0 -> sum_i c_i q q^T (eals.cc:179-191), 1 -> P^T P (:234-235)."""
        return (self.Q * self.C[:, None]).T @ self.Q if axis == 0 else self.P.T @ self.P

    # eals.cc:102-115, 176-281
    def update(self, indptr, keys, vals, axis):
        if not (self.cached[0] and self.cached[1]):
            return False
        X, Y = self._sides(axis)
        D, n_rows = self.d, X.shape[0]
        r, k, own = self.rows[axis], self.keys[axis], self.vhat[axis]
        v = vals.astype(np.float64)
        w = 1.0 + self.alpha * v
        wmc = w - (self.C[k] if axis == 0 else self.C[r])
        wv = w * v
        S = self._gram(axis)
        cx = self.C if axis == 1 else None
        reg = self.reg[axis]
        last = None
        if self.defect:
            end = self.indptr[axis]
            cnt = np.diff(np.concatenate([[0], end]))
            last = end[cnt > self.defect_min_len] - 1       # the last entry of every row the defect applies to
        for d in range(D):
            yd = Y[k, d]
            xd = X[:, d].copy()
            vf = own - xd[r] * yd
            tn, td = (wv - wmc * vf) * yd, wmc * yd * yd
            if self.defect == "drop_last_entry_one_dim" and d == D - 1:
                tn[last] = 0.0
                td[last] = 0.0
            num = np.bincount(r, weights=tn, minlength=n_rows)
            den = np.bincount(r, weights=td, minlength=n_rows)
            dot = X @ S[d]
            if axis == 0:       # eals.cc:214-215
                num += -dot + xd * S[d, d]
                den += S[d, d] + reg
            else:               # eals.cc:261-262
                num += -cx * (dot - xd * S[d, d])
                den += cx * S[d, d] + reg
            xn = num / den
            X[:, d] = xn
            fold = xn[r] * yd
            if self.defect == "skip_block_close" and d == 15:
                fold[np.isin(r, r[last])] = 0.0
            if self.defect == "stale_vhat_last_entry" and d == 0:
                fold[last] = 0.0
            own = vf + fold
        self.vhat[axis] = own
        self.vhat[1 - axis][self.map[axis]] = own
        return True

    # eals.cc:117-174: the objective from the caches
    def estimate_loss(self, nnz, indptr, keys, vals, axis):
        if not (self.cached[0] and self.cached[1]):
            return 0.0, 0.0
        assert nnz == self.vhat[axis].shape[0]
        v, vh = vals.astype(np.float64), self.vhat[axis]
        c = self.C[self.keys[axis]] if axis == 0 else self.C[self.rows[axis]]
        err = v - vh
        fb = ((1.0 + self.alpha * v) * err * err - c * vh * vh).sum()
        ip = ((self.P.T @ self.P) * ((self.Q * self.C[:, None]).T @ self.Q)).sum()       # <S^p, S^q> = sum_ui c_i (p_u . q_i)^2
        reg = self.reg[0] * (self.P ** 2).sum() + self.reg[1] * (self.Q ** 2).sum()
        return float(np.sqrt((err * err).sum() / max(nnz, 1))), float(fb + ip + reg)

    def dense_loss(self, indptr, keys, vals):
        """The objective recomputed from P and Q alone, every (user, item) cell written out (small cases): user-major arrays."""
        U, I = self.P.shape[0], self.Q.shape[0]
        rows = np.repeat(np.arange(U), np.diff(np.concatenate([[0], indptr])))
        Sc = self.P @ self.Q.T
        W = np.tile(self.C, (U, 1))
        R = np.zeros((U, I))
        R[rows, keys] = vals
        W[rows, keys] = 1.0 + self.alpha * vals.astype(np.float64)
        return float((W * (R - Sc) ** 2).sum() + self.reg[0] * (self.P ** 2).sum() + self.reg[1] * (self.Q ** 2).sum())
