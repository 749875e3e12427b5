"""numpy restatement of pLSI's EM epoch, written from the reference's lib/algo_impl/plsi/plsi.cc (CPLSI::partial_update :72-105,
normalize :107-125, swap :127-130) -- the yardstick of tests/test_plsi_gpu.py and tests/test_front_plsi_gpu.py.

There is no reference BINARY to pin against: plsi.cc does not compile against oracle/stand_in_3rd (the Eigen stand-in has no
`sum` / `cwiseMax`), so this file is a restatement and tests/test_plsi_ref_cpu.py pins it against a closed form instead.

Two precisions of one function:
  * float64 -- the mathematical epoch evaluated from the float32 inputs (order of the sums immaterial at 2^-53);
  * float32 -- the reference's arithmetic with ONE worker: entries in storage order, every operation rounded to float32 where plsi.cc
    rounds it (product, clamp, the sum over k front to back, latent / norm, * v, the += into P and Q, the float loss).  With more workers the
    reference's Q sums are a data race; one worker is the yardstick.
For every stored entry (x, c, v):
    latent_k = max(P_old[x,k] * Q_old[c,k], 1e-10f);  norm = sum_k latent_k;  loss -= log(norm) * v
    P_new[x,:] += latent / norm * v;  Q_new[c,:] += latent / norm * v
"""
import json

import numpy as np

CLAMP = np.float32(1e-10)   # `cwiseMax(1e-10)` on a VectorXf: the constant is a float
U24 = 2.0 ** -24            # unit roundoff of float32


def entry_rows(csr):
    beg = np.concatenate([[0], csr.indptr[:-1]])
    return np.repeat(np.arange(csr.num_users, dtype=np.int64), csr.indptr - beg)


def accumulate(P, Q, csr, dtype=np.float64):
    """The sums of plsi.cc:91-101 over the whole matrix from the old model (P, Q) -> (P_new, Q_new, loss), before normalize."""
    dtype = np.dtype(dtype)
    rows, keys = entry_rows(csr), csr.keys.astype(np.int64)
    v = csr.vals.astype(dtype)
    lat = np.maximum(P.astype(dtype)[rows] * Q.astype(dtype)[keys], dtype.type(CLAMP))
    if dtype == np.float64:
        norm = lat.sum(axis=1)
    else:   # front to back over k, each partial sum rounded
        norm = np.zeros(lat.shape[0], dtype=dtype)
        for k in range(lat.shape[1]):
            norm = norm + lat[:, k]
    contrib = (lat / norm[:, None]) * v[:, None]
    Pn, Qn = np.zeros(P.shape, dtype=dtype), np.zeros(Q.shape, dtype=dtype)
    if dtype == np.float64:
        import scipy.sparse as sp
        n = rows.shape[0]
        ones, idx = np.ones(n), np.arange(n)
        Pn[:] = sp.csr_matrix((ones, (rows, idx)), shape=(P.shape[0], n)) @ contrib
        Qn[:] = sp.csr_matrix((ones, (keys, idx)), shape=(Q.shape[0], n)) @ contrib
        loss = -float(np.sum(np.log(norm) * v))
    else:   # ufunc.at applies the additions one by one in entry order: the one-worker order of the reference
        np.add.at(Pn, rows, contrib)
        np.add.at(Qn, keys, contrib)
        terms = (np.log(norm) * v).astype(dtype)
        loss = -float(np.cumsum(terms, dtype=dtype)[-1]) if terms.size else 0.0
    return Pn, Qn, loss


def normalize(Pn, Qn, alpha1, alpha2, dtype=np.float64):
    """plsi.cc:107-125 (alpha1 / d and alpha2 / num_items are float divisions there)."""
    dtype = np.dtype(dtype)
    d, num_items = Pn.shape[1], Qn.shape[0]
    a1 = dtype.type(np.float32(alpha1) / np.float32(d))
    a2 = dtype.type(np.float32(alpha2) / np.float32(num_items))
    Pn = Pn.astype(dtype) + a1
    Qn = Qn.astype(dtype) + a2
    with np.errstate(invalid="ignore", divide="ignore"):
        if dtype == np.float64:
            Pn = Pn / Pn.sum(axis=1, keepdims=True)
            Qn = Qn / Qn.sum(axis=0, keepdims=True)
        else:
            ps = np.zeros(Pn.shape[0], dtype=dtype)
            for k in range(d):
                ps = ps + Pn[:, k]
            qs = np.zeros(d, dtype=dtype)
            for i in range(num_items):
                qs = qs + Qn[i]
            Pn, Qn = Pn / ps[:, None], Qn / qs[None, :]
    return Pn, Qn


def epoch(P, Q, csr, alpha1=1.0, alpha2=1.0, dtype=np.float64):
    """reset -> partial_update over everything -> normalize -> swap: (P', Q', loss) in `dtype`."""
    Pn, Qn, loss = accumulate(P, Q, csr, dtype)
    Pn, Qn = normalize(Pn, Qn, alpha1, alpha2, dtype)
    return Pn, Qn, loss


def relerr_elements(a, b):
    """Largest |a - b| / |b| over the elements (0 where both are 0)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(a - b) / np.abs(b)
    r[(a == b)] = 0.0
    return float(np.max(r)) if r.size else 0.0


def init_model(num_users, num_items, d, seed):
    """The reference's initial DISTRIBUTION (plsi.cc:52-66): |N(0, 1/d)|, rows of P and columns of Q sum to 1."""
    rng = np.random.default_rng(seed)
    P = np.abs(rng.normal(scale=1.0 / d, size=(num_users, d)))
    Q = np.abs(rng.normal(scale=1.0 / d, size=(num_items, d)))
    P /= P.sum(axis=1, keepdims=True)
    Q /= Q.sum(axis=0, keepdims=True)
    return np.ascontiguousarray(P, dtype=np.float32), np.ascontiguousarray(Q, dtype=np.float32)


class RefPLSI:
    """The float64 restatement behind CyPLSI's method surface (buffalo/algo/_plsi.pyx), so the front of
    tests/front_harness/buffalo_front/algo/plsi.py can drive it.  The model stays float64 between epochs; the caller's float32 arrays
    are rewritten at swap().  `initialize_model` keeps the arrays it is handed as the start (the tests hand both backends one start)."""

    def init(self, opt_path):
        with open(opt_path.decode() if isinstance(opt_path, bytes) else opt_path) as f:
            self.opt = json.load(f)
        self.d = int(self.opt["d"])
        return True

    def initialize_model(self, P, Q):
        self.P, self.Q = P, Q
        self.P64, self.Q64 = P.astype(np.float64), Q.astype(np.float64)

    def synchronize(self, device_to_host):
        if device_to_host:
            self.P[:], self.Q[:] = self.P64, self.Q64
        else:
            self.P64, self.Q64 = self.P.astype(np.float64), self.Q.astype(np.float64)

    def reset(self):
        self.Pn, self.Qn = np.zeros_like(self.P64), np.zeros_like(self.Q64)

    def partial_update(self, start_x, next_x, indptr, keys, vals):
        from buffalo_amd.synth import CSR
        beg = 0 if start_x == 0 else int(indptr[start_x - 1])
        ends = np.zeros(self.P.shape[0], dtype=np.int64)
        ends[start_x:next_x] = indptr[start_x:next_x] - beg
        ends[next_x:] = ends[next_x - 1] if next_x > 0 else 0
        Pn, Qn, loss = accumulate(self.P64, self.Q64, CSR(self.P.shape[0], self.Q.shape[0], ends, keys, vals), np.float64)
        self.Pn += Pn
        self.Qn += Qn
        return loss

    def normalize(self, alpha1, alpha2):
        self.Pn, self.Qn = normalize(self.Pn, self.Qn, alpha1, alpha2, np.float64)

    def swap(self):
        self.P64, self.Q64 = self.Pn, self.Qn
        self.P[:], self.Q[:] = self.P64, self.Q64

    def release(self):
        return


def skewed_case(num_users=1500, num_items=300, density=0.15, heavy_cols=5, seed=5, values="ratings", empty=False):
    """Test matrix: `density` overall, `heavy_cols` columns 90 % dense, values 1..5 ("ratings"), Poisson counts ("counts") or 1.0 ("ones");
    `empty`: rows 3, 4 and columns 7, 8 hold nothing.  Otherwise every row has an entry."""
    from buffalo_amd.synth import CSR
    rng = np.random.default_rng(seed)
    M = rng.random((num_users, num_items)) < density
    M[:, :heavy_cols] = rng.random((num_users, heavy_cols)) < 0.9
    M[np.arange(num_users), rng.integers(heavy_cols, num_items, size=num_users)] = True
    if empty:
        M[3:5, :] = False
        M[:, 7:9] = False
    r, c = np.nonzero(M)
    if values == "ratings":
        v = rng.integers(1, 6, size=r.shape[0])
    elif values == "counts":
        v = 1 + rng.poisson(1.0, size=r.shape[0])
    else:
        v = np.ones(r.shape[0])
    return CSR(num_users, num_items, np.cumsum(np.bincount(r, minlength=num_users), dtype=np.int64), c.astype(np.int32), v.astype(np.float32))


def clamped_start(num_users, num_items, d, seed):
    """init_model with a sprinkle of tiny factors, so that some products fall below the 1e-10 clamp of plsi.cc:94."""
    P, Q = init_model(num_users, num_items, d, seed)
    P[::7, d // 2] = 1e-7
    Q[::5, d // 2] = 1e-6
    return P, Q


def entry_counts(csr):
    """(entries per row, entries per column): the `n` of the error bounds."""
    beg = np.concatenate([[0], csr.indptr[:-1]])
    return (csr.indptr - beg).astype(np.int64), np.bincount(csr.keys, minlength=csr.num_items).astype(np.int64)


def bound_raw(n, d):
    """Relative forward error bound of one accumulator element against the float64 epoch: a sum of n non-negative terms of d + 5 roundings
    each (product, clamp-free max, d - 1 additions of the norm, the division(s), * v) plus the n - 1 additions, in ANY order."""
    return (np.asarray(n, dtype=np.float64) + d + 6) * U24


def bound_normalized(n, d, m):
    """After normalize: + the smoothing addition, the sum over m = d (a row of P) or m = rows of Q (a column of Q) and the division."""
    return (np.asarray(n, dtype=np.float64) + d + m + 10) * U24
