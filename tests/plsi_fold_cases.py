"""Yardstick and cases the pLSI fold-in tests share (test_plsi_fold_in_cpu.py, test_plsi_fold_in_gpu.py).

bfh_plsi_fold_in computes, for every history b with entries (c_j, v_j), n_b of them, against a frozen Q, from p(0) = init[b] (or 1 / d):

    acc_k  = sum_j max(p(t-1)_k Q[c_j, k], 1e-10f) / norm_j * v_j        norm_j = sum_k max(...)
    p(t)_k = (acc_k + a1) / sum_k (acc_k + a1)                            a1 = alpha1 / float(d),   t = 1 .. iters
    loss[b] = -sum_j log(norm_j) v_j of the last step

`fold_ref` is that, built from ref_plsi.accumulate / ref_plsi.normalize with Q put back after every step: in float64, and in float32 as the
reference's one-worker arithmetic.  One step from identical inputs is held to ref_plsi.bound_normalized(n_b, d, d) per element (the forward
error of the sums in ANY order, see ref_plsi); free-running steps to e_hip <= max(2.5 e32, that bound), the rule of tests/test_plsi_gpu.py.
"""
import functools

import numpy as np

import ref_plsi as R
from buffalo_amd.synth import CSR

SEG = 2048            # kPlsiSeg of csrc/plsi_fold_kernels.hpp
ITEMS = 300
DEFECTS = ("drop_last_entry", "no_smoothing", "skip_clamp", "wrong_q_row")


def layout(d):
    """(G, C, U) of the kernels at d: lanes of a group, float4 chunks per lane, entries in flight per group."""
    vdim = (d + 31) // 32 * 32
    G = 8
    while G < 64 and G * 4 < vdim:
        G *= 2
    C = 1
    while G * 4 * C < vdim:
        C *= 2
    return G, C, 4 if C == 1 else 2


def named_lengths(d, empty=True):
    """The row lengths at which the kernel takes another path at d: no entry, one, both sides of the short / team bound, one less, exactly and one
    more than a full set of in-flight entries (of one group walking alone, and of every group of a team), both sides of a segment, three segments."""
    G, C, U = layout(d)
    NG = 64 // G
    short_max = 2 * NG if NG > 1 else 0
    want = [0, 1, short_max, short_max + 1, U - 1, U, U + 1, NG * (U - 1), NG * U, NG * (U + 1), SEG - 1, SEG, SEG + 1, 2 * SEG + 1]
    out = []
    for n in want:
        if n not in out and (n > 0 or empty):
            out.append(n)
    return out


@functools.lru_cache(maxsize=None)
def pattern(d, values="ratings", empty=True, fill=150, seed=3):
    """The named lengths of `d` in rows 0 .., then `fill` rows of 1 .. 40 entries.  Keys are drawn with repetition from 300 items."""
    rng = np.random.default_rng(seed)
    lengths = np.array(named_lengths(d, empty) + list(rng.integers(1, 41, size=fill)), dtype=np.int64)
    nnz = int(lengths.sum())
    keys = rng.integers(0, ITEMS, size=nnz).astype(np.int32)
    if values == "ratings":
        vals = rng.integers(1, 6, size=nnz)
    elif values == "counts":
        vals = 1 + rng.poisson(1.0, size=nnz)
    else:
        vals = np.ones(nnz)
    m = CSR(lengths.shape[0], ITEMS, np.cumsum(lengths, dtype=np.int64), keys, vals.astype(np.float32))
    for a in (m.indptr, m.keys, m.vals):
        a.setflags(write=False)
    return m


def lengths_of(m):
    return R.entry_counts(m)[0]


def rows_of(m):
    beg = np.concatenate([[0], m.indptr[:-1]])
    return [(int(b), int(e)) for b, e in zip(beg, m.indptr)]


def take(m, rows):
    """The histories `rows` of m, in that order, as a CSR of their own."""
    bounds = rows_of(m)
    sel = [np.arange(*bounds[r]) for r in rows]
    idx = np.concatenate(sel) if sel else np.zeros(0, dtype=np.int64)
    return CSR(len(rows), m.num_items, np.cumsum([s.shape[0] for s in sel], dtype=np.int64), m.keys[idx], m.vals[idx])


def uniform(n, d):
    return np.full((n, d), np.float32(1.0) / np.float32(d), dtype=np.float32)


def row_losses(P, Q, csr, dtype=np.float64):
    """-sum_j log(norm_j) v_j per row from the old rows P: float64, or float32 with every operation rounded and the terms added in entry order."""
    dtype = np.dtype(dtype)
    rows, keys = R.entry_rows(csr), csr.keys.astype(np.int64)
    lat = np.maximum(P.astype(dtype)[rows] * Q.astype(dtype)[keys], dtype.type(R.CLAMP))
    if dtype == np.float64:
        norm = lat.sum(axis=1)
    else:
        norm = np.zeros(lat.shape[0], dtype=dtype)
        for k in range(lat.shape[1]):
            norm = norm + lat[:, k]
    terms = (np.log(norm) * csr.vals.astype(dtype)).astype(dtype)
    out = np.zeros(csr.num_users, dtype=dtype)
    np.subtract.at(out, rows, terms)
    return out


def _planted(P, Q, csr, defect, row):
    """The inputs of one step with `defect` planted in history `row` -> (P, Q, csr, skip_smoothing_row)."""
    bounds = rows_of(csr)
    b, e = bounds[row]
    if defect == "drop_last_entry":
        vals = csr.vals.copy()
        vals[e - 1] = 0            # the entry adds nothing
        csr = CSR(csr.num_users, csr.num_items, csr.indptr, csr.keys, vals)
    elif defect == "wrong_q_row":
        keys = csr.keys.copy()
        keys[b] = (keys[b] + 1) % csr.num_items
        csr = CSR(csr.num_users, csr.num_items, csr.indptr, keys, csr.vals)
    return P, Q, csr


def step(P, Q, csr, alpha1, dtype=np.float64, defect=None, defect_row=None):
    """One fold-in step of every row from the rows P: ref_plsi.accumulate with Q as it is, then ref_plsi.normalize.  `defect` (one of DEFECTS)
    is planted in history `defect_row` only."""
    dtype = np.dtype(dtype)
    if defect in ("drop_last_entry", "wrong_q_row"):
        P, Q, csr = _planted(P, Q, csr, defect, defect_row)
    Pn, Qn, _ = R.accumulate(P, Q, csr, dtype)
    if defect == "skip_clamp":     # that row's sums without the max(., 1e-10)
        one = take(csr, [defect_row])
        rows, keys = R.entry_rows(one), one.keys.astype(np.int64)
        lat = P.astype(dtype)[[defect_row]][rows] * Q.astype(dtype)[keys]
        Pn[defect_row] = ((lat / lat.sum(axis=1, dtype=dtype)[:, None]) * one.vals.astype(dtype)[:, None]).sum(axis=0, dtype=dtype)
    out, _ = R.normalize(Pn, Qn, alpha1, 1.0, dtype)
    if defect == "no_smoothing":
        out[defect_row] = R.normalize(Pn[[defect_row]], Qn, 0.0, 1.0, dtype)[0][0]
    return out


def fold_ref(init, Q, csr, iters, alpha1, dtype=np.float64):
    """The definition above in `dtype`: (rows after `iters` steps [n, d], per-row loss of the last step).  init None: the uniform start."""
    dtype = np.dtype(dtype)
    P = (uniform(csr.num_users, Q.shape[1]) if init is None else init).astype(dtype)
    loss = np.zeros(csr.num_users, dtype=dtype)
    for _ in range(iters):
        loss = row_losses(P, Q, csr, dtype)
        P = step(P, Q, csr, alpha1, dtype)
    return P, loss


def ratio(a, ref, bound):
    """Largest elementwise |a - ref| / (|ref| * bound); a == ref counts as 0, anything not finite as inf."""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(a - ref) / (np.abs(ref) * bound)
    r[a == ref] = 0.0
    r[~np.isfinite(r)] = np.inf
    return float(r.max()) if r.size else 0.0


def one_step_bound(m, d):
    """ref_plsi.bound_normalized(n_b, d, d) per row, as a column."""
    return R.bound_normalized(lengths_of(m), d, d)[:, None]


@functools.lru_cache(maxsize=None)
def start(n_rows, d, seed=11):
    """(init rows, Q) with a sprinkle of tiny factors (ref_plsi.clamped_start), so that some products fall below the clamp."""
    P, Q = R.clamped_start(n_rows, ITEMS, d, seed)
    P.setflags(write=False)
    Q.setflags(write=False)
    return P, Q


def clamp_is_reached(P, Q, m):
    return bool((P[R.entry_rows(m)].astype(np.float64) * Q[m.keys].astype(np.float64) < 1e-10).any())
