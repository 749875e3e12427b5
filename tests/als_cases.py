"""Shapes and drivers the ALS envelope tests share (test_als_ref_cpu.py, test_als_rows_gpu.py).

One bfh_als_partial_update chooses between five kernel families (als_handle.hpp, choose_plan): the producer / consumer pairs
(als_pc.hpp), the wave-per-row kernel in split-f16 and fp32 form (als_gram_kernel, rows solved from the accumulators), scratch slot +
als_solve_kernel, the wide kernel (als_wide_kernel, 128 < vdim <= 256) and the matrix-free fallback (als_ialspp_kernel).  `pattern`
puts a row on either side of every row-length bound those kernels have; which length sits on which branch:

  0                 skipped (work_list): the row keeps its bits
  1, 2              one group of 16 entries, 15 / 14 padding lanes (row 0 of the other factor, weight 0); fp32 form: one leftover pair,
                    half padding at 1.  Runs of one-group rows turn the two row boxes of a pair over fastest (the 8,228 rows of 3 .. 12
                    entries behind the long ones do that in every call)
  15 / 16 / 17      ng = (n + 15) >> 4 goes 1 -> 2: one padding lane, a full group, a second group of one entry
  31 / 32 / 33      ng 2 -> 3: the two register sets of the split pass of als_gram_kernel swap once / twice (odd and even group counts)
  47 / 48 / 49      ng 3 -> 4: the ring of NSLOT = 3 groups is full at 48 and wraps at 49
  63 / 64 / 65      the first 64-entry key chunk ((chunk + 1) * 4 < ng): a lane short, full, a second chunk of one entry; the batched
                    ticket draw fit = 1024 / l0 leaves its clamp of 16 at 65; fp32 form: 64-entry chunks eaten in pairs
  127 / 128 / 129   two key chunks = both staging buffers (NK = 2); the third chunk of 129 reuses staging buffer 0
  191 / 192 / 193   three / four key chunks: buffer 0 reused for a full chunk, buffer 1 for a chunk of one entry
  256 / 257         fit 4 -> 3, and the fourth chunk complete: both staging buffers used twice
  512 / 513         fit 2 -> 1
  1024 / 1025       fit = 1024 / l0 reaches 1 / would reach 0 (clamped to 1)
  4095 / 4096       the longest rows that stay one work item (HEAVY = 4096)
  4097              two work items of 2050 + 2047 entries adding into one scratch slot
  8192 / 8193       two chunks of exactly 4096 / three of 2732 + 2732 + 2729 (nch = ceil(n / 4096) goes 2 -> 3), the tail odd

`pattern_outliers`: the same matrix with weights outside the f16 path (als_defer_scan_kernel) planted AT those bounds.  `tiny_a` /
`tiny_b`: two matrices of one shape with different row bounds.

The start state is SIGNED normal(scale 0.1) for both factors: FF = F^T F is then close to N sigma^2 I (the off-diagonal sums cancel),
so the 32 x 32 blocks three CG steps are run on are well conditioned and the oracle's own distance from float64 is rounding, not
conditioning -- 1e-7 .. 1e-6 instead of the 1e-3 .. 1e-2 of the |normal| starts of test_als_gpu.py (which stay where they are).  A bound of
2.5 x that distance + 4 ulp is tight enough for ONE lost entry of one row to stick out (test_als_ref_cpu.py plants such defects).
"""
import functools
import os

import numpy as np

import helpers as H
import ref_numpy as rn
from cfr_cases import _csr, _long_rows, lengths_of
from conftest import als_opt, tiny_csr
from ref_eals import bound, relerr

NAMED_LENGTHS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 127, 128, 129, 191, 192, 193, 256, 257, 512, 513, 1024, 1025,
                 4095, 4096, 4097, 8192, 8193)
NAMED = len(NAMED_LENGTHS)
N_PATTERN = 8300        # users = items: the smallest square shape that holds a three-chunk row beside 64 untouched ids
FIRST_FREE = 64         # the long rows draw their columns from ids >= 64: the named rows of the other orientation hold no other entry
N_LONG = NAMED + 40
HEAVY = 4096
WCUT = 500              # als_split_wcut of the outlier cases, as test_als_gpu.py sets it
PATHS = {0: "none", 1: "pairs", 2: "wave", 3: "scratch", 4: "wide", 5: "fallback"}    # als_last_path (include/buffalo_hip.h)


def chunked_calls(n_rows):
    """[0, 14) [14, 14) [14, N_LONG) [N_LONG, 5000) [5000, N): an empty call, the long rows cut from the light ones."""
    return [(0, 14), (14, 14), (14, N_LONG), (N_LONG, 5000), (5000, n_rows)]


def K(**kw):
    """Options as a hashable key (for `references`)."""
    return tuple(sorted(kw.items()))


def opt(d, kw=()):
    return als_opt(d=d, alpha=4.0, reg_u=0.2, reg_i=0.3, num_iters=2, **dict({"compute_loss_on_training": True, "optimizer": "ialspp"}, **dict(kw)))


def vdim_of(d):
    return ((d + 31) // 32) * 32


class Case:
    """One rating matrix in both orientations (user-major `csr`, item-major `t`)."""
    def __init__(self, csr):
        self.csr, self.t = csr, csr.transpose()
        self.users, self.items = csr.num_users, csr.num_items

    def mat(self, axis):
        return self.csr if axis == 0 else self.t


def chunks_of_row(n):
    """Lengths of the work items of a row of n entries (als_core.hpp, work_list)."""
    if n <= HEAVY:
        return [n] if n else []
    nch = -(-n // HEAVY)
    per = (-(-n // nch) + 1) & ~1           # chunks of ceil(n / nch) entries, rounded up to even
    return [min(per, n - c0) for c0 in range(0, n, per)]


def work_items(m, a=0, b=None):
    """Work items of the call [a, b) on `m`: one per row with entries, the rows above 4,096 entries one per chunk."""
    n = lengths_of(m)[a:b]
    return int((n > 0).sum()) + sum(len(chunks_of_row(int(k))) - 1 for k in n[n > HEAVY])


def assert_second_tickets(case, cus, per_cu):
    """A whole-matrix call of either side must hold more work items than the launch has consumers: `per_cu` per CU of a `cus`-CU
    device (16 waves for the Gramian kernels, 4 pairs for als_pc_kernel, als_wide_blocks_per_cu for the wide kernel)."""
    for axis in (0, 1):
        n = work_items(case.mat(axis))
        assert n > per_cu * cus, "axis %d: %d work items do not outnumber %d consumers (%d CUs)" % (axis, n, per_cu * cus, cus)


@functools.lru_cache(maxsize=None)
def pattern():
    """U = I = 8,300.  User rows 0 .. 71 get the NAMED_LENGTHS, then 40 lengths of 1 .. 200, on items >= 64; item rows 0 .. 71 the same
    lengths on users >= 64; every user and every item from 64 on gets two more entries.  (Rows 64 .. 71, eight of the random-length
    rows, therefore hold their two extra entries on top; the named rows hold exactly their length.)  Only row 0 is empty, in either
    orientation.  Values 1 + Poisson(1).  About 91,000 entries, 8,303 work items per side."""
    rng = np.random.default_rng(29)
    N = N_PATTERN
    lengths = list(NAMED_LENGTHS) + [int(x) for x in rng.integers(1, 201, size=40)]
    ar, ac = _long_rows(rng, lengths, N, FIRST_FREE)                # user rows 0 .. 71
    bi, bu = _long_rows(rng, lengths, N, FIRST_FREE)                # item rows 0 .. 71
    M = N - FIRST_FREE                                              # 8236 = 4 x 29 x 71: 3 and 5 are units, both maps are bijections
    u = np.arange(FIRST_FREE, N)
    e1, e2 = FIRST_FREE + (3 * (u - FIRST_FREE) + 5) % M, FIRST_FREE + (5 * (u - FIRST_FREE) + 11) % M
    keep = e1 != e2
    rows, cols = np.concatenate([ar, bu, u, u[keep]]), np.concatenate([ac, bi, e1, e2[keep]])
    key = np.unique(rows.astype(np.int64) * N + cols)
    rows, cols = key // N, key % N
    case = Case(_csr(N, N, rows, cols, 1 + rng.poisson(1.0, size=rows.shape[0])))
    for m in (case.csr, case.t):
        n = lengths_of(m)
        assert tuple(n[:NAMED]) == NAMED_LENGTHS, n[:NAMED]
        assert tuple(n[NAMED:FIRST_FREE]) == tuple(lengths[NAMED:FIRST_FREE]) and (n[1:] > 0).all() and n[N_LONG:].max() <= 16, n[NAMED:N_LONG]
        assert work_items(m) == N - 1 + 1 + 1 + 2               # every row but row 0; 4097 and 8192 one more, 8193 two more
    return case


# (length of the named row, which of its entries, what happens to the value); the entry is the first of that stretch of the row
# whose value is at least 2 (a one-entry row's is set to 2): alpha v x 100 = 4 x 2 x 100 is past the cut of 500, 4 x 1 x 100 is not
PLANTED = ((1, (0, 1), "x100"), (16, (0, 16), "x100"), (64, (0, 64), "x100"), (65, (64, 65), "x100"), (4096, (0, 4096), "x100"),
           (8193, (2732, 5464), "x100"), (4097, (2050, 4097), "x100"), (17, (16, 17), "neg"), (4095, (0, 4095), "neg"))
N_DEF, N_DEF_ROWS = 18, 16


def deferred(m, alpha=4.0, wcut=WCUT):
    """als_defer_scan_kernel restated on the host -> (flagged work items, flagged whole rows) of a whole-matrix call."""
    beg = np.concatenate([[0], m.indptr[:-1]])
    n_def = n_rows = 0
    for r in np.unique(m.rows()[~((alpha * m.vals > 0) & (alpha * m.vals <= wcut))]):
        b, c0 = int(beg[r]), 0
        chunks = chunks_of_row(int(m.indptr[r]) - b)
        for c in chunks:
            w = alpha * m.vals[b + c0:b + c0 + c]
            if not ((w > 0) & (w <= wcut)).all():
                n_def += 1
                n_rows += len(chunks) == 1
            c0 += c
    return n_def, n_rows


@functools.lru_cache(maxsize=None)
def pattern_outliers():
    """`pattern` with weights outside the f16 path planted at the bounds (PLANTED), in the named user rows AND in the named item rows:
    x100 on one entry of the rows of 1, 16, 64, 65 (its second key chunk), 4096 and 8193 (its middle chunk) entries and on one entry of
    the second chunk alone of the 4,097-entry row; -0.05 on the last entry of the 17-entry row and one of the 4,095-entry row.  An entry
    planted in a named user row also sits in a light item row, and the other way round, so in EITHER orientation a whole-matrix call
    flags N_DEF = 18 work items (9 named + 9 light rows), N_DEF_ROWS = 16 of them whole rows (the chunks of the 4,097- and 8,193-entry
    rows keep their row's slot): 18 x 4 <= 8,303 work items, the call stays on the pairs."""
    base = pattern()
    vals = base.csr.vals.copy()
    beg = np.concatenate([[0], base.csr.indptr[:-1]])

    def plant(pos, how):
        if how == "neg":
            vals[pos] = -0.05
        else:
            vals[pos] = 100.0 * max(vals[pos], 2.0)

    used = [set(), set()]       # the light rows of the other orientation already hit: every planted entry flags a light row of its own

    def pick(m, r, lo, hi, seen):
        k, v = m.row(r)
        ok = [e for e in range(lo, hi) if int(k[e]) >= N_LONG and int(k[e]) not in seen]
        e = next((e for e in ok if v[e] >= 2), ok[0])
        seen.add(int(k[e]))
        return e, int(k[e])

    for n, (lo, hi), how in PLANTED:
        r = NAMED_LENGTHS.index(n)
        e, _ = pick(base.csr, r, lo, hi, used[0])                   # the named user row
        plant(int(beg[r]) + e, how)
        e, u = pick(base.t, r, lo, hi, used[1])                     # the named item row: its entry e is (user u, item r)
        pos = int(beg[u]) + int(np.searchsorted(base.csr.row(u)[0], r))
        assert base.csr.keys[pos] == r
        plant(pos, how)
    from buffalo_amd.synth import CSR
    case = Case(CSR(base.users, base.items, base.csr.indptr, base.csr.keys, vals))
    for m in (case.csr, case.t):
        assert deferred(m) == (N_DEF, N_DEF_ROWS), deferred(m)
        assert N_DEF * 4 <= work_items(m)
    return case


@functools.lru_cache(maxsize=None)
def tiny(seed):
    """The 320 x 280 shape of test_als_gpu.py at density 0.06: every row shorter than a wave."""
    return Case(tiny_csr(U=320, I=280, density=0.06, seed=seed, counts=True))


def case_of(name):
    if name == "pattern":
        return pattern()
    if name == "pattern_outliers":
        return pattern_outliers()
    return tiny({"tiny_a": 31, "tiny_b": 47}[name])


def start(case, d, seed=9):
    """The float32 start state (P, Q), [rows, d]: signed normal(scale 0.1) -- see the module docstring for why signed."""
    rng = np.random.default_rng(seed)
    return rng.normal(scale=0.1, size=(case.users, d)).astype(np.float32), rng.normal(scale=0.1, size=(case.items, d)).astype(np.float32)


def chunk(m, a, b):
    if b == a:
        return m.keys[:0], m.vals[:0]
    return H.chunk_arrays(m, a, b)


class Half:
    """One half-epoch: the solved factor [rows, d] (and the padding columns the backend holds beside it), (nume, deno), the backend's
    own Gramian [d, d] and, for the device, the plan read-back of every call."""
    def __init__(self, axis, X, pad, loss, ff, plans):
        self.axis, self.X, self.pad, self.loss, self.ff, self.plans = axis, X, pad, loss, ff, plans


def plan_of(obj):
    """Which kernel family the last partial_update of a CyALS ran, and on what (als_last_*: include/buffalo_hip.h)."""
    out = {k: obj.device_buffer("als_last_" + k)[1] for k in ("path", "split", "n_work", "n_heavy", "n_def", "n_def_rows")}
    out["path"] = PATHS[out["path"]]
    return out


def bind(obj, case, P, Q, hip):
    obj.initialize_model(P, Q)
    if hip:
        obj.set_placeholder(case.csr.indptr, case.t.indptr, case.csr.nnz + 1)


def half(obj, case, axis, state, d, hip, ranges=None):
    """Bind copies of the float32 `state` (re-binding the model as test_half_epochs_match_oracle does), run the half-epoch of `axis` in
    the calls of `ranges`, keys / vals handed over per call as the front does -> Half."""
    vdim = vdim_of(d) if hip else d
    P, Q = (H.pad(x.copy(), vdim) for x in state)
    bind(obj, case, P, Q, hip)
    m = case.mat(axis)
    obj.precompute(axis)
    ff = obj.device_tensor("FF", (vdim, vdim)).cpu().numpy()[:d, :d].copy() if hip else obj.get_ff(d)
    loss, plans = np.zeros(2), []
    for a, b in ranges or [(0, m.num_users)]:
        loss += obj.partial_update(a, b, m.indptr, *chunk(m, a, b), axis)
        if hip:
            plans.append(plan_of(obj))
    X, other = (P, Q) if axis == 0 else (Q, P)
    assert np.array_equal(other[:, :d], state[1 - axis])          # a half-epoch leaves the other side alone
    return Half(axis, X[:, :d].copy(), X[:, d:].copy(), tuple(loss), ff, plans)


def make_hip(d, kw=(), modes=None):
    from buffalo_amd.backend import CyALS
    obj = CyALS()
    path = H.write_opt(dict(opt(d, kw), accelerator=True))
    try:
        assert obj.init(path)
    finally:
        os.unlink(path)
    for k, v in (modes or {}).items():
        obj.set_mode(k, v)
    return obj


def run(make, case, d, kw=(), modes=None, ranges=None):
    """The two half-epochs of one backend, each from the same float32 state.  `make`: "hip" (CyALS, `modes` set after init) or a class
    with the oracle's surface.  `ranges`: row ranges per call, one list for both sides (a function of the row count) or None."""
    hip = make == "hip"
    if hip:
        obj = make_hip(d, kw, modes)
    else:
        obj, path = make(), H.write_opt(opt(d, kw))
        try:
            assert obj.init(path)
        finally:
            os.unlink(path)
    state = start(case, d)
    return [half(obj, case, axis, state, d, hip, ranges(case.mat(axis).num_users) if ranges else None) for axis in (0, 1)]


def f64_run(case, d, kw, ffs, **plant):
    """The float64 yardstick of both half-epochs from the Gramians `ffs` (one per side: each backend is held to the recurrence started
    from its OWN Gramian, whose rounding is checked apart -- test_precompute_gramian_mfma)."""
    P, Q = start(case, d)
    out = []
    for axis in (0, 1):
        X, Y = (P, Q) if axis == 0 else (Q, P)
        T, nume, deno = rn.als_half_epoch_f64_fast(X, Y, ffs[axis], case.mat(axis), opt(d, kw), axis, **plant)
        out.append(Half(axis, T, None, (nume, deno), ffs[axis], []))
    return out


@functools.lru_cache(maxsize=None)
def references(name, d, kw=()):
    """The oracle's and the yardstick's runs of one (case, d, options), computed once per process and shared by every design:
    ([oracle Half], [f64 Half from the oracle's Gramians])."""
    from oracle import oracle as orc
    orc.build()
    case = case_of(name)
    o = run(orc.OracleALS, case, d, kw)
    return o, f64_run(case, d, kw, [h.ff for h in o])


def hold(section, hip, orc, f64, f64_hip=None, named=0):
    """Both half-epochs of the device run inside the envelope of the oracle's: err(hip, f64 from the device's Gramian) <=
    2.5 x err(oracle, f64 from the oracle's Gramian) + 4 ulp (ref_eals.bound); the figures are recorded first.  `named`: print the per-row
    figures of the first `named` rows with their length, so that a failure names a row length."""
    lines, bad = [], []
    for h, o, f, fh in zip(hip, orc, f64, f64_hip or f64):
        eo, eh = relerr(o.X, f.X), relerr(h.X, fh.X)
        allowed = bound(eo)
        ln = "axis %d err(oracle, f64) %.3g err(hip, f64) %.3g ratio %.2f of bound %.3g: %.2f" % (h.axis, eo, eh, eh / max(eo, 1e-30), allowed, eh / allowed)
        lines.append(ln)
        if not eh <= allowed or not np.isfinite(h.X).all():
            bad.append(ln)
        if named:
            so, sh = np.abs(f.X).max(), np.abs(fh.X).max()
            per = ["%d: %.2g / %.2g" % (n, np.abs(o.X[i] - f.X[i]).max() / so, np.abs(h.X[i] - fh.X[i]).max() / sh) for i, n in enumerate(NAMED_LENGTHS[:named])]
            lines.append("  per row, entries: err(oracle) / err(hip)  " + "  ".join(per))
    record(section, lines)
    assert not bad, "\n".join(lines)
    return lines


def record(section, lines):
    """Print the measured figures of one case (pytest -s shows them); with BFH_ALS_PARITY_OUT=<file> they are appended to that file
    as well -- profiles/als_parity.txt is the output of such runs, so that a plain test run leaves the checkout clean."""
    text = "".join("%s | %s\n" % (section, ln) for ln in lines)
    print(text, end="")
    out = os.environ.get("BFH_ALS_PARITY_OUT")
    if out:
        with open(out, "a") as f:
            f.write(text)
