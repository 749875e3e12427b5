"""Planted score bits for the selection kernels of csrc/topk_kernels.hpp: case builders and the score-matrix form of the specification.

If query row P[q] is the unit vector e_c and Q[:, c] holds a float32 pattern s, then P[q] . Q[j] is s[j] BIT FOR BIT in any summation
order (1 * s plus exact zeros), on the matrix cores and in the oracle alike; with a bias, s[j] + Qb[j] is one fp32 addition on both
sides.  So any score bit pattern, tie layout and count of columns above a threshold can be put in front of every selection kernel
through the public calls, and every comparison is equality of keys and of score bits (`bits`).  No tolerance appears in this work.
(One thing the plant cannot carry: a -0.0.  Both sides start their sum at +0.0, and -0.0 + +0.0 = +0.0; the device also maps -0.0
to +0.0 before it forms the key -- `desc_key`: s += 0.0f -- so a zero is always LISTED as +0.0.  `spec_scores` does the same.)

Yardstick: `oracle.dot_topn` (held bit-identical to the compiled reference in test_oracle_vs_reference_sources.py) where the
FLT_MIN admission rule is on, and the closed form `spec_scores` -- `topk_cases.spec_dot_topn` taking the score matrix directly,
vectorised per row -- where it is off (`rule=False`: no oracle exists) and for the device's own tie order of `quickselect`
(score desc, index desc).  tests/test_topk_planted_cpu.py holds `spec_scores` to the oracle on every case the device file runs.

NaN: with the rule on a NaN is never admitted (`s > FLT_MIN` is false) and must not disturb its neighbours -- `specials`.  NaN with the
rule OFF is out of scope and nothing is asserted about it: reading the code, the dense path ranks a positive NaN first (its key is
below +inf's), while the fused filter compares `sc >= thr` against a NaN threshold and keeps nothing.

Which case straddles which bound of the kernels (test names: tests/test_topk_bounds_gpu.py)
--------------------------------------------------------------------------------------------
bound in the code                                             case (builder)                              test
second / third histogram level of the fast path               low_bits_fit: <= 1,000 keys share bits      test_low_key_bits_dense
  ((key >> 10) & 1023, key & 1023), cand_cap not exceeded       31..20, differ in 19..10 / 9..0 / both
passes 2-4 of the multi-pass path ((key >> shift) & 255)      low_bits_full (3,072 in one 12-bit bin),    test_low_key_bits_dense (fast_select 1: the bin
                                                                one_byte (four families, one byte each)     overflows; 0: multi-pass only)
levels 1 and 2 of wave_kth_key (bits 19..8, 7..0)             low_bits_full / one_byte padded to 6,176    test_low_key_bits_fused (wave routes)
candidate buffer, cand_cap = 1,024                            bin_1024: threshold bin holds 1,024 / 1,025 test_threshold_bin_at_the_candidate_buffer
256-column steps and 64-lane waves of the ordered tie walk    ties_at: F ends at column 63, 64, 255, 256, test_tie_walk_dense, test_tie_walk_fused
                                                                257, 511, 512; remaining = 1 and |A| - 1;
                                                                |A| over three steps; better after F
need_eq == eq_total (no straddle: fast path)                  ties_at row `exact`                         test_tie_walk_dense, test_tie_walk_fused (exchanges)
kSampleCap = 512 (sample segment)                             fused_rows `winners512` / `winners513`      test_fused_routes[c0_1024]
cap_seg = 512 (one swept segment)                             fused_rows `seg512` / `seg513`              test_fused_routes
kListCap = 2,048 (the row's list)                             fused_rows `list2048` / `list2049`          test_fused_routes
p2 = 1,024 / 2,048: wave_list switches off                    distinct_row, kk = 1,024 / 1,025            test_fused_wave_list_switch
p2 at 1,024 / 2,048 on the dense path, k = 1,024 ... 2,049    low_bits_full                               test_k_values_dense
TOPK_MAX_K = 16,384 run, not only refused                     distinct_row(16,400), two queries           test_largest_k
query counts around 32 and 128 (lanes of a wave's A operand,  score_case: nq = 1, 31, 32, 33, 127, 128,   test_score_kernel_query_counts
  four waves of a block, rows of a wave beyond nq)              129; fused: 1, 3, 4, 5, 129; a +inf score  test_fused_routes, test_specials_*[fused]
                                                                behind the sample with 3 queries (specials)
candidate counts around 32 (tile), 256 (select step)          tiny_cols: 1, 31, 32, 33, 255, 256, 257     test_candidate_counts
half-wave split of a K-chunk (W/2), second K-chunk's          score_case: planted column 0, W/2 - 1, W/2, test_score_kernel_columns
  `accumulate` read (column 128 upward)                         d - 1; 127, 128 and the second chunk's
                                                                split for d > 128
more than one tile per group, ragged last group               1,280 x 6,600, d = 128 (207 tiles on        test_score_kernel_many_tiles
                                                                2,048 = 8 x 256 CU slots: tpb = 2)
take_all, (-1, FLT_MIN) then (-1, 0.0) padding                few: fewer than kk, exactly kk, none;       test_few_admissible
                                                                k > q_rows, pool smaller than k
FLT_MIN itself, subnormals, +-0, FLT_MAX, +-inf, NaN          specials (d = 1)                            test_specials_rule_on / _rule_off
seen columns at the k-th / best place, at sample columns 0,   seen_case                                   test_seen_aware
  31, c0 - 1, at c0; runs of 64 / 65 seen keys in the sample;
  fewer than kk unseen columns (padding kernel)
"""
import os

import numpy as np

FMIN = np.finfo(np.float32).tiny
FMAX = np.finfo(np.float32).max
ONE = 0x3F800000            # bits of 1.0f: scores ONE | m, m < 2^20, share bits 31..20 of their key
WORSE = (0x3E800000, 0x3F000000)     # [0.25, 0.5): admissible, below everything planted around 1.0
GE = (0x3F900000, 0x40000000)        # [1.125, 2): above the 12-bit bin of 1.0
BETTER = (0x40000000, 0x40800000)    # [2, 4)


def f32(u):
    return np.ascontiguousarray(u, dtype=np.uint32).view(np.float32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def desc_key(s):
    """csrc/topk_kernels.hpp desc_key restated: smaller key <=> larger score, -0 and +0 coincide."""
    u = bits(np.asarray(s, np.float32) + np.float32(0.0))
    u = np.where(u >> 31, ~u, u | np.uint32(0x80000000))
    return ~u


def distinct(rng, n, rng_bits):
    """n distinct float32 values with bit patterns in [lo, hi), in random order."""
    lo, hi = rng_bits
    return f32(rng.choice(hi - lo, size=n, replace=False).astype(np.uint32) + np.uint32(lo))


# ------------------------------------------------------------------------------------------------
# the specification on a score matrix
# ------------------------------------------------------------------------------------------------
def spec_scores(S, k, rule=True, pool=None, exclude=None):
    """`topk_cases.spec_dot_topn` on the (biased) score matrix S [queries, columns] itself, one vectorised pass per row.
    rule: only scores > FLT_MIN are admissible (dot_topn); off: every score is (quickselect, the validation ranking).
    pool: the columns that may be listed (kk = min(k, columns, len(pool))); exclude [queries, columns]: per-row seen columns --
    row b then has kk_b = min(kk, allowed columns outside exclude[b]) slots, the rest read (-1, 0.0) (recommend_unseen).
    With t the kk-th largest admissible score: everything > t is kept; of the ties at t, F = the first kk candidates >= t by column,
    A = the ties inside F, and the survivors are the highest-index members of A.  Listed by (score desc, column desc), zeros as +0.0;
    unfilled slots (-1, FLT_MIN), slots beyond kk (-1, 0.0)."""
    S = np.asarray(S, dtype=np.float32)
    nq, cols = S.shape
    allowed = np.ones(cols, bool)
    kk = min(cols, k)
    if pool is not None and len(pool):
        allowed[:] = False
        allowed[np.asarray(pool)] = True
        kk = min(len(pool), kk)
    keys = np.full((nq, k), -1, np.int32)
    vals = np.zeros((nq, k), np.float32)
    for i in range(nq):
        adm = allowed.copy()
        kk_i = kk
        if exclude is not None:
            adm &= ~exclude[i]
            kk_i = min(kk, int(adm.sum()))
        with np.errstate(invalid="ignore"):
            s = S[i] + np.float32(0.0)
            adm &= (s > FMIN) if rule else ~np.isnan(s)
        cand = np.flatnonzero(adm)
        v = s[cand]
        keep = np.arange(len(cand))
        if len(cand) > kk_i:
            t = np.partition(v, len(v) - kk_i)[len(v) - kk_i]
            better = np.flatnonzero(v > t)
            first = np.flatnonzero(v >= t)[:kk_i]                 # F
            ties = first[v[first] == t]                           # A
            keep = np.concatenate([better, ties[len(ties) - (kk_i - len(better)):]])
        order = np.lexsort((-cand[keep], -v[keep]))
        n = len(keep)
        keys[i, :n] = cand[keep][order]
        vals[i, :n] = v[keep][order]
        vals[i, n:kk_i] = FMIN
    return keys, vals


def f_end(row, kk, rule=True):
    """Column at which F ends (the kk-th candidate >= t by column), |A|, and `remaining` = the slots left for ties; None without a
    straddling tie."""
    s = np.asarray(row, np.float32) + np.float32(0.0)
    adm = s > FMIN if rule else np.ones(len(s), bool)
    v = s[adm]
    if len(v) <= kk:
        return None
    t = np.partition(v, len(v) - kk)[len(v) - kk]
    ge = np.flatnonzero(adm & (s >= t))
    n_better, n_eq = int((v > t).sum()), int((v == t).sum())
    if kk - n_better == n_eq:
        return None
    F = ge[:kk]
    return int(F[-1]), int((s[F] == t).sum()), kk - n_better


# ------------------------------------------------------------------------------------------------
# planting
# ------------------------------------------------------------------------------------------------
def planted(score_rows, d, cols_at=None, queries=None):
    """(idx, P, Q): pattern i (row i of score_rows, all finite) is stored in factor column cols_at[i] of Q [columns, d]; query b is the
    unit vector of the column of pattern queries[b] (default: one query per pattern).  Every other entry is zero, so the score matrix
    of the call is score_rows[queries] bit for bit."""
    R = np.asarray(score_rows, dtype=np.float32)
    n_pat, cols = R.shape
    cols_at = np.arange(n_pat) if cols_at is None else np.asarray(cols_at)
    assert len(set(cols_at.tolist())) == n_pat and 0 <= cols_at.min() and cols_at.max() < d
    assert np.isfinite(R).all(), "non-finite plants need d = 1 (planted_d1): 0 * inf elsewhere would poison other queries"
    queries = np.arange(n_pat) if queries is None else np.asarray(queries)
    Q = np.zeros((cols, d), np.float32)
    Q[:, cols_at] = R.T
    P = np.zeros((len(queries), d), np.float32)
    P[np.arange(len(queries)), cols_at[queries]] = 1.0
    return np.arange(len(queries), dtype=np.int32), P, Q


def planted_d1(score_row, nq):
    """d = 1, every query [1.0]: the one score row may hold +-inf and NaN."""
    row = np.asarray(score_row, np.float32)
    return np.arange(nq, dtype=np.int32), np.ones((nq, 1), np.float32), np.ascontiguousarray(row[:, None])


# ------------------------------------------------------------------------------------------------
# 1. low_bits: the k-th place sits inside a bin of keys that share their top bits
# ------------------------------------------------------------------------------------------------
def _low_family(rng, n_a, n_b, n_c):
    a = (rng.choice(511, n_a, replace=False) + 1) << 10                        # differ only in bits 19..10 (m < 2^19: inside [1, 1.0625))
    b = rng.choice(1023, n_b, replace=False) + 1                               # only in bits 9..0
    c = ((rng.choice(511, n_c) + 1) << 10) | (rng.choice(1023, n_c) + 1)       # in both
    m = np.unique(np.concatenate([a, b, c]))
    return f32(m.astype(np.uint32) | np.uint32(ONE))


def low_bits_full(seed=1):
    """3,072 distinct scores inside [1.0, 1.0625), one 12-bit bin: the fast path's buffer overflows, passes 2-4 of the multi-pass path and
    levels 1 / 2 of wave_kth_key decide.  One row, shuffled."""
    rng = np.random.default_rng(seed)
    v = rng.permutation(_low_family(rng, 500, 1000, 4000))[:3072]
    assert len(v) == 3072 and len(np.unique(desc_key(v) >> 20)) == 1 and len(np.unique(desc_key(v) & 0xFFFFF)) == 3072
    assert len(np.unique((desc_key(v) >> 10) & 1023)) > 400 and len(np.unique(desc_key(v) & 1023)) > 800       # both digits vary
    return rng.permutation(v)[None, :]


def low_bits_fit(seed=2):
    """Rows of 3,000 distinct scores whose k-th place (k = 100) lies in a 12-bit bin of <= 1,000 keys: 60 better ones, then
    a) 900 that differ only in bits 19..10 [511 exist: 500], b) only in bits 9..0, c) in both, d) all three mixed; the rest worse.
    The candidate buffer holds the bin, so the second and third histogram level of the fast path decide."""
    rng = np.random.default_rng(seed)
    fams = [_low_family(rng, 500, 0, 0), _low_family(rng, 0, 900, 0), rng.permutation(_low_family(rng, 0, 0, 1200))[:900],
            rng.permutation(_low_family(rng, 200, 300, 500))[:900]]
    rows = []
    for fam in fams:
        row = np.concatenate([distinct(rng, 60, BETTER), fam, distinct(rng, 3000 - 60 - len(fam), WORSE)])
        key = desc_key(row)
        in_bin = (key >> 20) == (desc_key(np.float32(1.0)) >> 20)
        assert 100 < in_bin.sum() <= 1000 and in_bin.sum() == len(fam) and len(np.unique(row)) == 3000
        assert ((key >> 20) < (key[in_bin][0] >> 20)).sum() == 60                # the 100th best is the 40th of the bin
        rows.append(rng.permutation(row))
    return np.stack(rows)


def one_byte(seed=3):
    """Four rows of 1,000 scores for the four 8-bit passes: row p holds 255 scores that differ in byte p of their bits alone (the k-th
    place, k = 100, among them), 50 better and 695 worse ones where the family leaves room (byte 3 spans every exponent: no others)."""
    rng = np.random.default_rng(seed)
    b = (np.arange(255, dtype=np.uint32) + 1)
    fams = [f32(np.uint32(ONE) | b), f32(np.uint32(ONE) | (b << 8)), f32(np.uint32(0x3F000000) | (b[:127] << 16)),
            f32(np.uint32(0x00800000) | (b[:126] << 24))]
    rows = []
    for p, fam in enumerate(fams):
        x = bits(fam)
        assert len(np.unique(x)) == len(fam) and np.all((x ^ x[0]) & ~np.uint32(0xFF << (8 * p)) == 0)
        n_better = 50 if p < 2 else 0
        if p < 3:
            row = np.concatenate([distinct(rng, n_better, BETTER), fam, distinct(rng, 1000 - n_better - len(fam), (0x3E000000, 0x3E800000))])
        else:
            row = np.concatenate([fam, -fam, np.zeros(1000 - 2 * len(fam), np.float32)])
        assert (row > FMIN).sum() > 100 and np.sort(row)[::-1][99] in fam
        rows.append(rng.permutation(row))
    return np.stack(rows)


def distinct_row(cols, seed=4, nq=1):
    """nq rows of `cols` distinct scores inside one 12-bit bin (cols <= 2^20), each its own permutation."""
    rng = np.random.default_rng(seed)
    v = f32(rng.choice(1 << 20, cols, replace=False).astype(np.uint32) | np.uint32(ONE))
    return np.stack([rng.permutation(v) for _ in range(nq)])


# ------------------------------------------------------------------------------------------------
# 2. bin_1024: the threshold bin of the 12-bit level at the candidate buffer's size
# ------------------------------------------------------------------------------------------------
def bin_1024(n_in_bin, seed=5):
    """One row of 1,700 + columns: 50 better scores, n_in_bin distinct ones in the 12-bit bin of 1.0, the rest worse; k = 60 puts the
    k-th place 10 deep into the bin.  1,024: the last row the candidate buffer holds; 1,025: the first that falls to the multi-pass path.
    (The tests also ask for all but the last member of the bin: whichever candidate a too-small buffer loses, the list is then wrong.)"""
    rng = np.random.default_rng(seed)
    inb = f32(rng.choice(1 << 20, n_in_bin, replace=False).astype(np.uint32) | np.uint32(ONE))
    row = rng.permutation(np.concatenate([distinct(rng, 50, BETTER), inb, distinct(rng, 650, WORSE)]))
    key = desc_key(row)
    thr_bin = np.sort(key)[59] >> 20
    assert ((key >> 20) == thr_bin).sum() == n_in_bin and ((key >> 20) < thr_bin).sum() == 50
    return row[None, :]


# ------------------------------------------------------------------------------------------------
# 3. ties_at: ties that straddle the k-th place, F ending at chosen columns
# ------------------------------------------------------------------------------------------------
def tie_row(cols, kk, end, n_better_in, n_better_after, n_ties_after, rng, stride=1, t=1.0, ties_before=True):
    """F = the kk columns end, end - stride, ... (the kk-th candidate >= t arrives at column `end`): n_better_in of them better than t,
    the others the ties A; behind F n_better_after better scores (each evicts the oldest tie) and n_ties_after more ties (never
    admitted).  Everything else is worse."""
    F = end - stride * np.arange(kk)[::-1]
    assert F[0] >= 0 and end + 1 + n_better_after + n_ties_after <= cols
    row = distinct(rng, cols, WORSE)
    row[F] = t
    which_better = rng.choice(kk - 1, n_better_in, replace=False) if ties_before else np.arange(n_better_in)
    row[F[which_better]] = distinct(rng, n_better_in, BETTER)
    behind = end + 1 + rng.choice(cols - end - 1, n_better_after + n_ties_after, replace=False)
    row[behind[:n_better_after]] = distinct(rng, n_better_after, BETTER)
    row[behind[n_better_after:]] = t
    return row


def ties_at(seed=6):
    """kk = 10 on 700 columns.  Rows (name, F end, |A|, remaining), each premise asserted: F ends at column 63, 64, 255, 256, 257, 511,
    512 with ties behind F and one better score behind F; remaining = 1 (|A| - 1 better scores behind F) and = |A| - 1; and `exact`:
    need_eq == eq_total, no straddle."""
    rng = np.random.default_rng(seed)
    rows, names = [], []
    for end in (63, 64, 255, 256, 257, 511, 512):
        rows.append(tie_row(700, 10, end, 4, 1, 3, rng))                       # |A| = 6, remaining = 5 = |A| - 1
        names.append(("end%d" % end, end, 6, 5))
    rows.append(tie_row(700, 10, 300, 4, 5, 2, rng))                            # remaining = 1
    names.append(("remaining1", 300, 6, 1))
    rows.append(tie_row(700, 10, 9, 0, 3, 7, rng))                              # F = the first ten columns, all ties
    names.append(("first_ten", 9, 10, 7))
    rows.append(tie_row(700, 10, 699, 3, 0, 0, rng, stride=70))                 # ten candidates >= t, one every 70 columns up to the last ...
    rows[-1][5] = 1.0                                                           # ... and one more tie in front: F starts there, column 699's tie stays out
    names.append(("last_col", 629, 7, 7))                                       # every member of A survives, the eighth tie does not
    exact = tie_row(700, 10, 400, 4, 0, 0, rng)                                 # 4 better + 6 ties = kk: nothing straddles
    rows.append(exact)
    S = np.stack(rows)
    for r, (name, end, n_a, rem) in enumerate(names):
        assert f_end(S[r], 10) == (end, n_a, rem), (name, f_end(S[r], 10))
    assert f_end(exact, 10) is None
    return S, [n[0] for n in names] + ["exact"]


def ties_wide(seed=7):
    """kk = 600 on 1,500 columns: A spans more than one 256-column step.  Row 0: F = every other column up to 1,199, |A| = 590, 20 better
    scores behind F (remaining = 570); row 1: F = columns 0 .. 599, all ties but 100, |A| = 500, remaining = 1."""
    rng = np.random.default_rng(seed)
    S = np.stack([tie_row(1500, 600, 1199, 10, 20, 40, rng, stride=2), tie_row(1500, 600, 599, 100, 499, 30, rng)])
    assert f_end(S[0], 600) == (1199, 590, 570) and f_end(S[1], 600) == (599, 500, 1)
    return S


# ------------------------------------------------------------------------------------------------
# 4. specials (d = 1)
# ------------------------------------------------------------------------------------------------
def specials(nan, seed=8):
    """One row: +0.0 and -0.0 mixed, subnormals of both signs, FLT_MIN, nextafter(FLT_MIN, 1), FLT_MAX, -FLT_MAX, +-inf, ordinary scores
    of both signs [, NaNs of both signs and payloads], shuffled.  One +inf lies behind the 32 sampled columns of the fused path: with three
    queries the 29 unused rows of the wave see that score too and must keep nothing (they once did: a write behind the candidate buffer)."""
    rng = np.random.default_rng(seed)
    sub = f32(np.array([1, 2, 0x7FFFFF, 0x400000, 0x80000001, 0x807FFFFF], np.uint32))
    v = [np.array([0.0, -0.0, 0.0, -0.0, 0.0, -0.0], np.float32), sub, np.array([FMIN, -FMIN, np.nextafter(np.float32(FMIN), np.float32(1.0)),
         FMAX, -FMAX, np.inf, -np.inf, np.inf], np.float32), distinct(rng, 12, WORSE), -distinct(rng, 12, WORSE), distinct(rng, 3, BETTER)]
    if nan:
        v.append(f32(np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF], np.uint32)))
    row = np.concatenate(v)
    row = rng.permutation(row)
    assert (row[32:] == np.inf).any()
    return row


# ------------------------------------------------------------------------------------------------
# 5. few: fewer admissible columns than slots
# ------------------------------------------------------------------------------------------------
def few(seed=9):
    """40 columns, rows: 0 admissible, 1, 6, exactly 7 (= the k the test also runs), 39, all 40; the inadmissible ones are zeros,
    negatives, FLT_MIN itself and subnormals."""
    rng = np.random.default_rng(seed)
    bad = np.concatenate([np.zeros(10, np.float32), -distinct(rng, 20, WORSE), np.full(5, FMIN, np.float32), f32(np.arange(1, 6, dtype=np.uint32))])
    rows = []
    for n in (0, 1, 6, 7, 39, 40):
        row = rng.permutation(bad).copy()
        row[rng.choice(40, n, replace=False)] = distinct(rng, n, WORSE)
        assert (row > FMIN).sum() == n
        rows.append(row)
    return np.stack(rows)


# ------------------------------------------------------------------------------------------------
# the fused path: 6,176 candidates, d = 128, at most 129 queries
# ------------------------------------------------------------------------------------------------
FUSED_COLS = 6176
# route -> (fused_c0, wave_select)
ROUTES = {"rule": (0, 1), "c0_32": (32, 1), "c0_1024": (1024, 1), "c0_4128": (4128, 1), "block": (0, 0)}
K_LIST_CAP, K_SAMPLE_CAP = 2048, 512


def fused_layout(route, kk=10, q_rows=FUSED_COLS, nq=129, num_cus=256):
    """csrc/topk.hip fused_plan restated for a forced call: (c0, sample_seg, segments [(first column, end)], cap_seg).
    6,176 candidates = 193 tiles.  c0 = the forced sample, or by rule 32 doubled up to kk * q_rows / 682 (kk = 10: 128).  A sample of at
    most 4,096 columns on a wave route is its own segment and the sweep starts behind it; else the sweep covers all 193 tiles.  With at
    most two query blocks, 193 * 2 tile-blocks never fill 8 slots on each of >= 49 CUs, so tiles per group come from "at most 8 segments":
    tpb = ceil(sweep_tiles / 8) -- c0 = 32: 192 swept tiles -> 8 segments of 24 tiles = 768 columns, whatever the CU count; c0 = 128:
    189 -> 24 tiles; c0 = 1,024: 161 -> 21 tiles = 672 columns; all 193 -> 25 tiles = 800 columns -- and always 8 segments, so
    cap_seg = min(32 tpb, max(64, 4,096 / 8)) = 512."""
    c0_mode, wave = ROUTES[route]
    n_tiles = (q_rows + 31) // 32
    need = (kk * q_rows + K_LIST_CAP // 3 - 1) // (K_LIST_CAP // 3)
    c0 = 32
    while c0 < need:
        c0 <<= 1
    if c0_mode:
        c0 = c0_mode
    c0 = min((c0 + 31) // 32 * 32, n_tiles * 32, q_rows)
    sample_seg = bool(wave) and c0 <= 4096
    c0_tiles = (c0 + 31) // 32
    sweep_tiles = n_tiles - (c0_tiles if sample_seg else 0)
    qblocks = (nq + 127) // 128
    tpb = max(1, (sweep_tiles * qblocks + num_cus * 8 - 1) // (num_cus * 8), (sweep_tiles + 7) // 8)
    n_seg = max(1, (sweep_tiles + tpb - 1) // tpb)
    cap_seg = min(tpb * 32, max(64, 2 * K_LIST_CAP // n_seg))
    first = c0_tiles * 32 if sample_seg else 0
    segs = [(first + g * tpb * 32, min(first + (g + 1) * tpb * 32, q_rows)) for g in range(n_seg)]
    return c0, sample_seg, segs, cap_seg


def fused_predict(row, route, kk=10):
    """What the fused path does with one planted row (rule on, no pool): (overflow -> the dense redo, straddle -> the block-level list
    selection).  thr = the kk-th best admissible score of the sample, or FLT_MIN; a swept column is kept where score >= thr; the sample
    segment holds the admissible sampled columns >= thr."""
    c0, sample_seg, segs, cap_seg = fused_layout(route, kk)
    s = np.asarray(row, np.float32) + np.float32(0.0)
    adm0 = np.sort(s[:c0][s[:c0] > FMIN])[::-1]
    thr = adm0[kk - 1] if len(adm0) >= kk else np.float32(FMIN)
    counts = [int((s[a:b] >= thr).sum()) for a, b in segs]
    n0 = int(((s[:c0] > FMIN) & (s[:c0] >= thr)).sum()) if sample_seg else 0
    overflow = max(counts) > cap_seg or n0 > K_SAMPLE_CAP or sum(counts) + n0 > K_LIST_CAP
    return bool(overflow), f_end(s, kk) is not None, counts, n0


def fused_rows(route, seed=10):
    """The planted rows of one route (k = 10), as (names, S, overflow flags, straddle flags); thresholds t = 1.0:
    seg512 / seg513      the sample's ten best are 9 better scores and t; the first >= 513-column segment behind the sample holds exactly
                         512 / 513 scores in (t, 2)
    list2048 / list2049  the same sample; 2,038 / 2,039 scores in (t, 2) behind it, at most 500 per segment -- where the segments behind
                         the sample cannot hold them (c0 = 4,128) the rest are ties at t INSIDE the sample (they reach the list, not the
                         result: the final k-th place lies above t)
    winners512 / 513     c0 = 1,024 only: 9 better + 503 / 504 ties at t in the sample, nothing >= t behind it
    straddle             9 better and 3 ties in the sample, 4 more ties and nothing better behind it
    straddle_evict       5 better and 5 ties in the sample (F), 3 better behind it: the three oldest ties leave
    short                3 admissible sampled columns (thr = FLT_MIN), 40 admissible behind, everything else <= 0
    nothing              nothing admissible"""
    rng = np.random.default_rng(seed)
    c0, sample_seg, segs, cap_seg = fused_layout(route)
    assert cap_seg == 512 and len(segs) == 8
    t = np.float32(1.0)
    fixed = np.unique([0, 31, c0 - 1])
    in_sample = np.sort(np.concatenate([fixed, rng.choice(np.setdiff1d(np.arange(c0), fixed), 10 - len(fixed), replace=False)]))
    behind = [(max(a, c0), b) for a, b in segs if b > max(a, c0)]
    names, rows, over, strad = [], [], [], []

    def base():
        row = distinct(rng, FUSED_COLS, WORSE)
        row[in_sample] = np.concatenate([distinct(rng, 9, BETTER), [t]])
        return row

    def add(name, row, o, s):
        names.append(name), rows.append(row), over.append(o), strad.append(s)

    a, b = next((a, b) for a, b in segs if a >= c0 and b - a >= 513)      # wholly behind the sample
    for n in (512, 513):
        row = base()
        row[a + rng.choice(b - a, n, replace=False)] = distinct(rng, n, GE)
        add("seg%d" % n, row, n > 512, False)
    for n in (2048, 2049):
        row = base()
        left = n - 10
        for a2, b2 in behind:
            m = min(500 if a2 > c0 or sample_seg else 350, left, b2 - a2)      # (a segment the sample reaches into also holds sampled ties)
            row[a2 + rng.choice(b2 - a2, m, replace=False)] = distinct(rng, m, GE)
            left -= m
        if left:
            free = np.setdiff1d(np.arange(c0), in_sample)
            row[free[np.linspace(0, len(free) - 1, left).astype(int)]] = t
        add("list%d" % n, row, n > 2048, False)
    if route == "c0_1024":
        for n in (512, 513):
            row = base()
            free = np.setdiff1d(np.arange(c0), in_sample)
            row[rng.choice(free, n - 10, replace=False)] = t
            add("winners%d" % n, row, n > 512, True)
    row = base()
    free = np.setdiff1d(np.arange(c0), in_sample)
    row[rng.choice(free, 2, replace=False)] = t
    row[[s[0] + 5 for s in behind[:4]]] = t
    add("straddle", row, False, True)
    row = distinct(rng, FUSED_COLS, WORSE)
    row[in_sample] = np.concatenate([distinct(rng, 5, BETTER), np.full(5, t)])
    row[[s[0] + 7 for s in behind[-3:]]] = distinct(rng, 3, BETTER)
    add("straddle_evict", row, False, True)
    row = -distinct(rng, FUSED_COLS, WORSE)
    row[::3] = 0.0
    row[in_sample[:3]] = distinct(rng, 3, WORSE)
    row[c0 + rng.choice(FUSED_COLS - c0, 40, replace=False)] = distinct(rng, 40, GE)
    add("short", row, False, False)
    row = -distinct(rng, FUSED_COLS, WORSE)
    row[::3] = 0.0
    add("nothing", row, False, False)
    S = np.stack(rows)
    for r, name in enumerate(names):      # the premise of every row, from the restated plan
        o, s, counts, n0 = fused_predict(S[r], route)
        assert (o, s) == (over[r], strad[r]), (route, name, o, s, counts, n0)
        if name in ("seg512", "seg513"):
            assert max(counts) == int(name[3:])
        if name in ("list2048", "list2049"):
            assert sum(counts) + n0 == int(name[4:]) and max(counts) <= 512 and n0 <= 512
        if name in ("winners512", "winners513"):
            assert n0 == int(name[7:]) and sum(counts) == 0
    return names, S, np.array(over), np.array(strad)


def seen_case(seed=11):
    """recommend_unseen on 6,176 planted columns, k = 10: (S, M) with M [rows, columns] the seen matrix.  Every row has 30 scores in
    [2, 4) (`top`, among them columns 0, 31, 32, 127, 128, 1023, 1024, 4127: the last sampled and first swept column of every route) over
    distinct worse ones.  Rows: none seen; the best column; the k-th best; the ten best; the sample-edge columns; columns 0 .. 63;
    0 .. 64; a tie at the k-th place whose surviving member is seen; everything but 4 columns; everything."""
    rng = np.random.default_rng(seed)
    edge = np.array([0, 31, 32, 127, 128, 1023, 1024, 4127])
    rows, seen = [], []
    for r in range(10):
        top = np.concatenate([edge, rng.choice(np.setdiff1d(np.arange(FUSED_COLS), edge), 22, replace=False)])
        row = distinct(rng, FUSED_COLS, WORSE)
        row[top] = distinct(rng, 30, BETTER)
        order = top[np.argsort(-row[top])]
        m = np.zeros(FUSED_COLS, bool)
        if r == 1:
            m[order[0]] = True
        elif r == 2:
            m[order[9]] = True
        elif r == 3:
            m[order[:10]] = True
        elif r == 4:
            m[edge] = True
        elif r == 5:
            m[:64] = True
        elif r == 6:
            m[:65] = True
        elif r == 7:
            row[order[9:14]] = row[order[9]]              # five ties at the k-th place ...
            m[spec_scores(row[None, :], 10)[0][0, 9]] = True    # ... the one of them that would be listed is seen
        elif r == 8:
            m[:] = True
            m[[order[0], order[20], 5000, 6175]] = False
        elif r == 9:
            m[:] = True
        rows.append(row), seen.append(m)
    return np.stack(rows), np.stack(seen)


def csr_of_seen(M):
    """END-offset CSR (set_seen) of the boolean matrix M."""
    indptr = np.cumsum(M.sum(axis=1), dtype=np.int64)
    keys = np.nonzero(M)[1].astype(np.int32)
    return indptr, np.ascontiguousarray(keys)


# ------------------------------------------------------------------------------------------------
# the score kernel: which factor column carries the plant
# ------------------------------------------------------------------------------------------------
def plant_columns(d):
    """Factor columns that prove the score kernel's K-chunk handling at width d: 0, W/2 - 1, W/2 (the half-wave split of the first
    chunk, W = min(128, ceil8(d))), d - 1, and for d > 128 columns 127, 128 (the second chunk's `accumulate` read) and that chunk's split."""
    d_pad = (d + 7) // 8 * 8
    W = min(128, d_pad)
    want = [0, W // 2 - 1, W // 2, d - 1]
    if d > 128:
        W1 = d_pad - 128
        want += [127, 128, 128 + W1 // 2 - 1, 128 + W1 // 2]
    return sorted(set(c for c in want if 0 <= c < d))


def score_case(d, nq, cols=300, seed=12):
    """(S, idx, P, Q): every entry of Q [cols, d] is a planted score (distinct bit patterns in [0.5, 2));
    query b is the unit vector of factor column col_of[b] -- the columns of `plant_columns` first, then the others in turn -- so S[b] is
    Q[:, col_of[b]].  The queries are asked for in descending order of their row in P."""
    rng = np.random.default_rng(seed + d)
    Q = distinct(rng, cols * d, (0x3F000000, 0x40000000)).reshape(cols, d)
    first = plant_columns(d)
    col_of = np.array((first + [c for c in range(d) if c not in first]) * (nq // d + 1))[:nq]
    P = np.zeros((nq, d), np.float32)
    P[np.arange(nq), col_of] = 1.0
    idx = np.arange(nq, dtype=np.int32)[::-1].copy()
    return np.ascontiguousarray(Q[:, col_of[idx]].T), idx, P, Q


def record(section, lines):
    """Print the figures of one case (pytest -s shows them); with BFH_TOPK_PARITY_OUT=<file> they are appended to that file as well --
    profiles/topk_parity.txt is the output of such runs, so that a plain test run leaves the checkout clean."""
    text = "".join("%s | %s\n" % (section, ln) for ln in lines)
    print(text, end="")
    out = os.environ.get("BFH_TOPK_PARITY_OUT")
    if out:
        with open(out, "a") as f:
            f.write(text)


# ------------------------------------------------------------------------------------------------
# what the dense-selection tests run (CPU: spec == oracle; device: device == oracle)
# ------------------------------------------------------------------------------------------------
def tiny_cols(cols, seed=13):
    """Five rows of `cols` candidates: three of distinct scores, one with every score equal (ties at every place), one with none admissible."""
    rng = np.random.default_rng(seed + cols)
    rows = [distinct(rng, cols, (0x3F000000, 0x40000000)) for _ in range(3)]
    return np.stack(rows + [np.full(cols, 1.5, np.float32), -rows[0]])


def dense_cases():
    """(name, S, ks) of every finite planted score matrix the dense-selection tests run."""
    return [("low_bits_full", low_bits_full(), (1, 2, 3, 100, 1024, 1025, 2048, 2049, 3072, 3077)),
            ("low_bits_fit", low_bits_fit(), (100,)),
            ("one_byte", one_byte(), (100,)),
            ("bin_1024", bin_1024(1024), (60, 51, 1073, 1074)),         # 10 deep into the bin, its first member, all but its last, all
            ("bin_1025", bin_1024(1025), (60, 51, 1074, 1075)),
            ("ties_at", ties_at()[0], (10,)),
            ("ties_wide", ties_wide(), (600,)),
            ("few", few(), (7, 40, 45))]


def some_bias(cols, seed=14):
    """A bias column of small integers / 8: s + Qb is one fp32 addition on every side, and it moves scores across the planted bins."""
    return (np.random.default_rng(seed).integers(-4, 5, size=(cols, 1)) / 8.0).astype(np.float32)


def low_bits_fused(seed=15):
    """6,176 columns for the wave kernels' wave_kth_key (levels over key bits 31..20, 19..8, 7..0): row 0 all distinct inside one 12-bit
    bin, rows 1-4 the `one_byte` rows with worse columns appended (row 4, the byte-3 family: zeros)."""
    rng = np.random.default_rng(seed)
    ob = one_byte()
    rows = [distinct_row(FUSED_COLS, seed)[0]]
    for p in range(4):
        pad = distinct(rng, FUSED_COLS - ob.shape[1], (0x3D000000, 0x3E000000)) if p < 3 else np.zeros(FUSED_COLS - ob.shape[1], np.float32)
        rows.append(rng.permutation(np.concatenate([ob[p], pad])))
    return np.stack(rows)


def ties_fused(route):
    """The `ties_at` rows for the list-mode tie walk: the 700 columns are spread behind the sample, one every `stride` columns, and nothing
    else is admissible -- the sample bounds nothing (thr = FLT_MIN), every admissible column reaches the list, and the list sorted by
    column IS the ties_at row: F ends at list position 63, 64, 255, 256, 257, 511, 512."""
    S, names = ties_at()
    c0 = fused_layout(route)[0]
    stride = min(7, (FUSED_COLS - c0 - 1) // 700)
    out = -np.abs(distinct(np.random.default_rng(16), len(S) * FUSED_COLS, WORSE)).reshape(len(S), FUSED_COLS)
    out[:, c0 + stride * np.arange(700)] = S
    return out, names
