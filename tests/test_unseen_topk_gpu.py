"""`recommend_unseen` (bfh_topk_set_seen / bfh_topk_recommend_unseen[_device], buffalo_amd.parallel): the k best items a user has not
seen, excluded inside the selection on the dense and on the fused path.  Every comparison is exact (keys and score bits):

* the fused path's seen-aware steps against the dense step, for every route of the fused path;
* against `dot_topn` of the single user with pool = the complement of the seen row (the documented meaning of a row);
* against the CPU specification `topk_cases.spec_dot_topn` on integer factors (exact arithmetic);
* the device form against the host form; d = 200 (dense inside); the refusals."""
import functools

import numpy as np
import pytest

import eval_cases as ec
import helpers as H
import topk_cases as tc

pytestmark = pytest.mark.gpu

U, I = 300, 6000
FMIN = np.finfo(np.float32).tiny
# planted users (rows of the training matrix)
NONE, ONE, S2047, S2048, S2049, BUT3, ALL, FAN, HALVES, CONST = range(10)
PLANTED = list(range(10))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def common_input(d):
    """6,000 items x 300 users, float factors with exact duplicate rows (Q[1000:1400] = Q[2000:2400]) and a constant block
    (Q[3000:3300]); a ~3 % random training matrix with the planted rows; queries: a shuffled subset of the users with repeats."""
    rng = np.random.default_rng(1000 + d)
    Q = rng.normal(scale=0.3, size=(I, d)).astype(np.float32)
    Q[1000:1400] = Q[2000:2400]
    Q[3000:3300] = Q[3000]
    P = rng.normal(scale=0.3, size=(U, d)).astype(np.float32)
    M = rng.random((U, I)) < 0.03
    M[NONE] = False
    M[ONE] = False
    M[ONE, 4321] = True
    for u, n in ((S2047, 2047), (S2048, 2048), (S2049, 2049)):     # the LDS staging boundary of the training row
        M[u] = False
        M[u, rng.choice(I, size=n, replace=False)] = True
    M[BUT3] = True
    M[BUT3, [17, 3100, 5999]] = False
    M[ALL] = True
    M[FAN] = False
    fan_items = rng.choice(I, size=400, replace=False)
    M[FAN, fan_items] = True
    P[FAN] = Q[fan_items].mean(axis=0) * 8.0                        # its best-scoring items are the seen ones: lists fill with them
    M[HALVES, 1000:1400] = False
    M[HALVES, 2000:2400] = False
    M[HALVES, 3000:3300] = False
    M[HALVES, 1000:1200] = True                                     # of every duplicated pair exactly one column is seen
    M[HALVES, 2200:2400] = True
    M[HALVES, 3000:3300:2] = True                                   # every other column of the constant block
    P[HALVES] = 2.0 * Q[3000] + 0.5 * Q[2100] + 0.5 * Q[2300]
    P[CONST] = 4.0 * Q[3000]                                        # the constant block is this user's best score: ties at the k-th place
    rows, cols = np.nonzero(M)
    train = ec.csr_of(U, I, rows, cols)
    users = np.concatenate([PLANTED, rng.choice(np.arange(10, U), size=260, replace=False), PLANTED[2:9], rng.integers(0, U, size=50)])
    users = np.ascontiguousarray(rng.permutation(users), dtype=np.int32)
    assert not np.array_equal(users, np.arange(len(users)))
    Qb = rng.normal(scale=0.1, size=(I, 1)).astype(np.float32)
    pool = np.ascontiguousarray(rng.permutation(I)[:700], dtype=np.int32)
    return train, M, P, Q, Qb, pool, users


def _engine(train, fused, c0=0, wave=1, flt=1):
    from buffalo_amd import parallel as par
    eng = par.TopK()
    eng.set_mode("fused", fused)
    eng.set_mode("fused_c0", c0)
    eng.set_mode("wave_select", wave)
    eng.set_mode("flt_min_rule", flt)
    if train is not None:
        eng.set_seen(train.indptr, train.keys, train.num_items)
    return eng


def _recommend(eng, users, P, Q, Qb, pool, k):
    keys = np.full((len(users), k), 12345, dtype=np.int32)
    scores = np.full((len(users), k), 9.75, dtype=np.float32)
    eng.recommend_unseen(users, P, Q, Qb, keys, scores, pool, k)
    return keys, scores


PATHS = (("dense", 0, 0, 1), ("fused", 1, 0, 1), ("fused32", 1, 32, 1), ("fused1024", 1, 1024, 1), ("fused4128", 1, 4128, 1),
         ("fused_block", 1, 0, 0))
CASES = [(k, bias, pooled, flt) for k in (10, 100, 1500) for bias in (False, True) for pooled in (False, True) for flt in (1, 0)]


@pytest.mark.parametrize("d", [96, 128])
@pytest.mark.parametrize("k,bias,pooled,flt", CASES)
def test_fused_path_is_bit_identical_to_dense_seen_aware(d, k, bias, pooled, flt):
    """d = 96: the guarded-chunk FILTER instance of the sweep, d = 128: the FULL one.  Routes: the rule's sample, one sampled tile
    (loose thresholds: overflowing lists, the dense redo with each row's own user), 1,024 columns, 4,128 columns (no sample segment:
    block-level thresholds with the seen-aware dense selection, then the wave list kernel), and wave_select = 0 (list-mode
    topk_select_kernel with the staged seen keys behind the list)."""
    train, M, P, Q, Qb, pool, users = common_input(d)
    qb = Qb if bias else tc.NO_BIAS
    pl = pool if pooled else tc.EMPTY_POOL
    out, redo = {}, {}
    for name, fused, c0, wave in PATHS:
        eng = _engine(train, fused, c0, wave, flt)
        out[name] = _recommend(eng, users, P, Q, qb, pl, k)
        redo[name] = eng.stats()["merges"]
    print("rows handed back to the dense path of %d: %s" % (len(users), redo))
    assert redo["dense"] == 0
    for name in [p[0] for p in PATHS[1:]]:
        assert np.array_equal(out[name][0], out["dense"][0]), name
        assert np.array_equal(_bits(out[name][1]), _bits(out["dense"][1])), name
    if not pooled:                                     # (a 700-item pool fits every list whatever the threshold, as in test_topk_gpu.py)
        assert redo["fused32"] > 0                     # a one-tile sample overflows lists: the dense redo path ran
        if k <= 100:
            assert redo["fused"] < len(users)          # the fused path itself produced rows
    # what the planted rows must look like on every path
    keys, scores = out["dense"]
    for b, u in enumerate(users):
        if u == ALL:
            assert np.all(keys[b] == -1) and np.all(_bits(scores[b]) == 0)
        if u == BUT3 and not pooled:
            assert np.all(keys[b, 3:] == -1) and np.all(_bits(scores[b, 3:]) == 0)
            assert set(keys[b, :3]) <= {17, 3100, 5999, -1}
        valid = keys[b] >= 0
        assert not M[u, keys[b][valid]].any()          # nothing seen is ever listed


def _oracle_rows(train, M, which, P, Q, qb, pool, k, flt):
    """dot_topn (dense path) of each single user with pool = the items outside the user's seen row [intersected with `pool`]."""
    eng = _engine(None, 0, flt=flt)
    want_k = np.full((len(which), k), -1, dtype=np.int32)
    want_s = np.zeros((len(which), k), dtype=np.float32)          # nothing left to recommend: (-1, 0.0) in every slot
    for i, u in enumerate(which):
        unseen = np.flatnonzero(~M[u])
        if len(pool):
            unseen = np.intersect1d(unseen, pool)
        if len(unseen) == 0:
            continue
        kk, ss = tc.run(lambda *a: eng.dot_topn(*a[:8]), np.array([u], np.int32), P, Q, qb, unseen.astype(np.int32), k)
        want_k[i], want_s[i] = kk[0], ss[0]
    return want_k, want_s


@pytest.mark.parametrize("k,bias,pooled,flt", CASES)
def test_rows_equal_dot_topn_with_the_unseen_items_as_pool(k, bias, pooled, flt):
    """The planted users and 12 random ones, through the fused path (d = 96): keys, scores and padding of every row equal one
    dot_topn call for that user alone."""
    train, M, P, Q, Qb, pool, _ = common_input(96)
    qb = Qb if bias else tc.NO_BIAS
    pl = pool if pooled else tc.EMPTY_POOL
    which = np.ascontiguousarray(np.concatenate([np.random.default_rng(k).choice(np.arange(10, U), size=12, replace=False), PLANTED[::-1]]),
                                 dtype=np.int32)
    got_k, got_s = _recommend(_engine(train, 1, flt=flt), which, P, Q, qb, pl, k)
    want_k, want_s = _oracle_rows(train, M, which, P, Q, qb, pl, k, flt)
    assert np.array_equal(got_k, want_k), which[np.flatnonzero((got_k != want_k).any(axis=1))]
    assert np.array_equal(_bits(got_s), _bits(want_s)), which[np.flatnonzero((_bits(got_s) != _bits(want_s)).any(axis=1))]


@pytest.mark.parametrize("k", [5, 30, 250])
@pytest.mark.parametrize("bias,pooled", [(False, False), (True, False), (True, True)])
def test_rows_equal_the_cpu_specification(k, bias, pooled):
    """Integer factors (exact arithmetic), 40 users x 200 items, d = 12: every row equals `spec_dot_topn` with the user's own pool,
    on the dense path, the fused path and the fused path with a one-tile sample."""
    rng = np.random.default_rng(77)
    P, Q = tc.integer_factors(40, 12, seed=21), tc.integer_factors(200, 12, seed=22)
    Qb = tc.integer_factors(200, 1, seed=23, lo=-1, hi=2) if bias else tc.NO_BIAS
    M = rng.random((40, 200)) < 0.1
    M[0] = False
    M[1] = True
    M[2] = True
    M[2, [5, 77, 199]] = False
    rows, cols = np.nonzero(M)
    train = ec.csr_of(40, 200, rows, cols)
    pool = np.ascontiguousarray(rng.permutation(200)[:60], dtype=np.int32) if pooled else tc.EMPTY_POOL
    users = np.ascontiguousarray(np.concatenate([rng.permutation(40), [2, 1, 0, 7, 7]]), dtype=np.int32)
    want_k = np.full((len(users), k), -1, dtype=np.int32)
    want_s = np.zeros((len(users), k), dtype=np.float32)
    for b, u in enumerate(users):
        unseen = np.flatnonzero(~M[u])
        if pooled:
            unseen = np.intersect1d(unseen, pool)
        if len(unseen):
            kk, ss = tc.spec_dot_topn(np.array([u]), P, Q, Qb, unseen, k, False)
            want_k[b], want_s[b] = kk[0], ss[0]
    for fused, c0 in ((0, 0), (1, 0), (1, 32)):
        got_k, got_s = _recommend(_engine(train, fused, c0), users, P, Q, Qb, pool, k)
        assert np.array_equal(got_k, want_k), (fused, c0)
        assert np.array_equal(_bits(got_s), _bits(want_s)), (fused, c0)


def test_device_form_equals_the_host_form_on_a_training_handle():
    """After three BPRMF epochs: recommend_unseen_device from the handle's P / Q / Qb in HBM == the host form on the synchronised
    arrays, bit for bit, on the dense and on the fused path."""
    from conftest import bpr_opt
    from buffalo_amd.backend import CyBPR
    train, _, P0, Q0, Qb = ec.planted(U=200, I=300, d=20, bias=True, seed=9)
    d, vdim = 20, 32
    P, Q = H.pad(0.1 * P0, vdim), H.pad(0.1 * Q0, vdim)
    Qb = np.ascontiguousarray(0.1 * Qb)
    obj = H.run_hip_sgd(CyBPR, bpr_opt(d=d, lr=0.05, num_iters=3), train, P, Q, Qb, epochs=3)
    hP, hQ = np.ascontiguousarray(P[:, :d]), np.ascontiguousarray(Q[:, :d])
    users = np.ascontiguousarray(np.random.default_rng(3).permutation(200)[:150], dtype=np.int32)
    for fused in (0, 1):
        eng = _engine(train, fused)
        dk, ds = np.empty((150, 15), np.int32), np.empty((150, 15), np.float32)
        eng.recommend_unseen_device(users, obj.device_buffer("P")[0], 200, obj.device_buffer("Q")[0], 300, d, vdim, obj.device_buffer("Qb")[0],
                                    dk, ds, tc.EMPTY_POOL, 15)
        hk, hs = _recommend(eng, users, hP, hQ, Qb, tc.EMPTY_POOL, 15)
        assert np.array_equal(dk, hk) and np.array_equal(_bits(ds), _bits(hs)), fused
        k1, s1 = dk[users == 1][0], ds[users == 1][0]                  # ec.planted: user 1 has seen all but 3 items
        assert (k1[3:] == -1).all() and (s1[3:] == 0.0).all()           # beyond the user's own pool: (-1, 0.0)
        assert ((k1[:3] >= 0) | (s1[:3] == FMIN)).all()                 # inside it: an item, or (-1, FLT_MIN) under the FLT_MIN rule


def test_more_than_128_columns_stay_dense_and_equal_dot_topn():
    """d = 200 through the same call, module-level function included: two K-chunks, no fused path (merges stays 0)."""
    from buffalo_amd import parallel as par
    train, M, _, _, Qb, pool, users = common_input(96)
    rng = np.random.default_rng(200)
    P = rng.normal(scale=0.3, size=(U, 200)).astype(np.float32)
    Q = rng.normal(scale=0.3, size=(I, 200)).astype(np.float32)
    Q[3000:3300] = Q[3000]
    P[CONST] = 4.0 * Q[3000]
    which = np.ascontiguousarray(np.concatenate([PLANTED, [150, 151, 299]]), dtype=np.int32)
    eng = _engine(train, 1)
    for k, qb, pl in ((10, tc.NO_BIAS, tc.EMPTY_POOL), (100, Qb, pool)):
        got_k, got_s = _recommend(eng, which, P, Q, qb, pl, k)
        want_k, want_s = _oracle_rows(train, M, which, P, Q, qb, pl, k, 1)
        assert np.array_equal(got_k, want_k) and np.array_equal(_bits(got_s), _bits(want_s)), k
    assert eng.stats()["merges"] == 0
    par._engine().set_seen(train.indptr, train.keys, train.num_items)
    mk, ms = np.empty((len(which), 10), np.int32), np.empty((len(which), 10), np.float32)
    par.recommend_unseen(which, P, Q, tc.NO_BIAS, mk, ms, tc.EMPTY_POOL, 10)
    want_k, want_s = _oracle_rows(train, M, which, P, Q, tc.NO_BIAS, tc.EMPTY_POOL, 10, 1)
    assert np.array_equal(mk, want_k) and np.array_equal(_bits(ms), _bits(want_s))


def test_refusals_carry_their_own_message():
    from buffalo_amd._lib import BuffaloHipError
    train, _, P, Q, _ = ec.planted(d=24, seed=8)
    Un, In = train.num_users, train.num_items
    users = np.arange(5, dtype=np.int32)
    eng = _engine(None, -1)
    with pytest.raises(BuffaloHipError, match="set_seen has not been called"):
        _recommend(eng, users, P, Q, tc.NO_BIAS, tc.EMPTY_POOL, 10)
    bad = train.keys.copy()
    beg = int(train.indptr[2])                       # row 3 of ec.planted has at least two keys
    bad[beg], bad[beg + 1] = bad[beg + 1], bad[beg]
    assert bad[beg] > bad[beg + 1]
    with pytest.raises(BuffaloHipError, match="set_seen: the keys of a training row must ascend"):
        eng.set_seen(train.indptr, bad, In)
    with pytest.raises(BuffaloHipError, match="set_seen has not been called"):     # a refused matrix binds nothing
        _recommend(eng, users, P, Q, tc.NO_BIAS, tc.EMPTY_POOL, 10)
    eng.set_seen(train.indptr, train.keys, In)
    with pytest.raises(BuffaloHipError, match="one row per user of set_seen"):
        _recommend(eng, users, P[:-1].copy(), Q, tc.NO_BIAS, tc.EMPTY_POOL, 10)
    with pytest.raises(BuffaloHipError, match="one row per item of set_seen"):
        _recommend(eng, users, P, Q[:-1].copy(), tc.NO_BIAS, tc.EMPTY_POOL, 10)
    for outside in (-1, Un):
        with pytest.raises(BuffaloHipError, match="user outside"):
            _recommend(eng, np.array([0, outside], np.int32), P, Q, tc.NO_BIAS, tc.EMPTY_POOL, 10)
    for k in (0, 16385):
        with pytest.raises(BuffaloHipError, match="k must be in"):
            _recommend(eng, users, P, Q, tc.NO_BIAS, tc.EMPTY_POOL, k)
    got_k, got_s = _recommend(eng, users, P, Q, tc.NO_BIAS, tc.EMPTY_POOL, 10)      # the handle survives
    assert (got_k[0] >= 0).all() and (got_k[1, 3:] == -1).all()

