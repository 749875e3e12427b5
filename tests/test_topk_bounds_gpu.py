"""The selection kernels of csrc/topk_kernels.hpp at every bound they have, on planted score bits (tests/topk_planted.py: the module
docstring there maps each bound to its case and to the test below).  Every assertion is equality of keys and of score bits against
`oracle.dot_topn` (the FLT_MIN rule on) or against the closed form `topk_planted.spec_scores` (the rule off, quickselect's tie order);
tests/test_topk_planted_cpu.py holds the two to each other on all of these cases.  No tolerance anywhere."""
import numpy as np
import pytest

import topk_cases as tc
import topk_planted as tp

pytestmark = pytest.mark.gpu


def _engine(**modes):
    from buffalo_amd import parallel as par
    eng = par.TopK()
    for name, v in modes.items():
        eng.set_mode(name, v)
    return eng


def _dot_topn(eng, idx, P, Q, Qb, pool, k):
    return tc.run(lambda *a: eng.dot_topn(*a[:8]), idx, P, Q, Qb, pool, k)


def _same(got, want, what):
    rows = np.flatnonzero((got[0] != want[0]).any(axis=1) | (tp.bits(got[1]) != tp.bits(want[1])).any(axis=1))
    assert len(rows) == 0, (what, "rows", rows[:8].tolist(), got[0][rows[0]][:12], want[0][rows[0]][:12], got[1][rows[0]][:12], want[1][rows[0]][:12])


def _check(eng, oracle, S, k, d=None, what="", bias=False, pool=tc.EMPTY_POOL, planted=None):
    """dot_topn on the planted product of S (or the given (idx, P, Q)) == the oracle == the specification."""
    idx, P, Q = planted if planted is not None else tp.planted(S, d or max(8, len(S)))
    Qb = tp.some_bias(S.shape[1]) if bias else tc.NO_BIAS
    got = _dot_topn(eng, idx, P, Q, Qb, pool, k)
    _same(got, tc.run(oracle.dot_topn, idx, P, Q, Qb, pool, k), (what, k, "oracle"))
    _same(got, tp.spec_scores(S + Qb.T if bias else S, k, pool=pool), (what, k, "spec"))
    return got


def _check_quickselect(eng, oracle, S, k, what):
    """quickselect on the score matrix itself: the device's documented order (score desc, index desc) through the specification with the
    rule off, and the oracle's nth_element + sort where no two scores of a row are equal."""
    S = np.ascontiguousarray(S)
    got = np.full((len(S), k), -7, np.int32)
    eng.quickselect(S, got, True)
    assert np.array_equal(got, tp.spec_scores(S, k, rule=False)[0]), (what, k)
    if all(len(np.unique(r)) == len(r) for r in S):
        want = np.empty_like(got)
        oracle.quickselect(S, want, True)
        assert np.array_equal(got, want), (what, k, "oracle")


CASES = {c[0]: c for c in tp.dense_cases()}


# ------------------------------------------------------------------------------------------------
# dense selection
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast", [1, 0])
def test_low_key_bits_dense(oracle, fast):
    """Keys that share bits 31..20 and differ below: the second / third level of the fast path where the bin fits the candidate buffer
    (low_bits_fit), passes 2-4 of the multi-pass path where it does not (low_bits_full: 3,072 in one bin) or the fast path is off, one
    byte per pass (one_byte)."""
    eng = _engine(fused=0, fast_select=fast)
    for name in ("low_bits_fit", "low_bits_full", "one_byte"):
        _, S, _ = CASES[name]
        for k in (100, 101):
            _check(eng, oracle, S, k, what=name)
            _check_quickselect(eng, oracle, S, k, name)
        _check(eng, oracle, S, 100, what=name + " + bias", bias=True)
        tp.record("dense low bits", ["%s fast_select=%d: k = 100, 101, bias, quickselect: equal" % (name, fast)])


@pytest.mark.parametrize("fast", [1, 0])
def test_threshold_bin_at_the_candidate_buffer(oracle, fast):
    """1,024 admissible columns in the threshold bin: the last row the candidate buffer holds; 1,025: the first for the multi-pass path."""
    eng = _engine(fused=0, fast_select=fast)
    for name in ("bin_1024", "bin_1025"):
        _, S, ks = CASES[name]
        for k in ks:                                     # 10 deep into the bin, its first member, all but its last (whichever candidate a
            _check(eng, oracle, S, k, what=name)         # too-small buffer loses, that list is wrong), all of it
            _check_quickselect(eng, oracle, S, k, name)
        tp.record("dense candidate buffer", ["%s fast_select=%d: k = %s: equal" % (name, fast, ks)])


@pytest.mark.parametrize("fast", [1, 0])
def test_tie_walk_dense(oracle, fast):
    """Ties that straddle the k-th place: F ending on either side of the 64-lane waves and 256-column steps of the ordered walk, better
    scores behind F evicting the oldest ties, A over several steps; and a row without a straddle."""
    eng = _engine(fused=0, fast_select=fast)
    S, names = tp.ties_at()
    _check(eng, oracle, S, 10, what="ties_at")
    _check(eng, oracle, S, 10, what="ties_at + pool", pool=np.arange(0, 700, dtype=np.int32)[::-1].copy())
    _check_quickselect(eng, oracle, S, 10, "ties_at")
    _check(eng, oracle, tp.ties_wide(), 600, what="ties_wide")
    _check_quickselect(eng, oracle, tp.ties_wide(), 600, "ties_wide")
    tp.record("dense tie walk", ["fast_select=%d: %s, ties_wide: equal" % (fast, " ".join(names))])


def test_k_values_dense(oracle):
    """k = 1, 2, 3, across p2 = 1,024 / 2,048 / 4,096, k = q_rows, k = q_rows + 5, a pool smaller than k."""
    eng = _engine(fused=0)
    _, S, ks = CASES["low_bits_full"]
    for k in ks:
        got = _check(eng, oracle, S, k, what="low_bits_full")
        _check_quickselect(eng, oracle, S, min(k, S.shape[1]), "low_bits_full")
    assert np.all(got[0][:, 3072:] == -1) and np.all(tp.bits(got[1][:, 3072:]) == 0)
    pool = np.random.default_rng(5).permutation(3072)[:1500].astype(np.int32)
    got = _check(eng, oracle, S, 2049, what="pool of 1500", pool=pool)
    assert np.all(got[0][:, :1500] >= 0) and np.all(got[0][:, 1500:] == -1)
    tp.record("dense k values", ["low_bits_full k = %s, pool 1500 < k = 2049: equal" % (ks,)])


def test_largest_k(oracle):
    """TOPK_MAX_K = 16,384 runs (the 128 KiB sort buffer), on 16,400 columns with two queries."""
    S = tp.distinct_row(16400, nq=2)
    for fast in (1, 0):
        _check(_engine(fused=0, fast_select=fast), oracle, S, 16384, what="k = 16384")
    _check_quickselect(_engine(), oracle, S, 16384, "k = 16384")
    tp.record("dense k values", ["16,400 columns x 2 queries, k = 16384, fast_select 1 / 0, quickselect: equal"])


@pytest.mark.parametrize("cols", [1, 31, 32, 33, 255, 256, 257])
def test_candidate_counts(oracle, cols):
    eng = _engine(fused=0)
    S = tp.tiny_cols(cols)
    for k in (1, 2, 3, cols, cols + 5):
        _check(eng, oracle, S, k, what=cols)
        if k <= cols:
            _check_quickselect(eng, oracle, S, k, cols)
    _check(_engine(fused=1), oracle, S, 3, d=8, what=(cols, "fused"))


def test_few_admissible(oracle):
    """Fewer admissible columns than kk, exactly kk, none: take_all and the (-1, FLT_MIN) then (-1, 0.0) padding, k > q_rows, a pool < k."""
    _, S, ks = CASES["few"]
    for modes in (dict(fused=0), dict(fused=0, fast_select=0), dict(fused=1)):
        eng = _engine(**modes)
        for k in ks:
            got = _check(eng, oracle, S, k, what=("few", modes))
        assert np.all(got[0][0] == -1) and np.all(got[1][0, :40] == tp.FMIN) and np.all(tp.bits(got[1][0, 40:]) == 0)
        _check(eng, oracle, S, 45, what=("few + pool", modes), pool=np.arange(3, 33, dtype=np.int32))
    tp.record("dense few", ["0, 1, 6, 7, 39, 40 admissible of 40, k = 7, 40, 45, pool of 30: equal (dense, multi-pass, fused)"])


@pytest.mark.parametrize("modes", [dict(fused=0), dict(fused=0, fast_select=0), dict(fused=1)], ids=["dense", "multipass", "fused"])
def test_specials_rule_on(oracle, modes):
    """d = 1: +-0, subnormals, FLT_MIN, its successor, FLT_MAX, +-inf and NaNs in one row.  Only scores > FLT_MIN are listed, a NaN never
    is and moves nothing around it."""
    row = tp.specials(nan=True)
    planted = tp.planted_d1(row, 3)
    S = np.tile(row, (3, 1))
    eng = _engine(**modes)
    for k in (1, 3, 17, len(row), len(row) + 4):
        got = _check(eng, oracle, S, k, what="specials", planted=planted)
    listed = got[1][0][got[0][0] >= 0]
    assert len(listed) == (row > tp.FMIN).sum() and listed[0] == np.inf and listed[-1] == np.nextafter(np.float32(tp.FMIN), np.float32(1))


@pytest.mark.parametrize("modes", [dict(fused=0), dict(fused=0, fast_select=0), dict(fused=1)], ids=["dense", "multipass", "fused"])
def test_specials_rule_off(modes):
    """The same row without NaN, the rule off (no oracle: the specification): negative scores, zeros of both signs -- they tie, by column,
    and are listed as +0.0 -- and subnormals in their order."""
    row = tp.specials(nan=False)
    idx, P, Q = tp.planted_d1(row, 3)
    S = np.tile(row, (3, 1))
    eng = _engine(flt_min_rule=0, **modes)
    for k in (1, 5, 20, 23, 30, len(row), len(row) + 4):
        _same(_dot_topn(eng, idx, P, Q, tc.NO_BIAS, tc.EMPTY_POOL, k), tp.spec_scores(S, k, rule=False), ("specials, rule off", k))
    got = np.empty((1, 30), np.int32)
    _engine().quickselect(np.ascontiguousarray(row[None, :]), got, True)          # -0.0 arrives as it is here
    assert np.array_equal(got, tp.spec_scores(row[None, :], 30, rule=False)[0])


# ------------------------------------------------------------------------------------------------
# the score kernel
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [1, 31, 32, 33, 127, 128, 129])
def test_score_kernel_query_counts(oracle, nq):
    """Each query its own planted column; d = 128 (one full K-chunk) and d = 200 (a second, guarded one)."""
    for d in (128, 200):
        S, idx, P, Q = tp.score_case(d, nq)
        _check(_engine(fused=0), oracle, S, 10, what=(d, nq), planted=(idx, P, Q))
    S, idx, P, Q = tp.score_case(128, nq)
    _check(_engine(fused=1), oracle, S, 10, what=(128, nq, "fused"), planted=(idx, P, Q), bias=True)


@pytest.mark.parametrize("d", [1, 8, 64, 72, 120, 128, 136, 200, 256])
def test_score_kernel_columns(oracle, d):
    """The plant at factor column 0, W/2 - 1, W/2 (the half-wave split), d - 1, and for d > 128 at 127, 128 (the second chunk reads what
    the first stored) and at the second chunk's own split: a column the kernel drops or counts twice changes that query's every score."""
    nq = min(max(d, 8), 129)
    S, idx, P, Q = tp.score_case(d, nq)
    assert set(tp.plant_columns(d)) <= set(np.nonzero(P[idx])[1].tolist())
    _check(_engine(fused=0), oracle, S, 10, what=d, planted=(idx, P, Q))
    _check(_engine(fused=0), oracle, S, 10, what=(d, "bias"), planted=(idx, P, Q), bias=True)
    if d <= 128:
        _check(_engine(fused=1), oracle, S, 10, what=(d, "fused"), planted=(idx, P, Q))
    tp.record("score kernel", ["d = %d, %d queries, planted columns %s (+ the others in turn): equal" % (d, nq, tp.plant_columns(d))])


def test_score_kernel_many_tiles(oracle):
    """1,280 queries x 6,600 candidates, d = 128: 207 tiles x 10 query blocks on 8 x 256 slots -> two tiles per group, a last group of one."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus == 256, "the shape is sized for 256 CUs: n_tiles * qblocks = 2,070 > 8 * CUs = 2,048 gives two tiles per group"
    S, idx, P, Q = tp.score_case(128, 1280, cols=6600)
    _check(_engine(fused=0), oracle, S, 10, what="1280 x 6600", planted=(idx, P, Q))
    tp.record("score kernel", ["1,280 x 6,600, d = 128 (%d CUs): equal" % cus])


# ------------------------------------------------------------------------------------------------
# the fused path, each route
# ------------------------------------------------------------------------------------------------
def _route_engine(route, **more):
    c0, wave = tp.ROUTES[route]
    return _engine(fused=1, fused_c0=c0, wave_select=wave, **more)


@pytest.mark.parametrize("nq", [1, 3, 4, 5, 129])
@pytest.mark.parametrize("route", list(tp.ROUTES))
def test_fused_routes(oracle, route, nq):
    """6,176 candidates, d = 128, k = 10: 8 segments with cap_seg = 512 on every route (`topk_planted.fused_layout` derives it; the redo
    counts below hold only if it is so).  Rows at 512 / 513 columns in one segment, list totals 2,048 / 2,049, 512 / 513 sample winners,
    ties straddling the k-th place, a sample that bounds nothing, nothing admissible.  `merges` = the rows handed back to the dense
    path = exactly the planted overflow rows; `exchanges` = the rows the wave kernel passed to the block-level tie walk = exactly the
    planted tie rows that did not overflow (none on the block route, which selects every row at block level)."""
    names, S, over, strad = tp.fused_rows(route)
    queries = np.arange(nq) % len(S)
    planted = tp.planted(S, 128, cols_at=np.arange(len(S)) * 9 % 128, queries=queries)
    eng = _route_engine(route)
    _check(eng, oracle, S[queries], 10, what=(route, nq), planted=planted)
    st = eng.stats()
    want_redo = int(over[queries].sum())
    want_general = int((strad & ~over)[queries].sum()) if tp.ROUTES[route][1] else 0
    tp.record("fused routes", ["%s, %d queries: equal; merges %d (planted %d) exchanges %d (planted %d)"
                               % (route, nq, st["merges"], want_redo, st["exchanges"], want_general)])
    assert st["merges"] == want_redo, [names[i] for i in queries[:len(S)]]
    assert st["exchanges"] == want_general


@pytest.mark.parametrize("route", list(tp.ROUTES))
def test_low_key_bits_fused(oracle, route):
    """wave_kth_key's levels over key bits 19..8 and 7..0 (sample thresholds: topk_thr_wave_kernel; lists: topk_list_wave_kernel) and the
    block route's list-mode select, on keys that share their top bits."""
    S = tp.low_bits_fused()
    planted = tp.planted(S, 128)
    for k in (10, 100):
        eng = _route_engine(route)
        _check(eng, oracle, S, k, what=(route, "low bits"), planted=planted)
        if route != "c0_32" and k == 10:                  # (a 32-column sample bounds too little for 6,176 distinct scores)
            assert eng.stats()["merges"] == 0
        tp.record("fused low bits", ["%s k = %d: equal; merges %d" % (route, k, eng.stats()["merges"])])


@pytest.mark.parametrize("route", list(tp.ROUTES))
def test_tie_walk_fused(oracle, route):
    """The ties_at rows through the list-mode tie walk (the list sorted by column first): F ends at list position 63 ... 512."""
    S, names = tp.ties_fused(route)
    eng = _route_engine(route)
    _check(eng, oracle, S, 10, what=(route, "ties"), planted=tp.planted(S, 128))
    st = eng.stats()
    tp.record("fused tie walk", ["%s: equal; merges %d exchanges %d of %d rows" % (route, st["merges"], st["exchanges"], len(S))])
    assert st["merges"] == 0 and st["exchanges"] == (len(S) - 1 if tp.ROUTES[route][1] else 0)


@pytest.mark.parametrize("wave", [1, 0])
def test_fused_wave_list_switch(oracle, wave):
    """kk = 1,024 (p2 = 1,024: topk_list_wave_kernel) and 1,025 (p2 = 2,048: list-mode topk_select_kernel for every row)."""
    S = tp.distinct_row(tp.FUSED_COLS, seed=21, nq=3)
    planted = tp.planted(S, 128)
    for k in (1024, 1025):
        eng = _engine(fused=1, wave_select=wave)
        _check(eng, oracle, S, k, what=("wave_list", wave), planted=planted)
        assert eng.stats()["merges"] == 0
        tp.record("fused wave_list switch", ["wave_select=%d kk = %d: equal; merges 0" % (wave, k)])


# ------------------------------------------------------------------------------------------------
# seen-aware
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["dense"] + list(tp.ROUTES))
def test_seen_aware(route):
    """recommend_unseen on planted scores: seen columns at the best and at the k-th place, the ten best, the last sampled / first swept
    column of every route, runs of 64 and 65 keys inside the sample, the listed member of a tie, all but four columns, all columns --
    against the specification and against dot_topn with the unseen columns as the pool."""
    S, M = tp.seen_case()
    _, P, Q = tp.planted(S, 128)
    users = np.ascontiguousarray(np.concatenate([np.arange(10)[::-1], [8, 3, 9, 0]]), dtype=np.int32)
    eng = _engine(fused=0) if route == "dense" else _route_engine(route)
    eng.set_seen(*tp.csr_of_seen(M), tp.FUSED_COLS)
    keys = np.full((len(users), 10), 12345, np.int32)
    scores = np.full((len(users), 10), 9.75, np.float32)
    eng.recommend_unseen(users, P, Q, tc.NO_BIAS, keys, scores, tc.EMPTY_POOL, 10)
    _same((keys, scores), tp.spec_scores(S[users], 10, exclude=M[users]), (route, "spec"))
    plain = _engine(fused=0)
    for b, u in enumerate(users[:10]):
        unseen = np.flatnonzero(~M[u]).astype(np.int32)
        if len(unseen):
            want = _dot_topn(plain, np.array([u], np.int32), P, Q, tc.NO_BIAS, unseen, 10)
        else:
            want = np.full((1, 10), -1, np.int32), np.zeros((1, 10), np.float32)
        _same((keys[b:b + 1], scores[b:b + 1]), want, (route, "dot_topn with the complement pool", u))
    tp.record("seen-aware", ["%s: 14 users equal to the specification, 10 to dot_topn with the complement pool; merges %d" % (route, eng.stats()["merges"])])
