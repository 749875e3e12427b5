"""The yardstick of tests/test_topk_bounds_gpu.py, proven without a GPU: the score-matrix form of the specification
(`topk_planted.spec_scores`) equals `oracle.dot_topn` -- keys and score BITS -- on every planted case the device file runs, the planted
product really is the planted score, every builder's premise holds (the builders assert them; here they all run), and three planted
defects of the kind a tolerance forgives each change the compared arrays."""
import numpy as np
import pytest

import topk_cases as tc
import topk_planted as tp


def _same(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, np.flatnonzero((got[0] != want[0]).any(axis=1))[:5])
    assert np.array_equal(tp.bits(got[1]), tp.bits(want[1])), (what, np.flatnonzero((tp.bits(got[1]) != tp.bits(want[1])).any(axis=1))[:5])


def _oracle(oracle, idx, P, Q, Qb, pool, k):
    return tc.run(oracle.dot_topn, idx, P, Q, Qb, pool, k)


@pytest.mark.parametrize("name,S,ks", tp.dense_cases(), ids=[c[0] for c in tp.dense_cases()])
def test_spec_equals_oracle_on_the_dense_cases(oracle, name, S, ks):
    d = max(8, len(S))
    idx, P, Q = tp.planted(S, d, cols_at=np.arange(len(S))[::-1] + d - len(S))
    assert np.array_equal(tp.bits(P @ Q.T), tp.bits(S + np.float32(0.0)))                   # the plant arrives bit for bit
    Qb = tp.some_bias(S.shape[1])
    for k in ks:
        _same(tp.spec_scores(S, k), _oracle(oracle, idx, P, Q, tc.NO_BIAS, tc.EMPTY_POOL, k), (name, k))
    k = ks[0]
    _same(tp.spec_scores(S + Qb.T, k), _oracle(oracle, idx, P, Q, Qb, tc.EMPTY_POOL, k), (name, "bias"))
    pool = np.random.default_rng(1).permutation(S.shape[1])[:max(1, min(k, S.shape[1]) - 2)].astype(np.int32)    # a pool smaller than k
    _same(tp.spec_scores(S, k, pool=pool), _oracle(oracle, idx, P, Q, tc.NO_BIAS, pool, k), (name, "pool"))
    # and the closed form this one restates, on its own terms (exact float64 dot products of unit vectors)
    small = min(len(S), 2)
    _same(tp.spec_scores(S[:small], k), tc.spec_dot_topn(idx[:small], P, Q, tc.NO_BIAS, tc.EMPTY_POOL, k, False), (name, "spec_dot_topn"))


@pytest.mark.parametrize("cols", [1, 31, 32, 33, 255, 256, 257])
def test_spec_equals_oracle_on_the_candidate_counts(oracle, cols):
    S = tp.tiny_cols(cols)
    idx, P, Q = tp.planted(S, 8)
    for k in (1, 2, 3, cols, cols + 5):
        _same(tp.spec_scores(S, k), _oracle(oracle, idx, P, Q, tc.NO_BIAS, tc.EMPTY_POOL, k), (cols, k))


def test_spec_equals_oracle_on_the_largest_k(oracle):
    S = tp.distinct_row(16400, nq=2)
    idx, P, Q = tp.planted(S, 8)
    _same(tp.spec_scores(S, 16384), _oracle(oracle, idx, P, Q, tc.NO_BIAS, tc.EMPTY_POOL, 16384), "k = 16384")


def test_spec_equals_oracle_on_the_specials(oracle):
    """d = 1, NaN and +-inf in the row: the rule's `score > last` is false for NaN, which therefore never enters and moves nothing."""
    row = tp.specials(nan=True)
    idx, P, Q = tp.planted_d1(row, 3)
    S = np.tile(row, (3, 1))
    for k in (1, 3, 17, len(row), len(row) + 4):
        got = tp.spec_scores(S, k)
        _same(got, _oracle(oracle, idx, P, Q, tc.NO_BIAS, tc.EMPTY_POOL, k), k)
        assert np.all(got[1][got[0] >= 0] > tp.FMIN) and not np.isnan(got[1]).any()
    # the rule off has no oracle: the order of everything below FLT_MIN by the specification's own properties
    row = tp.specials(nan=False)
    keys, vals = tp.spec_scores(row[None, :], len(row), rule=False)
    assert sorted(keys[0].tolist()) == list(range(len(row))) and np.all(vals[0][:-1] >= vals[0][1:])
    zeros = keys[0][vals[0] == 0]
    assert len(zeros) == 6 and np.all(np.diff(zeros) < 0) and np.all(tp.bits(vals[0][vals[0] == 0]) == 0)      # +-0 tie: by column, listed as +0.0


@pytest.mark.parametrize("d,nq", [(1, 129), (8, 33), (64, 129), (72, 127), (120, 128), (128, 129), (136, 129), (200, 129), (256, 129)])
def test_spec_equals_oracle_on_the_score_cases(oracle, d, nq):
    S, idx, P, Q = tp.score_case(d, nq)
    assert np.array_equal(tp.bits(P[idx] @ Q.T), tp.bits(S))
    assert set(tp.plant_columns(d)) <= set(np.nonzero(P[idx])[1].tolist())
    _same(tp.spec_scores(S, 10), _oracle(oracle, idx, P, Q, tc.NO_BIAS, tc.EMPTY_POOL, 10), d)
    Qb = tp.some_bias(S.shape[1])
    _same(tp.spec_scores(S + Qb.T, 10), _oracle(oracle, idx, P, Q, Qb, tc.EMPTY_POOL, 10), (d, "bias"))


@pytest.mark.parametrize("route", list(tp.ROUTES))
def test_spec_equals_oracle_on_the_fused_rows(oracle, route):
    """... and the premises of the rows: counts per segment, sample winners and list totals at the bounds (asserted in the builder from
    the restated plan), overflow and straddle flags as planted."""
    names, S, over, strad = tp.fused_rows(route)
    c0, sample_seg, segs, cap_seg = tp.fused_layout(route)
    assert cap_seg == 512 and len(segs) == 8 and segs[-1][1] == tp.FUSED_COLS
    if route == "c0_32":
        assert all(b - a == 768 for a, b in segs) and segs[0][0] == 32
    assert over.sum() == (3 if route == "c0_1024" else 2) and strad.sum() == (4 if route == "c0_1024" else 2)
    queries = np.arange(129) % len(S)
    idx, P, Q = tp.planted(S, 128, cols_at=np.arange(len(S)) * 9 % 128, queries=queries)
    _same(tp.spec_scores(S[queries], 10), _oracle(oracle, idx, P, Q, tc.NO_BIAS, tc.EMPTY_POOL, 10), route)


@pytest.mark.parametrize("route", list(tp.ROUTES))
def test_spec_equals_oracle_on_the_fused_low_bits_and_tie_rows(oracle, route):
    S = tp.low_bits_fused()
    idx, P, Q = tp.planted(S, 128)
    for k in (10, 100):
        _same(tp.spec_scores(S, k), _oracle(oracle, idx, P, Q, tc.NO_BIAS, tc.EMPTY_POOL, k), k)
    S, names = tp.ties_fused(route)
    c0 = tp.fused_layout(route)[0]
    assert not (S[:, :c0] > tp.FMIN).any() and all(not o for o, _, _, _ in (tp.fused_predict(r, route) for r in S))
    assert [tp.fused_predict(r, route)[1] for r in S] == [n != "exact" for n in names]
    idx, P, Q = tp.planted(S, 128)
    _same(tp.spec_scores(S, 10), _oracle(oracle, idx, P, Q, tc.NO_BIAS, tc.EMPTY_POOL, 10), route)


def test_spec_equals_oracle_on_the_wave_list_switch_and_the_seen_rows(oracle):
    S = tp.distinct_row(tp.FUSED_COLS, seed=21, nq=3)
    idx, P, Q = tp.planted(S, 128)
    for k in (1024, 1025):
        _same(tp.spec_scores(S, k), _oracle(oracle, idx, P, Q, tc.NO_BIAS, tc.EMPTY_POOL, k), k)
    S, M = tp.seen_case()
    idx, P, Q = tp.planted(S, 128)
    want = tp.spec_scores(S, 10, exclude=M)
    for u in range(len(S)):                     # the documented meaning of a row: dot_topn with the unseen columns as the pool
        unseen = np.flatnonzero(~M[u]).astype(np.int32)
        if len(unseen):
            got = _oracle(oracle, idx[u:u + 1], P, Q, tc.NO_BIAS, unseen, 10)
        else:
            got = np.full((1, 10), -1, np.int32), np.zeros((1, 10), np.float32)
        _same(got, (want[0][u:u + 1], want[1][u:u + 1]), u)
    assert (want[0][8] >= 0).sum() == 4 and np.all(tp.bits(want[1][8, 4:]) == 0) and np.all(want[0][9] == -1)


def test_spec_equals_oracle_on_the_many_tiles_shape(oracle):
    S, idx, P, Q = tp.score_case(128, 1280, cols=6600)
    _same(tp.spec_scores(S, 10), _oracle(oracle, idx, P, Q, tc.NO_BIAS, tc.EMPTY_POOL, 10), "1280 x 6600")


def test_planted_defects_change_the_compared_arrays():
    """What `==` on keys and score bits sees and the older float comparison (2e-6 of the row's largest score, any key in the last slot
    or inside a near-tie) does not."""
    # 1. the wrong one of two ties kept
    S = tp.ties_at()[0][:1]
    keys, vals = tp.spec_scores(S, 10)
    tied = np.flatnonzero(S[0] == vals[0, 9])
    other = [c for c in tied if c not in keys[0]][0]
    bad = keys.copy()
    bad[0, np.flatnonzero(vals[0] == vals[0, 9])[0]] = other
    assert np.array_equal(tp.bits(S[0][bad[0]]), tp.bits(vals[0])) and not np.array_equal(bad, keys)      # same scores: only the key tells
    # 2. the k-th entry swapped for the (k + 1)-th, which differs only in bit 3
    row = tp.distinct(np.random.default_rng(0), 50, tp.WORSE)
    row[[7, 33]] = tp.f32([tp.ONE | 0x18, tp.ONE | 0x10])
    keys, vals = tp.spec_scores(row[None, :], 1)
    assert keys[0, 0] == 7
    bad_k, bad_v = np.array([[33]], np.int32), row[[33]][None, :]
    assert abs(float(bad_v[0, 0]) - float(vals[0, 0])) <= 2e-6 * float(vals[0, 0])                       # inside the old tolerance ...
    assert not np.array_equal(tp.bits(bad_v), tp.bits(vals)) and not np.array_equal(bad_k, keys)          # ... and caught here
    # 3. a -0.0 listed as a different column / with its sign
    row = np.array([3.0, -0.0, -1.0, 0.0, 2.0, -0.0], np.float32)
    keys, vals = tp.spec_scores(row[None, :], 3, rule=False)
    assert keys.tolist() == [[0, 4, 3]] and tp.bits(vals).tolist() == [[0x40400000, 0x40000000, 0]]       # F = columns 0, 1, 3: the later zero stays
    bad_k, bad_v = keys.copy(), vals.copy()
    bad_k[0, 2], bad_v[0, 2] = 5, row[5]
    assert np.array_equal(bad_v, vals)                                                                    # -0.0 == 0.0 as floats ...
    assert not np.array_equal(bad_k, keys) and not np.array_equal(tp.bits(bad_v), tp.bits(vals))         # ... not as columns or bits
