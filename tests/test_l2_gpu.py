"""Ranking by squared distance ("score_func" = 1 of bfh_topk_set_mode / bfh_eval_set_mode; TopK.set_score_func, Evaluator.set_score_func,
parallel.l2_*).  Every test sets the mode, which the library refused before it knew L2.

* Key equivalence: the keys of an L2 call are the keys of the same call in dot mode with "flt_min_rule" = 0 and Qb = l2_cases.half_norms(Q),
  with the same `merges` / `exchanges` -- on the dense path and on every fused route, with a pool, with self-exclusion, with seen rows.
  This pins ties, padding and routes to what the planted-bits tests of the dot mode hold, and the bits of the hb kernel with them.
* Distance bits: `out_scores` are l2_cases.sqdist32 of (query, key) bit for bit, +inf where the key is -1.
* Exact cases (coordinates k / 8): the lists are the float64 order outright.
* Float cases (rows inside the unit ball, near-duplicates 1e-3 from the queries): the tau rule, derived in l2_cases' docstring.
* Validation, end to end through CyWARP, refusals, and the default mode's bits after a round trip through L2."""
import functools

import numpy as np
import pytest

import eval_cases as ec
import l2_cases as lc
import topk_cases as tc

pytestmark = pytest.mark.gpu

INF = np.float32(np.inf)
# d -> (queries, candidates): 1 .. 129 queries, 1 .. 257 candidates, every d of the restatement tests
SHAPES = {1: (1, 1), 7: (5, 33), 8: (33, 257), 9: (129, 64), 20: (64, 257), 127: (17, 100), 128: (129, 257), 129: (32, 31), 136: (5, 200),
          200: (40, 257), 256: (9, 129), 300: (33, 257)}
GRID = ((1, 9, 2, 11), (7, 40, 3, 12), (8, 60, 5, 13), (20, 257, 9, 14), (128, 257, 9, 15), (136, 200, 5, 16), (300, 129, 5, 17))   # as tests/test_l2_cpu.py
FUSED_ROWS = 6176
ROUTES = ((32, 1), (1024, 1), (32, 0), (1024, 0))      # "fused_c0", "wave_select" under "fused" = 1


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _engine(l2, fused=0, c0=0, wave=1):
    """An engine per mode set: the L2 one, or its dot-mode twin (every score admissible) that is handed hb as the bias."""
    from buffalo_amd import parallel as par
    eng = par.TopK()
    eng.set_mode("fused", fused)
    eng.set_mode("fused_c0", c0)
    eng.set_mode("wave_select", wave)
    if l2:
        eng.set_score_func("l2")
    else:
        eng.set_mode("flt_min_rule", 0)
    return eng


def _out(n, k):
    return np.full((n, k), 12345, dtype=np.int32), np.full((n, k), 9.75, dtype=np.float32)


def _hb(Q):
    return np.ascontiguousarray(lc.half_norms(Q).reshape(-1, 1))


def _counted(eng, fn):
    eng.reset_stats()
    out = fn()
    st = eng.stats()
    return out, (st["merges"], st["exchanges"])


def _topn(eng, idx, P, Q, Qb, pool, k):
    keys, scores = _out(len(idx), k)
    eng.dot_topn(idx, P, Q, Qb, keys, scores, pool, k)
    return keys, scores


def _unseen(eng, users, P, Q, Qb, pool, k):
    keys, scores = _out(len(users), k)
    eng.recommend_unseen(users, P, Q, Qb, keys, scores, pool, k)
    return keys, scores


def _similar(eng, idx, F, pool, k):
    keys, scores = _out(len(idx), k)
    eng.most_similar(idx, F, keys, scores, pool, k)
    return keys, scores


def _vectors(eng, V, F, pool, k):
    keys, scores = _out(len(V), k)
    eng.most_similar_vectors(V, F, keys, scores, pool, k)
    return keys, scores


def _device(a, extra=8, fill=7.5):
    """a [rows, d] as a torch tensor [rows, ld] in HBM, ld = ceil8(d) + extra: columns [d, ceil8(d)) zero, the rest `fill` -- no sweep
    reads them, and a norm summed over the pitch would."""
    import torch
    d_pad = (a.shape[1] + 7) // 8 * 8
    padded = np.full((a.shape[0], d_pad + extra), fill, dtype=np.float32)
    padded[:, :d_pad] = 0.0
    padded[:, :a.shape[1]] = a
    t = torch.from_numpy(padded).cuda()
    torch.cuda.synchronize()
    return t, d_pad + extra


def _distance_bits(keys, scores, V, Q, what):
    """out_scores of query vectors V: sqdist32 of (query, key) bit for bit, +inf in the empty slots."""
    for b in range(len(V)):
        listed = keys[b] >= 0
        assert np.array_equal(_bits(scores[b, listed]), _bits(lc.sqdist32(Q[keys[b, listed]], V[b]))), (what, b)
        assert (scores[b, ~listed] == INF).all(), (what, b)


def _tau_rule(keys, scores, V, Q, D, adm, what):
    bad, share = lc.tau_rule(keys, D, adm, lc.tau(V, Q), scores)
    assert not bad, (what, bad[:10])
    return share


@functools.lru_cache(maxsize=None)
def _seen(users, items, seed):
    """A training matrix over `users` x `items`: ~30 % of the items per user, user 0 with none, the last user with all but (at most) 3."""
    rng = np.random.default_rng(seed)
    M = rng.random((users, items)) < 0.3
    M[0] = False
    M[users - 1] = True
    M[users - 1, rng.choice(items, size=min(3, items), replace=False)] = False
    rows, cols = np.nonzero(M)
    return ec.csr_of(users, items, rows, cols)


def _bind(train, *engines):
    for eng in engines:
        eng.set_seen(train.indptr, train.keys, train.num_items)


def _pool(rows, seed):
    return np.ascontiguousarray(np.random.default_rng(seed).permutation(rows)[:max(1, rows // 3)], dtype=np.int32)


_D64 = {}


def _dist(P, Q):
    """dist64 of a cached case (float_case returns the same read-only arrays every time), computed once."""
    at = (P.ctypes.data, Q.ctypes.data, P.shape, Q.shape)
    if at not in _D64:
        _D64[at] = lc.dist64(P, Q)
    return _D64[at]


def _calls_agree(l2, dot, P, Q, k, what):
    """dot_topn (host and device form, with and without a pool), recommend_unseen, the three most_similar: keys and counters of the L2
    engine against its dot twin, distance bits, tau rule.  Returns the largest share of tau seen."""
    nq, rows = P.shape[0], Q.shape[0]
    rng = np.random.default_rng(rows * 1000 + nq)
    idx = np.ascontiguousarray(rng.permutation(nq), dtype=np.int32)
    pool, hb = _pool(rows, nq), _hb(Q)
    D = _dist(P, Q)
    share = 0.0
    for pl in (tc.EMPTY_POOL, pool):
        got, c1 = _counted(l2, lambda: _topn(l2, idx, P, Q, tc.NO_BIAS, pl, k))
        want, c2 = _counted(dot, lambda: _topn(dot, idx, P, Q, hb, pl, k))
        assert np.array_equal(got[0], want[0]) and c1 == c2, (what, "dot_topn", len(pl), c1, c2)
        _distance_bits(*got, P[idx], Q, (what, "dot_topn"))
        share = max(share, _tau_rule(*got, P[idx], Q, D[idx], lc.admissible(nq, rows, pool=pl), (what, "dot_topn", len(pl))))
    dP, ldp = _device(P)
    dQ, ldq = _device(Q)
    assert ldp == ldq
    keys, scores = _out(nq, k)
    l2.dot_topn_device(idx, dP.data_ptr(), nq, dQ.data_ptr(), rows, P.shape[1], ldq, None, False, keys, scores, pool, k)
    assert np.array_equal(keys, got[0]) and np.array_equal(_bits(scores), _bits(got[1])), (what, "dot_topn_device")
    # seen rows
    train = _seen(nq, rows, 7)
    _bind(train, l2, dot)
    runs = lc.seen_runs(train, idx)
    for pl in (tc.EMPTY_POOL, pool):
        got, c1 = _counted(l2, lambda: _unseen(l2, idx, P, Q, tc.NO_BIAS, pl, k))
        want, c2 = _counted(dot, lambda: _unseen(dot, idx, P, Q, hb, pl, k))
        assert np.array_equal(got[0], want[0]) and c1 == c2, (what, "recommend_unseen", len(pl), c1, c2)
        _distance_bits(*got, P[idx], Q, (what, "recommend_unseen"))
        share = max(share, _tau_rule(*got, P[idx], Q, D[idx], lc.admissible(nq, rows, pool=pl, seen=runs), (what, "recommend_unseen", len(pl))))
    keys, scores = _out(nq, k)
    l2.recommend_unseen_device(idx, dP.data_ptr(), nq, dQ.data_ptr(), rows, P.shape[1], ldq, None, keys, scores, pool, k)
    assert np.array_equal(keys, got[0]) and np.array_equal(_bits(scores), _bits(got[1])), (what, "recommend_unseen_device")
    # the rows of Q among themselves: a query's own row is left out, nothing is normalised
    sidx = np.ascontiguousarray(np.concatenate([rng.integers(0, rows, size=min(nq, 40)), [rows - 1, 0]]), dtype=np.int32)
    Ds = lc.dist64(Q[sidx], Q)
    q0 = Q.tobytes()
    for pl in (tc.EMPTY_POOL, pool):
        got, c1 = _counted(l2, lambda: _similar(l2, sidx, Q, pl, k))
        want, c2 = _counted(dot, lambda: _topn(dot, sidx, Q, Q, hb, pl, k))       # P is Q: self-exclusion
        assert np.array_equal(got[0], want[0]) and c1 == c2, (what, "most_similar", len(pl), c1, c2)
        assert all(q not in got[0][b] for b, q in enumerate(sidx))
        _distance_bits(*got, Q[sidx], Q, (what, "most_similar"))
        share = max(share, _tau_rule(*got, Q[sidx], Q, Ds, lc.admissible(len(sidx), rows, self_idx=sidx, pool=pl), (what, "most_similar", len(pl))))
    keys, scores = _out(len(sidx), k)
    l2.most_similar_device(sidx, dQ.data_ptr(), rows, Q.shape[1], ldq, keys, scores, pool, k)
    assert np.array_equal(keys, got[0]) and np.array_equal(_bits(scores), _bits(got[1])), (what, "most_similar_device")
    V = np.ascontiguousarray(np.concatenate([P[:3], Q[sidx[:3]]]))                 # vectors, some of them rows of Q: nothing is left out
    got, c1 = _counted(l2, lambda: _vectors(l2, V, Q, tc.EMPTY_POOL, k))
    want, c2 = _counted(dot, lambda: _topn(dot, np.arange(len(V), dtype=np.int32), V, Q, hb, tc.EMPTY_POOL, k))
    assert np.array_equal(got[0], want[0]) and c1 == c2, (what, "most_similar_vectors")
    _distance_bits(*got, V, Q, (what, "most_similar_vectors"))
    share = max(share, _tau_rule(*got, V, Q, lc.dist64(V, Q), lc.admissible(len(V), rows), (what, "most_similar_vectors")))
    assert Q.tobytes() == q0
    return share


@pytest.mark.parametrize("d", lc.DS)
def test_float_cases_every_call(d):
    """Every d of the restatement (d = 256 / 300: the second K-chunk of the sweep, the pairwise split of the sums), k = 1 (inside the block of
    near-duplicates), 10, and more than there are candidates (padding: +inf); dense, and at d <= 128 the fused route with a one-tile sample."""
    nq, rows = SHAPES[d]
    P, Q = lc.float_case(d, nq, rows, 400 + d)
    for fused, c0 in ((0, 0), (1, 32)) if d <= 128 else ((0, 0),):
        l2, dot = _engine(True, fused, c0), _engine(False, fused, c0)
        for k in (1, 10, rows + 3):
            share = _calls_agree(l2, dot, P, Q, k, (d, fused, k))
            print("d = %d, %d x %d, fused = %d, k = %d: largest share of tau %.4f" % (d, nq, rows, fused, k, share))


@functools.lru_cache(maxsize=None)
def _fused_case(nq):
    P, Q = lc.float_case(128, nq, FUSED_ROWS, 900 + nq)
    return P, Q


@pytest.mark.parametrize("nq", [1, 5, 129])
@pytest.mark.parametrize("c0,wave", ROUTES)
def test_fused_routes(c0, wave, nq):
    """6,176 candidates at d = 128 under "fused" = 1: a one-tile sample (most rows overflow their lists and take the dense redo), 1,024
    sampled columns, wave-level and block-level selection."""
    P, Q = _fused_case(nq)
    l2, dot = _engine(True, 1, c0, wave), _engine(False, 1, c0, wave)
    for k in (10, 100):
        share = _calls_agree(l2, dot, P, Q, k, (c0, wave, nq, k))
        print("fused_c0 = %d, wave_select = %d, %d queries, k = %d: largest share of tau %.4f" % (c0, wave, nq, k, share))


@pytest.mark.parametrize("d,rows,nq,seed", GRID)
def test_exact_cases_equal_the_float64_order(d, rows, nq, seed):
    """Coordinates k / 8: keys and distances are exact, every distance of a query distinct (tests/test_l2_cpu.py), so the lists ARE the
    float64 lists and the scores the float64 distances; with the planted tie the full list falls by (distance, index descending)."""
    F = lc.grid_matrix(d, rows, nq, seed)
    P = F[:nq].copy()                                     # its own memory: the same pointer would mean self-exclusion
    idx = np.arange(nq, dtype=np.int32)
    D = lc.dist64(P, F)
    train = _seen(nq, rows, 3)
    runs = lc.seen_runs(train, idx)
    for fused in (0, 1) if d <= 128 else (0,):
        l2 = _engine(True, fused, 32 if fused else 0)
        _bind(train, l2)
        for k in (1, 10, rows):
            for name, got, adm in (("dot_topn", _topn(l2, idx, P, F, tc.NO_BIAS, tc.EMPTY_POOL, k), lc.admissible(nq, rows)),
                                   ("most_similar", _similar(l2, idx, F, tc.EMPTY_POOL, k), lc.admissible(nq, rows, self_idx=idx)),
                                   ("recommend_unseen", _unseen(l2, idx, P, F, tc.NO_BIAS, tc.EMPTY_POOL, k), lc.admissible(nq, rows, seen=runs))):
                want = lc.lists64(D, adm, k)
                assert np.array_equal(got[0], want), (name, d, fused, k)
                listed = want >= 0
                assert np.array_equal(got[1][listed].astype(np.float64), np.take_along_axis(D, np.maximum(want, 0), 1)[listed])
                assert (got[1][~listed] == INF).all()
        if rows > nq + 1:
            T = lc.grid_matrix(d, rows, nq, seed, True)
            keys, _ = _topn(l2, idx, T[:nq].copy(), T, tc.NO_BIAS, tc.EMPTY_POOL, rows)
            assert np.array_equal(keys, lc.lists64(lc.dist64(T[:nq], T), lc.admissible(nq, rows), rows)), ("tie", d, fused)


# ------------------------------------------------------------------------------------------------
def _evaluator(train, vali, l2, **modes):
    from buffalo_amd.evaluate import Evaluator
    ev = Evaluator()
    ev.set_score_func("l2" if l2 else "dot")
    for name, v in modes.items():
        ev.set_mode(name, v)
    ev.set_data(train.num_users, train.num_items, train.indptr, train.keys, vali["row"], vali["col"], vali["val"])
    return ev


@pytest.mark.parametrize("d,fused", [(20, 0), (20, 1), (128, 1), (200, 0)])
def test_validation(d, fused):
    """Evaluator under "l2" on the planted training matrix of the dot tests (a user without seen items, one who has seen all but 3,
    duplicate vali pairs) with factors inside the unit ball: lists = the dot twin's with Qb = hb (same counters) and within the tau rule;
    the four metrics and N = the restated metric loop over those lists (1e-12); rmse / error = the float64 sums of the restated float32
    predictions (two float64 sums of n terms in different orders, a division and a root: (2 n + 4) 2^-53 relative); the same from two
    "batch" values and from device buffers."""
    train, vali, _, _, _ = ec.planted(d=d, seed=5 + d)
    P, Q = lc.float_case(d, train.num_users, train.num_items, 600 + d)
    ev, twin = _evaluator(train, vali, True, fused=fused), _evaluator(train, vali, False, fused=fused)
    rows = np.unique(vali["row"])
    D = lc.dist64(P[rows], Q)
    adm = lc.admissible(len(rows), train.num_items, seen=lc.seen_runs(train, rows))
    dP, ld = _device(P)
    dQ, _ = _device(Q)
    n = len(vali["row"])
    want_rmse, want_err = lc.score_metrics(P, Q, vali)
    for topk in (10, 25):
        (got, keys), c1 = _counted(ev, lambda: ev.ranking(P, Q, topk=topk, return_keys=True))
        (_, twin_keys), c2 = _counted(twin, lambda: twin.ranking(P, Q, lc.half_norms(Q), topk=topk, return_keys=True))
        assert np.array_equal(keys, twin_keys) and c1 == c2, (topk, c1, c2)
        bad, share = lc.tau_rule(keys, D, adm, lc.tau(P[rows], Q))
        print("d = %d, fused = %d, topk = %d: largest share of tau %.4f" % (d, fused, topk, share))
        assert not bad, bad[:10]
        want = ec.host_metrics(keys, rows, train, vali, topk)[0]
        for i, name in enumerate(("ndcg", "map", "accuracy", "auc")):
            print(topk, name, got[name], want[i], abs(got[name] - want[i]))
            assert abs(got[name] - want[i]) <= 1e-12, (topk, name, got[name], want[i])
        assert got["N"] == want[4] == len(rows) - 1                                # user 0 has no seen items
        subset = np.ascontiguousarray(rows[::-3], dtype=np.int32)
        for batch in (128, 0):
            ev.set_mode("batch", batch)
            again, keys2 = ev.ranking(P, Q, topk=topk, return_keys=True)
            dev, keys3 = ev.ranking_device(dP.data_ptr(), len(P), dQ.data_ptr(), len(Q), d, ld, topk=topk, return_keys=True)
            assert again == got and dev == got and np.array_equal(keys2, keys) and np.array_equal(keys3, keys), batch
            sub, keys4 = ev.ranking_device(dP.data_ptr(), len(P), dQ.data_ptr(), len(Q), d, ld, rows=subset, topk=topk, return_keys=True)
            assert np.array_equal(keys4, keys[::-3])
            want_sub = ec.host_metrics(keys4, subset, train, vali, topk)[0]
            assert all(abs(sub[name] - want_sub[i]) <= 1e-12 for i, name in enumerate(("ndcg", "map", "accuracy", "auc")))
    sc = ev.scores(P, Q)
    print(d, "rmse", sc["rmse"], want_rmse, "error", sc["error"], want_err)
    tol = (2 * n + 4) * 2.0 ** -53
    assert abs(sc["rmse"] - want_rmse) <= tol * want_rmse and abs(sc["error"] - want_err) <= tol * want_err
    assert ev.scores_device(dP.data_ptr(), len(P), dQ.data_ptr(), len(Q), d, ld) == sc


def test_end_to_end_warp_l2():
    """Train the d = 32 L2 case of tests/test_warp_gpu.py for its 3 epochs through CyWARP, validate straight from the training handle's
    device buffers under "l2": the lists are l2_topn's from the copied-back factors (topk + |seen| candidates, seen items filtered on the
    host).  The ranking metrics under "l2" and under "dot" are printed side by side; which is higher on this toy case is not asserted."""
    import helpers as H
    from buffalo_amd import parallel as par
    from buffalo_amd.backend import CyWARP
    from conftest import tiny_csr, warp_opt
    d, vdim, topk = 32, 32, 10
    csr = tiny_csr(U=48, I=90, density=0.12, seed=17)
    opt = warp_opt(d=d, random_seed=11, num_iters=3, lr=0.05, max_trials=20, threshold=0.5, score_func="l2")
    rng = np.random.default_rng(3)
    P = H.pad(rng.normal(scale=0.4, size=(csr.num_users, d)).astype(np.float32), vdim)
    Q = H.pad(rng.normal(scale=0.4, size=(csr.num_items, d)).astype(np.float32), vdim)
    Qb = np.zeros((csr.num_items, 1), np.float32)
    obj = H.run_hip_sgd(CyWARP, opt, csr, P, Q, Qb, epochs=3, n_chunks=2, modes=dict(chunk=64))
    assert np.linalg.norm(P, axis=1).max() <= 1 + 1e-5 and np.linalg.norm(Q, axis=1).max() <= 1 + 1e-5      # projected into the unit ball
    seen = np.zeros((csr.num_users, csr.num_items), dtype=bool)
    seen[csr.rows(), csr.keys] = True
    vr, vc = np.nonzero(~seen & (rng.random(seen.shape) < 0.03))
    vali = {"row": np.ascontiguousarray(vr, dtype=np.int32), "col": np.ascontiguousarray(vc, dtype=np.int32), "val": np.ones(len(vr), np.float32)}
    rows = np.unique(vali["row"])
    args = (obj.device_buffer("P")[0], csr.num_users, obj.device_buffer("Q")[0], csr.num_items, d, obj.get_vdim())
    ev = _evaluator(csr, vali, True)
    got, keys = ev.ranking_device(*args, topk=topk, return_keys=True)
    Ph, Qh = np.ascontiguousarray(P[:, :d]), np.ascontiguousarray(Q[:, :d])
    cands = ec.old_path_candidates(lambda r, k: tc.run(lambda i, p, q, qb, ok, os_, pl, kk, nt: par.l2_topn(i, p, q, ok, os_, pl, kk), r, Ph, Qh,
                                                       tc.NO_BIAS, tc.EMPTY_POOL, k), csr, rows, topk)
    assert np.array_equal(keys, ec.filtered(cands, csr, rows, topk))
    want = ec.host_metrics(keys, rows, csr, vali, topk)[0]
    assert all(abs(got[name] - want[i]) <= 1e-12 for i, name in enumerate(("ndcg", "map", "accuracy", "auc")))
    sc = ev.scores_device(*args)
    want_rmse, want_err = lc.score_metrics(Ph, Qh, vali)
    tol = (2 * len(vr) + 4) * 2.0 ** -53
    assert abs(sc["rmse"] - want_rmse) <= tol * want_rmse and abs(sc["error"] - want_err) <= tol * want_err
    dot = _evaluator(csr, vali, False).ranking_device(*args, topk=topk)
    for name in ("ndcg", "map", "accuracy", "auc"):
        print("%-8s  l2 %.6f   dot %.6f" % (name, got[name], dot[name]))


def test_refusals():
    from buffalo_amd import parallel as par
    from buffalo_amd._lib import BuffaloHipError
    from buffalo_amd.evaluate import Evaluator
    P, Q = lc.float_case(20, 5, 33, 1)
    idx = np.arange(5, dtype=np.int32)
    bias = np.zeros((33, 1), np.float32)
    eng = par.TopK()
    eng.set_score_func("l2")
    _bind(_seen(5, 33, 7), eng)
    dP, ld = _device(P)
    dQ, _ = _device(Q)
    with pytest.raises(BuffaloHipError, match="no item bias"):
        _topn(eng, idx, P, Q, bias, tc.EMPTY_POOL, 3)
    with pytest.raises(BuffaloHipError, match="no item bias"):
        _unseen(eng, idx, P, Q, bias, tc.EMPTY_POOL, 3)
    with pytest.raises(BuffaloHipError, match="no item bias"):
        eng.dot_topn_device(idx, dP.data_ptr(), 5, dQ.data_ptr(), 33, 20, ld, dQ.data_ptr(), False, *_out(5, 3), tc.EMPTY_POOL, 3)
    with pytest.raises(BuffaloHipError, match="no item bias"):
        eng.recommend_unseen_device(idx, dP.data_ptr(), 5, dQ.data_ptr(), 33, 20, ld, dQ.data_ptr(), *_out(5, 3), tc.EMPTY_POOL, 3)
    st = eng.stats()
    assert st["samples"] == 0 and st["kernel_ms"] == 0 and st["aux_ms"] == 0       # nothing was launched
    for v in (2, -1):
        with pytest.raises(BuffaloHipError, match="score_func must be"):
            eng.set_mode("score_func", v)
    with pytest.raises(ValueError, match="'dot' or 'l2'"):
        eng.set_score_func("cosine")
    keys, scores = _topn(eng, idx, P, Q, tc.NO_BIAS, tc.EMPTY_POOL, 3)             # the handle survives, still in L2 mode
    _distance_bits(keys, scores, P, Q, "after the refusals")
    train, vali, _, _, _ = ec.planted(U=40, I=33, d=20, n_vali=30)
    ev = Evaluator()
    ev.set_data(train.num_users, train.num_items, train.indptr, train.keys, vali["row"], vali["col"], vali["val"])
    Pe, Qe = lc.float_case(20, 40, 33, 2)
    with pytest.raises(BuffaloHipError, match="score_func must be"):
        ev.set_mode("score_func", 2)
    ev.set_score_func("l2")
    with pytest.raises(BuffaloHipError, match="no item bias"):
        ev.ranking(Pe, Qe, bias)
    with pytest.raises(BuffaloHipError, match="no item bias"):
        ev.scores(Pe, Qe, bias)
    assert ev.ranking(Pe, Qe)["N"] > 0


def test_default_mode_keeps_its_bits_after_a_round_trip():
    """The reference's own dot_topn case (tests/parallel/test_base.py) on one handle: before "score_func" = 1, and after 1 and back to 0."""
    from buffalo_amd import parallel as par
    P, Q = tc.unit_factors(60, 12, 1), tc.unit_factors(257, 12, 2)
    Qb = np.random.default_rng(3).normal(scale=0.1, size=(257, 1)).astype(np.float32)
    idx = np.arange(60, dtype=np.int32)
    eng = par.TopK()
    before = _topn(eng, idx, P, Q, Qb, tc.EMPTY_POOL, 10), _similar(eng, idx, Q, tc.EMPTY_POOL, 10)
    eng.set_score_func("l2")
    keys, scores = _topn(eng, idx, P, Q, tc.NO_BIAS, tc.EMPTY_POOL, 10)
    _distance_bits(keys, scores, P, Q, "l2")
    eng.set_score_func("dot")
    after = _topn(eng, idx, P, Q, Qb, tc.EMPTY_POOL, 10), _similar(eng, idx, Q, tc.EMPTY_POOL, 10)
    for a, b in zip(before, after):
        assert np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))
    # the module-level L2 calls run on an engine of their own: the default dot engine is never switched
    want = tc.run(par.dot_topn, idx, P, Q, Qb, tc.EMPTY_POOL, 10)
    k1, s1 = _out(60, 10)
    par.l2_topn(idx, P, Q, k1, s1, tc.EMPTY_POOL, 10)
    assert np.array_equal(k1, keys) and np.array_equal(_bits(s1), _bits(scores))
    k2, s2 = _out(60, 10)
    par.l2_most_similar(idx, Q, k2, s2, tc.EMPTY_POOL, 10)
    _distance_bits(k2, s2, Q[idx], Q, "l2_most_similar")
    _bind(_seen(60, 257, 7), par._l2_engine())
    k3, s3 = _out(60, 10)
    par.l2_recommend_unseen(idx, P, Q, k3, s3, tc.EMPTY_POOL, 10)
    _distance_bits(k3, s3, P, Q, "l2_recommend_unseen")
    got = tc.run(par.dot_topn, idx, P, Q, Qb, tc.EMPTY_POOL, 10)
    assert np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1]))
