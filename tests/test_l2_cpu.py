"""The L2 restatements of tests/l2_cases.py, held to numpy and to the reference's own output, the premise of the exact cases, and the
teeth of the tau rule -- everything the GPU tests of the L2 mode (tests/test_l2_gpu.py) lean on, checked without a GPU."""
import os

import numpy as np
import pytest

import l2_cases as lc

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "l2_vectors.npz")
GRID = ((1, 9, 2, 11), (7, 40, 3, 12), (8, 60, 5, 13), (20, 257, 9, 14), (128, 257, 9, 15), (136, 200, 5, 16), (300, 129, 5, 17))   # d, rows, nq, seed


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("d", lc.DS)
def test_restatement_has_numpys_bits(d):
    rng = np.random.default_rng(700 + d)
    Q = rng.normal(scale=0.5, size=(50, d)).astype(np.float32)
    P = rng.normal(scale=0.5, size=(5, d)).astype(np.float32)
    assert np.array_equal(_bits(lc.half_norms(Q)), _bits(np.float32(-0.5) * (Q ** 2).sum(-1)))
    for p in P:
        want = ((Q - p) ** 2).sum(-1)
        assert want.dtype == np.float32
        assert np.array_equal(_bits(lc.sqdist32(Q, p)), _bits(want))
    rows, cols = rng.integers(0, 5, size=30), rng.integers(0, 50, size=30)
    assert np.array_equal(_bits(lc.predictions32(P, Q, rows, cols)), _bits(1.0 - ((P[rows] - Q[cols]) ** 2).sum(-1)))


@pytest.mark.parametrize("d", lc.DS)
def test_restatement_has_the_references_bits(d):
    """tests/golden/l2_vectors.npz: WARP._get_topk_recommendation / _get_most_similar_L2 / _get_scores with score_func forced to "L2"."""
    g = np.load(GOLDEN)
    assert d in g["ds"].tolist() and int(g["seeds"][g["ds"].tolist().index(d)]) == 9100 + d
    P, Q, rows, cols = lc.golden_input(d)
    D32 = np.stack([lc.sqdist32(Q, p) for p in P])
    assert np.array_equal(_bits(D32), _bits(g["topn_dist_%d" % d]))
    if all(len(np.unique(row)) == Q.shape[0] for row in D32):      # no two float32 distances of a query coincide: the order is the reference's
        assert np.array_equal(g["topn_keys_%d" % d], np.argsort(D32, axis=1, kind="stable")[:, :10])
    for i in range(4):
        keys, dist = g["sim_keys_%d" % d][i], g["sim_dist_%d" % d][i]
        assert keys[0] == i and np.array_equal(_bits(dist), _bits(lc.sqdist32(Q[keys], Q[i])))
    assert np.array_equal(_bits(g["vec_dist_%d" % d]), _bits(lc.sqdist32(Q[g["vec_keys_%d" % d]], P[0])))
    assert np.array_equal(_bits(g["pred_%d" % d]), _bits(lc.predictions32(P, Q, rows, cols)))


@pytest.mark.parametrize("d,rows,nq,seed", GRID)
def test_the_exact_cases_are_exact_and_free_of_ties(d, rows, nq, seed):
    """Coordinates k / 8, |k| <= 8: float32 dots (any order: every partial sum is a multiple of 1 / 64 below 2^18), norms, keys and
    distances equal the float64 ones, and a query's distances to all rows are distinct -- but for the tie a case plants."""
    F = lc.grid_matrix(d, rows, nq, seed)
    assert (np.abs(F * 8) <= 8).all() and np.array_equal(F * 8, np.round(F * 8))
    P = F[:nq]
    F64, P64 = F.astype(np.float64), P.astype(np.float64)
    dots32 = np.stack([(F * p).astype(np.float32).sum(-1, dtype=np.float32) for p in P])
    assert np.array_equal(dots32.astype(np.float64), P64 @ F64.T)
    hb = lc.half_norms(F)
    assert np.array_equal(hb.astype(np.float64), -0.5 * (F64 ** 2).sum(-1))
    keys32 = dots32 + hb
    assert keys32.dtype == np.float32 and np.array_equal(keys32.astype(np.float64), P64 @ F64.T - 0.5 * (F64 ** 2).sum(-1))
    D64 = lc.dist64(P, F)
    for b in range(nq):
        assert np.array_equal(lc.sqdist32(F, P[b]).astype(np.float64), D64[b])
        assert len(np.unique(D64[b])) == rows and D64[b, b] == 0
        # the order of the keys is the order of the distances
        assert np.array_equal(np.argsort(-keys32[b], kind="stable"), np.argsort(D64[b], kind="stable"))
    T = lc.grid_matrix(d, rows, nq, seed, True)
    Dt = lc.dist64(T[:nq], T)
    if rows > nq + 1:
        assert np.array_equal(T[:rows - 1], F[:rows - 1]) and (Dt[:, rows - 1] == Dt[:, nq]).all()
        assert all(len(np.unique(Dt[b])) == rows - 1 for b in range(nq))


def _ranked_by(keys32, k):
    return np.argsort(-keys32, axis=1, kind="stable")[:, :k].astype(np.int32)


@pytest.mark.parametrize("d", [20, 128, 200])
def test_the_tau_rule_has_teeth(d):
    """On a float case the float32 key passes the tau rule; plain dot product, hb without the 1/2 and norms summed over a pitch whose pad
    columns are not zero each break it in most rows."""
    nq, rows, k = 64, 257, 10
    P, Q = lc.float_case(d, nq, rows, 300 + d)
    assert np.linalg.norm(P, axis=1).max() <= 1 and np.linalg.norm(Q, axis=1).max() <= 1 + 2e-3
    D, adm, tau_b = lc.dist64(P, Q), lc.admissible(nq, rows), lc.tau(P, Q)
    dots = P @ Q.T
    assert dots.dtype == np.float32
    bad, share = lc.tau_rule(_ranked_by(dots + lc.half_norms(Q), k), D, adm, tau_b)
    print("d = %d: the float32 key uses %.3f of tau" % (d, share))
    assert not bad
    padded = np.random.default_rng(d).uniform(0.0, 1.0, size=(rows, (d + 7) // 8 * 8 + 8)).astype(np.float32)      # a pitch with 8+ pad columns of garbage
    padded[:, :d] = Q
    for name, keys32 in (("plain dot product", dots), ("hb without the half", dots + 2 * lc.half_norms(Q)),
                         ("norms over the pitch", dots + lc.half_norms(padded))):
        bad, _ = lc.tau_rule(_ranked_by(keys32, k), D, adm, tau_b)
        print("d = %d: %s breaks %d of %d rows" % (d, name, len(bad), nq))
        assert len(bad) > nq // 2, name


def test_the_mixin_validates_by_dot_unless_the_front_says_l2(monkeypatch):
    """DeviceEvaluable.validation_score_func: "dot" by default whatever opt.score_func says (the handle is then not touched); a front that
    sets "l2" gets an evaluator switched to "l2" before the data is bound, and no bias is passed even with use_bias."""
    from buffalo_amd import evaluate
    from buffalo_amd.parallel import _score_func_value
    assert (_score_func_value("dot"), _score_func_value("l2"), _score_func_value("L2")) == (0, 1, 1)
    with pytest.raises(ValueError, match="'dot' or 'l2'"):
        _score_func_value("cosine")

    class Fake:
        calls = []

        def set_score_func(self, name):
            Fake.calls.append(("set_score_func", name))

        def set_data(self, *a):
            Fake.calls.append(("set_data",))

        def ranking(self, P, Q, Qb, rows=None, topk=10):
            Fake.calls.append(("ranking", Qb is not None))
            return {"ndcg": 0.5, "map": 0.25, "accuracy": 0.75, "auc": 0.9, "N": 7.0}

        def scores(self, P, Q, Qb):
            Fake.calls.append(("scores", Qb is not None))
            return {"rmse": 1.5, "error": 1.0}
    monkeypatch.setattr(evaluate, "Evaluator", Fake)

    class Data:
        groups = {"rowwise": {"indptr": np.array([1, 2, 3], np.int64), "key": np.array([0, 1, 0], np.int32)},
                  "vali": {"row": np.array([2, 0, 2], np.int32), "col": np.array([1, 1, 0], np.int32), "val": np.ones(3, np.float32)}}

        def get_header(self):
            return {"num_users": 3, "num_items": 2}

        def get_group(self, name):
            return self.groups[name]

        def has_group(self, name):
            return name in self.groups

    class Opt(dict):
        __getattr__ = dict.get

    class DotFront(evaluate.DeviceEvaluable):
        pass

    class L2Front(evaluate.DeviceEvaluable):
        validation_score_func = "l2"
    assert evaluate.DeviceEvaluable.validation_score_func == "dot"
    for cls, want in ((DotFront, [("set_data",), ("ranking", True), ("scores", True)]),
                      (L2Front, [("set_score_func", "l2"), ("set_data",), ("ranking", False), ("scores", False)])):
        del Fake.calls[:]
        f = cls()
        f.data, f.opt = Data(), Opt(d=4, use_bias=True, score_func="l2", validation={"topk": 5})
        f.P, f.Q, f.Qb = np.zeros((3, 32), np.float32), np.zeros((2, 32), np.float32), np.zeros((2, 1), np.float32)
        assert set(f.get_validation_results()) == {"ndcg", "map", "accuracy", "auc", "rmse", "error"}
        assert Fake.calls == want, cls.__name__
