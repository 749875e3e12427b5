"""The validation evaluator (`bfh_eval_*`, buffalo_amd/evaluate.py) on the device: seen-aware top-k + NDCG / MAP / accuracy / AUC /
RMSE / error of evaluate/base.py:44-148, against the reference's golden values, against the old path (dot_topn of topk + |seen|
candidates, filtered and walked on the host by the unmodified front-harness `Evaluable`) and against itself (device buffers,
batching, repeat runs)."""
import json
import os
import sys

import numpy as np
import pytest

import eval_cases as ec
import helpers as H
import topk_cases as tc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
RANK = ("ndcg", "map", "accuracy", "auc")


def _evaluator(train, vali):
    from buffalo_amd.evaluate import Evaluator
    ev = Evaluator()
    ev.set_data(train.num_users, train.num_items, train.indptr, train.keys, vali["row"], vali["col"], vali["val"])
    return ev


def _old_engine():
    from buffalo_amd.parallel import TopK
    eng = TopK()
    eng.set_mode("flt_min_rule", 0)
    return eng


def _harness_model(train, vali, P, Q, Qb, topk, cands):
    """The unmodified front-harness Evaluable over a data object, fed the old path's candidate lists."""
    from buffalo_front.algo.base import Algo, Evaluable
    from buffalo_front.data import Data, MatrixMarketOptions
    from buffalo_front.misc import Option

    class Model(Algo, Evaluable):
        def _get_topk_recommendation(self, rows, topk, pool=None):
            return [(int(r), cands[int(r)][0]) for r in rows]

        def _get_scores(self, row, col):      # bpr.py / warp.py: the SGD fronts add the item bias
            s = (self.P[row] * self.Q[col]).sum(axis=1)
            return s + self.Qb[col, 0] if self.Qb is not None else s

    data = Data(MatrixMarketOptions().get_default_option())
    data.groups = {"rowwise": {"indptr": train.indptr, "key": train.keys, "val": train.vals}, "vali": vali}
    data.header = {"num_nnz": train.nnz, "num_users": train.num_users, "num_items": train.num_items, "completed": 1}
    m = Model()
    m.data, m.P, m.Q, m.Qb = data, P, Q, Qb
    m.opt = Option({"d": P.shape[1], "use_bias": Qb is not None, "validation": {"topk": topk, "batch": 64}})
    return m


def test_reference_golden_metrics():
    """metrics_case() (60 x 40, d = 20) reproduces the values the reference's own Evaluable produced: ranking metrics within 1e-12
    (same integer hit positions -- the smallest score gap of a user is 5.7e-4, the fp32 dot error at most 1e-4 -- so only the float64
    rounding of a mean over <= 60 users differs), rmse / error within (n_vali + d + 2) 2^-24 relative (the golden sums ran in float32)."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_front_traces as G
    golden = json.load(open(G.OUT))["validation_metrics"]
    U, I, rows, cols, vals, vali, P, Q = G.metrics_case()
    train = ec.csr_of(U, I, rows, cols)
    ev = _evaluator(train, vali)
    sc = ev.scores(P, Q)
    tol = (len(vali["row"]) + 20 + 2) * 2.0 ** -24
    for topk in (10, 25):
        want = golden["topk%d" % topk]
        got = ev.ranking(P, Q, topk=topk)
        for k in RANK:
            print(topk, k, got[k], want[k], abs(got[k] - want[k]))
        for k in ("rmse", "error"):
            print(topk, k, sc[k], want[k], abs(sc[k] - want[k]) / want[k])
        for k in RANK:
            assert abs(got[k] - want[k]) <= 1e-12, (topk, k, got[k], want[k])
        for k in ("rmse", "error"):
            assert abs(sc[k] - want[k]) <= tol * abs(want[k]), (k, sc[k], want[k])


@pytest.mark.parametrize("d,bias", [(20, False), (20, True), (128, False), (128, True), (200, False), (200, True)])
def test_lists_and_metrics_match_the_old_path(d, bias):
    """Planted input (a user without seen items: skipped; a user who has seen all but 3 items: padded list, topk > unseen items;
    duplicate vali pairs) at topk 10 and 25, all validation users and an explicit subset: the lists equal the dot_topn lists of
    topk + |seen_u| candidates with the seen items filtered out, the metrics equal the unmodified harness Evaluable fed those lists."""
    train, vali, P, Q, Qb = ec.planted(d=d, bias=bias, seed=5 + d)
    ev = _evaluator(train, vali)
    eng = _old_engine()
    qb = Qb if bias else tc.NO_BIAS

    def dot_topn(rows, k):
        return tc.run(lambda *a: eng.dot_topn(*a[:8]), rows, P, Q, qb, tc.EMPTY_POOL, k)
    all_rows = np.unique(vali["row"])
    assert ev.num_rows() == len(all_rows) and 0 in all_rows and 1 in all_rows
    subset = np.ascontiguousarray(all_rows[::-3], dtype=np.int32)
    for topk in (10, 25):
        cands = ec.old_path_candidates(dot_topn, train, all_rows, topk)
        model = _harness_model(train, vali, P, Q, Qb, topk, cands)
        for rows in (None, subset):
            got, keys = ev.ranking(P, Q, Qb, rows=rows, topk=topk, return_keys=True)
            use = all_rows if rows is None else rows
            want_keys = ec.filtered(cands, train, use, topk)
            assert np.array_equal(keys, want_keys), (topk, np.flatnonzero((keys != want_keys).any(axis=1))[:10])
            if rows is None:
                want = model._evaluate_ranking_metrics(topk)
                assert got["N"] == len(all_rows) - 1                   # user 0 has no seen items
            else:
                want = dict(zip(RANK, ec.host_metrics(want_keys, use, train, vali, topk)[0]))
            for k in RANK:
                print(d, bias, topk, "all" if rows is None else "subset", k, got[k], want[k], abs(got[k] - want[k]))
                assert abs(got[k] - want[k]) <= 1e-12, (topk, k, got[k], want[k])
        i1 = int(np.flatnonzero(all_rows == 1)[0])
        _, keys = ev.ranking(P, Q, Qb, topk=topk, return_keys=True)
        assert (keys[i1, :3] >= 0).all() and (keys[i1, 3:] == -1).all()     # 3 unseen items, then padding
    want = model._evaluate_score_metrics()
    got = ev.scores(P, Q, Qb)
    tol = (len(vali["row"]) + d + 2) * 2.0 ** -24
    for k in ("rmse", "error"):
        print(d, bias, k, got[k], float(want[k]), abs(got[k] - want[k]) / want[k])
        assert abs(got[k] - want[k]) <= tol * abs(want[k]), (k, got[k], want[k])


def test_synth_input_matches_the_old_path():
    """synth.generate shape (Zipf items, log-normal degrees), one held-out entry per user with two or more."""
    from buffalo_amd import synth
    full = synth.generate(700, 900, 30000, seed=3)
    train, vali = ec.hold_out(full, seed=1)
    rng = np.random.default_rng(2)
    P = rng.normal(size=(700, 64)).astype(np.float32)
    Q = rng.normal(size=(900, 64)).astype(np.float32)
    ev, eng = _evaluator(train, vali), _old_engine()
    rows = np.unique(vali["row"])
    cands = ec.old_path_candidates(lambda r, k: tc.run(lambda *a: eng.dot_topn(*a[:8]), r, P, Q, tc.NO_BIAS, tc.EMPTY_POOL, k), train, rows, 10)
    got, keys = ev.ranking(P, Q, topk=10, return_keys=True)
    assert np.array_equal(keys, ec.filtered(cands, train, rows, 10))
    want = _harness_model(train, vali, P, Q, None, 10, cands)._evaluate_ranking_metrics(10)
    for k in RANK:
        assert abs(got[k] - want[k]) <= 1e-12, (k, got[k], want[k])


def test_device_buffers_of_a_training_handle_give_the_host_form_bits():
    """After three BPRMF epochs: ranking / scores from the handle's P / Q / Qb in HBM == the host forms on the synchronised arrays,
    bit for bit in all seven doubles (and in the lists)."""
    from conftest import bpr_opt
    from buffalo_amd.backend import CyBPR
    train, vali, P0, Q0, Qb = ec.planted(U=200, I=300, d=20, bias=True, seed=9)
    d, vdim = 20, 32
    P, Q = H.pad(0.1 * P0, vdim), H.pad(0.1 * Q0, vdim)
    Qb = np.ascontiguousarray(0.1 * Qb)
    obj = H.run_hip_sgd(CyBPR, bpr_opt(d=d, lr=0.05, num_iters=3), train, P, Q, Qb, epochs=3)
    ev = _evaluator(train, vali)
    dev, dkeys = ev.ranking_device(obj.device_buffer("P")[0], 200, obj.device_buffer("Q")[0], 300, d, vdim, obj.device_buffer("Qb")[0],
                                   topk=10, return_keys=True)
    dsc = ev.scores_device(obj.device_buffer("P")[0], 200, obj.device_buffer("Q")[0], 300, d, vdim, obj.device_buffer("Qb")[0])
    hP, hQ = np.ascontiguousarray(P[:, :d]), np.ascontiguousarray(Q[:, :d])
    host, hkeys = ev.ranking(hP, hQ, Qb, topk=10, return_keys=True)
    hsc = ev.scores(hP, hQ, Qb)
    assert np.array_equal(dkeys, hkeys)
    assert host["N"] > 100 and host["ndcg"] > 0
    for k in RANK + ("N",):
        assert dev[k] == host[k], (k, dev[k], host[k])
    for k in ("rmse", "error"):
        assert dsc[k] == hsc[k] and hsc[k] > 0, (k, dsc[k], hsc[k])


def test_results_do_not_depend_on_runs_or_batching():
    train, vali, P, Q, Qb = ec.planted(d=128, bias=True, seed=4)
    ev = _evaluator(train, vali)
    base, base_keys = ev.ranking(P, Q, Qb, topk=10, return_keys=True)
    base_sc = ev.scores(P, Q, Qb)
    for batch in (0, 7, 128, 256):
        ev.set_mode("batch", batch)
        got, keys = ev.ranking(P, Q, Qb, topk=10, return_keys=True)
        assert got == base and np.array_equal(keys, base_keys), batch
        assert ev.scores(P, Q, Qb) == base_sc
    other = _evaluator(train, vali)                      # a second handle, multi-pass selection only
    other.set_mode("fast_select", 0)
    got, keys = other.ranking(P, Q, Qb, topk=10, return_keys=True)
    assert got == base and np.array_equal(keys, base_keys)
    st = ev.stats()
    assert st["kernel_ms"] > 0 and st["optimizer_ms"] > 0 and st["launches"] == 5
    ev.reset_stats()
    assert ev.stats()["launches"] == 0


def test_empty_and_uncounted_inputs_are_not_errors():
    train, vali, P, Q, _ = ec.planted(d=20, seed=6)
    none = {"row": np.zeros(0, np.int32), "col": np.zeros(0, np.int32), "val": np.zeros(0, np.float32)}
    ev = _evaluator(train, none)
    assert ev.num_rows() == 0
    assert ev.ranking(P, Q, topk=10) == dict(ndcg=0.0, map=0.0, accuracy=0.0, auc=0.0, N=0.0)
    assert ev.scores(P, Q) == {"rmse": 0.0, "error": 0.0}
    ev = _evaluator(train, vali)
    got = ev.ranking(P, Q, rows=np.array([0], np.int32), topk=10)       # the only row has no seen items: N == 0
    assert got == dict(ndcg=0.0, map=0.0, accuracy=0.0, auc=0.0, N=0.0)


def test_bad_arguments_are_refused_with_a_message():
    import torch
    from buffalo_amd._lib import BuffaloHipError
    from buffalo_amd.evaluate import Evaluator
    train, vali, P, Q, _ = ec.planted(d=24, seed=8)
    U, I = train.num_users, train.num_items
    ev = Evaluator()
    with pytest.raises(BuffaloHipError, match="set_data has not been called"):
        ev.ranking(P, Q, topk=10)
    bad = train.keys.copy()
    bad[5] = I
    with pytest.raises(BuffaloHipError, match="training key outside"):
        ev.set_data(U, I, train.indptr, bad, vali["row"], vali["col"], vali["val"])
    bad = vali["col"].copy()
    bad[3] = -1
    with pytest.raises(BuffaloHipError, match="vali col outside"):
        ev.set_data(U, I, train.indptr, train.keys, vali["row"], bad, vali["val"])
    bad = vali["row"].copy()
    bad[0] = U
    with pytest.raises(BuffaloHipError, match="vali row outside"):
        ev.set_data(U, I, train.indptr, train.keys, bad, vali["col"], vali["val"])
    bad = train.indptr.copy()
    bad[-1] += 1
    with pytest.raises(BuffaloHipError, match="END offsets"):
        ev.set_data(U, I, bad, train.keys, vali["row"], vali["col"], vali["val"])
    ev.set_data(U, I, train.indptr, train.keys, vali["row"], vali["col"], vali["val"])     # the handle survives
    for topk in (0, -3, 16385):
        with pytest.raises(BuffaloHipError, match="topk must be in"):
            ev.ranking(P, Q, topk=topk)
    with pytest.raises(BuffaloHipError, match="row outside"):
        ev.ranking(P, Q, rows=np.array([0, U], np.int32), topk=10)
    with pytest.raises(BuffaloHipError, match="one row per item"):
        ev.ranking(P, Q[:-1].copy(), topk=10)
    with pytest.raises(BuffaloHipError, match="same number of columns"):
        ev.scores(P, np.ascontiguousarray(Q[:, :16]))
    dP, dQ = torch.from_numpy(P).cuda(), torch.from_numpy(Q).cuda()
    for d, ld in ((24, 20), (24, 28), (32, 24)):                          # ld < d, ld % 8 != 0, d > ld
        with pytest.raises(BuffaloHipError, match="leading dimension"):
            ev.ranking_device(dP.data_ptr(), U, dQ.data_ptr(), I, d, ld, topk=10)
        with pytest.raises(BuffaloHipError, match="leading dimension"):
            ev.scores_device(dP.data_ptr(), U, dQ.data_ptr(), I, d, ld)
    with pytest.raises(BuffaloHipError, match="unknown mode"):
        ev.set_mode("no_such_knob", 1)
    assert ev.ranking_device(dP.data_ptr(), U, dQ.data_ptr(), I, 24, 24, topk=10) == ev.ranking(P, Q, topk=10)


def test_mixin_returns_the_reference_keys():
    """DeviceEvaluable in front of the harness Evaluable: the reference's dict, equal to the harness's own host evaluation."""
    from buffalo_amd.evaluate import DeviceEvaluable
    train, vali, P, Q, Qb = ec.planted(d=20, bias=True, seed=12)
    eng = _old_engine()
    rows = np.unique(vali["row"])
    cands = ec.old_path_candidates(lambda r, k: tc.run(lambda *a: eng.dot_topn(*a[:8]), r, P, Q, Qb, tc.EMPTY_POOL, k), train, rows, 10)
    host = _harness_model(train, vali, P, Q, Qb, 10, cands)
    want = host.get_validation_results()

    class Front(DeviceEvaluable, type(host)):
        pass
    front = Front()
    front.data, front.opt, front.P, front.Q, front.Qb = host.data, host.opt, P, Q, Qb
    got = front.get_validation_results()
    assert list(got) == ["ndcg", "map", "accuracy", "auc", "rmse", "error"]
    for k in RANK:
        assert abs(got[k] - want[k]) <= 1e-12, (k, got[k], want[k])
    tol = (len(vali["row"]) + 20 + 2) * 2.0 ** -24
    for k in ("rmse", "error"):
        assert abs(got[k] - want[k]) <= tol * abs(want[k])
    front.opt.validation["eval_samples"] = 50
    np.random.seed(3)
    sampled = front._evaluate_ranking_metrics()
    assert 0 < sampled["ndcg"] <= 1 and sampled != {k: got[k] for k in RANK}
