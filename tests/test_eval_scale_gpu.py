"""The validation evaluator at the ML-20M shape (138,493 x 27,278, 20 M entries, one held-out entry per user, d = 128) against the
old path: dot_topn_device of topk + max |seen| candidates per batch of users (users sorted by history length), filtered on the host.

A row's list may differ from the old path's only where the old path's own scores prove a tie: every differing position holds a score
that another candidate of that row shares bit for bit (the kept set of a tie at a selection boundary depends on how many candidates
were asked for).  At most 1 % of the rows may differ; the count is printed.  (Recorded in profiles/eval_first_contact.txt: the
CPU pre-check of the cap, `scripts/run_eval.py mode=precheck` -- numpy fp32 scores of 4096 users of this input, 0 rows with a tie -- and
this test on an MI355X: 0 differing rows of 138,488.)"""
import numpy as np
import pytest

import eval_cases as ec
import topk_cases as tc

pytestmark = pytest.mark.gpu

TOPK = 10


def _old_path_lists(eng, dP, dQ, U, I, d, train, rows):
    """Filtered lists [n, TOPK] of the old path + per row whether a score at position p has a bit-equal twin among the row's candidates."""
    beg = np.concatenate([[0], train.indptr[:-1]])
    deg = (train.indptr - beg)[rows]
    order = np.argsort(deg, kind="stable")
    seen_global = train.rows().astype(np.int64) * I + train.keys          # ascending: the CSR is sorted by (row, key)
    lists = np.empty((len(rows), TOPK), np.int32)
    tied = np.zeros((len(rows), TOPK), bool)
    for a in range(0, len(rows), 4096):
        sel = order[a:a + 4096]
        batch = np.ascontiguousarray(rows[sel], dtype=np.int32)
        need = int(min(TOPK + deg[sel].max(), I))
        keys, scores = np.empty((len(batch), need), np.int32), np.empty((len(batch), need), np.float32)
        eng.dot_topn_device(batch, dP, U, dQ, I, d, d, None, False, keys, scores, tc.EMPTY_POOL, need)
        q = batch.astype(np.int64)[:, None] * I + keys
        pos = np.minimum(np.searchsorted(seen_global, q), len(seen_global) - 1)
        seen = seen_global[pos] == q
        first = np.argsort(seen, axis=1, kind="stable")[:, :TOPK]          # the first TOPK unseen candidates, in list order
        assert not np.take_along_axis(seen, first, axis=1).any()
        lists[sel] = np.take_along_axis(keys, first, axis=1)
        s = np.take_along_axis(scores, first, axis=1)
        bits = scores.view(np.int32)
        twin = np.zeros(bits.shape, bool)                                  # lists are sorted by score: twins are neighbours
        eq = bits[:, 1:] == bits[:, :-1]
        twin[:, 1:] |= eq
        twin[:, :-1] |= eq
        twin[:, -1] = True                                                 # the last candidate: its twin may be the one that was cut
        tied[sel] = np.take_along_axis(twin, first, axis=1)
        del s
    return lists, tied


def test_ml20m_shape_lists_and_metrics_match_the_old_path():
    import torch
    from buffalo_amd import synth
    from buffalo_amd.evaluate import Evaluator
    from buffalo_amd.parallel import TopK
    U, I, nnz = synth.SHAPES["ml20m"]
    train, vali = ec.hold_out(synth.generate(U, I, nnz, seed=7), seed=11)
    d = 128
    rng = np.random.default_rng(20)
    P = (0.5 * rng.standard_normal((U, d), dtype=np.float32))
    Q = (0.5 * rng.standard_normal((I, d), dtype=np.float32))
    tP, tQ = torch.from_numpy(P).cuda(), torch.from_numpy(Q).cuda()
    ev = Evaluator()
    ev.set_data(U, I, train.indptr, train.keys, vali["row"], vali["col"], vali["val"])
    rows = np.unique(vali["row"])
    got, keys = ev.ranking_device(tP.data_ptr(), U, tQ.data_ptr(), I, d, d, topk=TOPK, return_keys=True)
    again, keys2 = ev.ranking_device(tP.data_ptr(), U, tQ.data_ptr(), I, d, d, topk=TOPK, return_keys=True)
    assert got == again and np.array_equal(keys, keys2)
    eng = TopK()
    eng.set_mode("flt_min_rule", 0)
    want_keys, tied = _old_path_lists(eng, tP.data_ptr(), tQ.data_ptr(), U, I, d, train, rows)
    differ = keys != want_keys
    bad_rows = np.flatnonzero(differ.any(axis=1))
    print("rows whose list differs from the old path's: %d of %d" % (len(bad_rows), len(rows)))
    assert not (differ & ~tied).any(), "lists differ where the old path's scores show no tie: rows %s" % rows[np.flatnonzero((differ & ~tied).any(axis=1))[:10]]
    assert len(bad_rows) <= 0.01 * len(rows)
    want, _ = ec.host_metrics(want_keys, rows, train, vali, TOPK)
    own, _ = ec.host_metrics(keys, rows, train, vali, TOPK)
    assert got["N"] == want[4] == len(rows)
    for i, k in enumerate(("ndcg", "map", "accuracy", "auc")):
        print(k, got[k], want[i], abs(got[k] - want[i]), abs(got[k] - own[i]))
        assert abs(got[k] - own[i]) <= 1e-12, (k, got[k], own[i])                               # the host loop over the device's own lists
        assert abs(got[k] - want[i]) <= 1e-12 + len(bad_rows) / len(rows), (k, got[k], want[i])   # a proven-tie row moves a mean by at most 1 / N
    sc = ev.scores_device(tP.data_ptr(), U, tQ.data_ptr(), I, d, d)
    p64, q64 = P[vali["row"]].astype(np.float64), Q[vali["col"]].astype(np.float64)
    err = np.einsum("ij,ij->i", p64, q64) - vali["val"]
    # an fp32 dot of d terms and the fp32 subtraction are off by at most (d + 2) 2^-24 (sum |p||q| + |val|) per triple; the sums run in
    # float64 on both sides, and a norm moves by at most the norm of the change
    bound = (d + 2) * 2.0 ** -24 * (np.einsum("ij,ij->i", np.abs(p64), np.abs(q64)) + np.abs(vali["val"]))
    print("rmse", sc["rmse"], np.sqrt((err ** 2).mean()), "error", sc["error"], np.abs(err).mean())
    assert abs(sc["error"] - np.abs(err).mean()) <= bound.mean()
    assert abs(sc["rmse"] - np.sqrt((err ** 2).mean())) <= np.sqrt((bound ** 2).mean())
