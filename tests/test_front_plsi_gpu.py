"""pLSI end to end through the buffalo-compatible front (tests/front_harness/buffalo_front/algo/plsi.py): the reference test's options
(tests/algo/test_plsi.py: defaults, d = 20, 10 iterations) on the planted data of tests/test_front_gpu.py.  The yardstick is the SAME front driving
the float64 restatement of tests/ref_plsi.py from the same initial factors, never the device's own output."""
import numpy as np
import pytest

import ref_plsi as R
from test_front_gpu import _data

pytestmark = pytest.mark.gpu


def _front(backend=None, **kw):
    from buffalo_front.algo import plsi as M
    opt = M.PLSIOption().get_default_option()
    opt.update(d=20, num_iters=10, validation={"topk": 10}, random_seed=7)
    opt.update(kw)
    cls = M.PLSI if backend is None else type("PLSIOn" + backend.__name__, (M.PLSI,), {"backend": backend})
    np.random.seed(7)
    m = cls(opt, data_opt=_data())
    m.initialize()
    return m


def test_train_and_validate_against_the_float64_front():
    m = _front()
    P0, Q0 = m.P.copy(), m.Q.copy()
    assert m.P.shape == (m.data.get_header()["num_users"], 20)
    calls = []
    ret = m.train(training_callback=lambda i, metrics: calls.append(i))
    assert calls and "train_loss" in ret and np.isfinite(m.P).all() and np.isfinite(m.Q).all()
    res = m.get_validation_results()

    ref = _front(R.RefPLSI)
    ref.P[:], ref.Q[:] = P0, Q0
    ref.obj.synchronize(False)          # the same start
    ref_ret = ref.train()
    want = ref.get_validation_results()
    print("pLSI on planted data: device ndcg %.4f map %.4f | float64 front ndcg %.4f map %.4f | reference thresholds on ML-100K: ndcg 0.03 map 0.02 (%s)"
          % (res["ndcg"], res["map"], want["ndcg"], want["map"], "reached" if res["ndcg"] > 0.03 and res["map"] > 0.02 else "not reached on this data"))
    assert res["ndcg"] >= 0.9 * want["ndcg"] and res["map"] >= 0.9 * want["map"], (res, want)
    assert res["ndcg"] > 0.015, res      # a random ranking of 300 items scores ndcg@10 ~ 0.015 (tests/test_front_gpu.py)
    print("train_loss after 10 epochs: device %.6f float64 front %.6f" % (ret["train_loss"], ref_ret["train_loss"]))


def test_batched_front_topk_scores_and_save_load(tmp_path):
    from buffalo_front.algo import plsi as M
    m = _front(num_iters=3)
    one = _front(num_iters=3)
    m.batch_rows = 97
    m.train()
    one.train()
    assert m.P.tobytes() == one.P.tobytes() and m.Q.tobytes() == one.Q.tobytes()      # batches do not change the bits
    rows = [0, 5, 17, 499]
    top = m.topk_recommendation(rows, topk=7)
    dense = m.P @ m.Q.T
    for r in rows:
        want = np.argsort(-dense[r], kind="stable")[:7]
        assert sorted(dense[r][top[r]].tolist(), reverse=True) == sorted(dense[r][want].tolist(), reverse=True)
        np.testing.assert_allclose(dense[r][top[r]], dense[r][want], rtol=1e-5)
    pairs = [(0, 3), (7, 200), (499, 299)]
    got = m.get_scores(pairs)
    for (r, c) in pairs:
        assert abs(got[(r, c)] - float(dense[r, c])) <= 1e-6 * abs(dense[r, c]) + 1e-12
    np.testing.assert_allclose(m._get_scores(np.array([0, 7]), np.array([3, 200])), [dense[0, 3], dense[7, 200]], rtol=1e-5)
    path = str(tmp_path / "plsi.bin")
    m.save(path)
    back = M.PLSI.instantiate(M.PLSIOption, path)
    assert back.P.tobytes() == m.P.tobytes() and back.Q.tobytes() == m.Q.tobytes() and back.opt.d == 20
    q = m.Q.copy()
    m.normalize("item")
    np.testing.assert_allclose(m.Q, q / (q.sum(axis=0, keepdims=True) + 1e-10), rtol=1e-6)


def test_overwritten_rows_are_what_the_next_epoch_trains_from():
    """inherit() writes rows of a previous model into P / Q after initialize_model; synchronize(False) takes them to the device."""
    m = _front()
    before = (m.P.copy(), m.Q.copy())
    rng = np.random.default_rng(3)
    newP, newQ = R.init_model(m.P.shape[0], m.Q.shape[0], 20, seed=99)
    up, uq = rng.choice(m.P.shape[0], 50, replace=False), rng.choice(m.Q.shape[0], 40, replace=False)
    m.P[up], m.Q[uq] = newP[up], newQ[uq]
    m.obj.synchronize(False)
    P0, Q0 = m.P.copy(), m.Q.copy()
    m._iterate()
    from buffalo_amd.synth import CSR
    g = m.data.get_group("rowwise")
    csr = CSR(m.P.shape[0], m.Q.shape[0], g["indptr"][:], g["key"][:], g["val"][:])
    P64, Q64, _ = R.epoch(P0, Q0, csr, 1.0, 1.0, np.float64)
    n_row, n_col = R.entry_counts(csr)
    assert (np.abs(m.P - P64) <= P64 * R.bound_normalized(n_row, 20, 20)[:, None]).all()
    assert (np.abs(m.Q - Q64) <= Q64 * R.bound_normalized(n_col, 20, m.Q.shape[0])[:, None]).all()
    # and NOT what the epoch from the untouched start gives
    assert np.abs(m.P - P64).max() < 1e-3 * np.abs(m.P - R.epoch(before[0], before[1], csr, 1.0, 1.0, np.float64)[0]).max()
