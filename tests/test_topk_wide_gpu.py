"""The fused sweep for 128 < d <= 256 (csrc/topk_kernels.hpp: topk_scores_wide_kernel): both K-chunks in one accumulator must end on the
bits the dense path's two launches produce, and the filter epilogue behind them must keep, drop and overflow as at d <= 128."""
import functools
import numpy as np
import pytest

import topk_cases as tc
import topk_planted as tp

pytestmark = pytest.mark.gpu
COLS, K = tp.FUSED_COLS, 10


def _engine(**modes):
    from buffalo_amd import parallel as par
    eng = par.TopK()
    for name, v in modes.items():
        eng.set_mode(name, v)
    return eng


def _dot_topn(eng, idx, P, Q, Qb=tc.NO_BIAS, k=K):
    return tc.run(lambda *a: eng.dot_topn(*a[:8]), idx, P, Q, Qb, tc.EMPTY_POOL, k)


def _same(got, want, what):
    assert np.array_equal(got[0], want[0]) and np.array_equal(tp.bits(got[1]), tp.bits(want[1])), what


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("nq", [1, 33, 129])
@pytest.mark.parametrize("d", [136, 192, 200, 248, 256])
def test_planted_columns(oracle, d, nq, bias):
    """Each query its own factor column, 127 / 128 and chunk 1's half-wave split among them (tp.plant_columns).  d = 136: one float4 per half
    of chunk 1; 200: nv1 = 9, one float4 into the second pipeline half; 256: the straight-line instance; nq = 129: a wave with 31 absent rows."""
    S, idx, P, Q = tp.score_case(d, nq)
    Qb = tp.some_bias(S.shape[1]) if bias else tc.NO_BIAS
    got = _dot_topn(_engine(fused=1), idx, P, Q, Qb)
    _same(got, tc.run(oracle.dot_topn, idx, P, Q, Qb, tc.EMPTY_POOL, K), (d, nq, "oracle"))
    _same(got, tp.spec_scores(S + Qb.T if bias else S, K), (d, nq, "spec"))


def test_the_sweep_ran_and_overflow_rows_come_back(oracle):
    """d = 256, a 32-column sample.  Rows 0, 3, 6, ...: the sample lies below every other score, so all 6,144 swept columns pass and the
    768-column segments overflow their 512 slots (-> the dense redo); the others: the sample lies above everything, the sweep keeps
    nothing.  `merges` counts exactly the planted overflow rows -- a dense plan (what d > 128 got before this kernel) counts none."""
    rng, nq = np.random.default_rng(31), 40
    over = np.arange(nq) % 3 == 0
    S = np.stack([tp.distinct(rng, COLS, tp.WORSE) for _ in range(nq)])
    for r in range(nq):
        S[r, :32] = tp.distinct(rng, 32, (0x3D000000, 0x3E000000) if over[r] else tp.BETTER)
    assert all(tp.fused_predict(S[r], "c0_32")[0] == over[r] for r in range(nq))
    planted = tp.planted(S, 256, cols_at=np.arange(nq) * 7 % 256)      # plants in both chunks and both halves of each
    eng = _engine(fused=1, fused_c0=32)
    got = _dot_topn(eng, *planted)
    _same(got, _dot_topn(_engine(fused=0), *planted), "dense engine")
    _same(got, tp.spec_scores(S, K), "spec")
    assert eng.stats()["merges"] == over.sum() and 0 < over.sum() < nq


@functools.lru_cache(maxsize=None)
def _dense_data(d, n=129, cols=COLS):
    """Random normal factors and a 5 % training matrix (user 1: nearly everything seen)."""
    rng = np.random.default_rng(100 + d)
    P, Q = rng.standard_normal((n, d), dtype=np.float32), rng.standard_normal((cols, d), dtype=np.float32)
    M = rng.integers(0, 20, size=(n, cols), dtype=np.uint8) == 0
    M[1, 3:] = True
    return P, Q, M


@pytest.mark.parametrize("d,via", [(136, "dot"), (200, "dot"), (256, "dot"), (256, "unseen"), (256, "unseen_auto"), (256, "l2"), (256, "eval")])
def test_dense_data_through_both_chunks(d, via):
    """fused = 1 (sample by rule) against fused = 0 on random factors: keys and score bits identical -- through dot_topn, and at d = 256
    through recommend_unseen, the L2 mode (hb rides as the bias) and the validation ranking (seen-aware instances).  A forced
    recommend_unseen fuses up to d = 128 only; `unseen_auto` is the call the default rule fuses, 8,192 x 8,192: user 1 comes back (merges).
    Bound of a listed dot score against the float64 product: the fp32 sum of d terms applies at most d roundings to any term (one for
    its product, at most d - 1 for the additions it passes through), each of relative size u = 2^-24, so
    |fl(sum) - sum| <= ((1 + u)^d - 1) sum_c |p_c q_c| = d * 2^-24 * sum_c |p_c q_c| to first order, in ANY summation order."""
    P, Q, M = _dense_data(d, 8192, 8192) if via == "unseen_auto" else _dense_data(d)
    idx = np.arange(len(P), dtype=np.int32)
    if via == "eval":
        from buffalo_amd.evaluate import Evaluator
        out = []
        for fused, ev in ((1, Evaluator()), (0, Evaluator())):
            ev.set_data(len(P), COLS, *tp.csr_of_seen(M), idx, np.argmin(M, axis=1).astype(np.int32), np.ones(len(P), np.float32))
            ev.set_mode("fused", fused)
            out.append(ev.ranking(P, Q, topk=K, return_keys=True))
        assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1])
        return
    got = []
    for fused in (-1 if via == "unseen_auto" else 1, 0):
        eng = _engine(fused=fused)
        if via == "l2":
            eng.set_score_func("l2")
        if via.startswith("unseen"):
            eng.set_seen(*tp.csr_of_seen(M), Q.shape[0])
            got.append(tc.run(lambda *a: eng.recommend_unseen(*a[:8]), idx, P, Q, tc.NO_BIAS, tc.EMPTY_POOL, K))
        else:
            got.append(_dot_topn(eng, idx, P, Q))
        merges = eng.stats()["merges"]
        assert merges == 0 or fused                     # the dense engine hands nothing back
        assert merges < len(P)                          # fused: the sweep itself produced rows
        assert merges >= 1 or not (via == "unseen_auto" and fused)      # user 1 is handed back, which only a fused run does
    _same(got[0], got[1], (d, via))
    if via == "dot":
        keys, scores = got[0]
        p64, q64 = P.astype(np.float64)[:, None, :], Q.astype(np.float64)[keys]
        err = np.abs(scores - (p64 * q64).sum(-1))
        bound = d * 2.0 ** -24 * np.abs(p64 * q64).sum(-1)
        print("d = %d: largest error / bound = %.3f" % (d, (err / bound).max()))
        assert (keys >= 0).all() and (err <= bound).all()
