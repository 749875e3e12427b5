"""bfh_als_fold_in under "als_fold_solve" = 2 (als_fold_wide_kernel: Gramian and Cholesky of a history fused in one block, vdim <= 256): the
row-length edges of als_cases.pattern() inside the fold-in envelope at 128 < d <= 256 and below, every row -- the ones above 4,096 entries
included -- to the same bits whatever its batch, a training run that does not notice the calls, and top-k from the folded rows at d = 256.

The rows folded are 0 .. N_LONG - 1 of pattern() (they carry every length edge), against the full 8,300-row factor."""
import functools

import numpy as np
import pytest

import als_cases as AC
import fold_in_cases as FC
import helpers as H

pytestmark = pytest.mark.gpu

N = AC.N_LONG
WIDE = {"als_fold_solve": 2}


@functools.lru_cache(maxsize=None)
def references(d, adaptive, axis):
    """(float32 comparison run, float64 yardstick) of the N rows, [N, d] each, computed once per process."""
    case = AC.pattern()
    Y = AC.start(case, d)[1 - axis]
    m = case.mat(axis)
    out = FC.fold_f32(m, Y, axis, adaptive, rows=range(N))[:N], FC.fold_f64(m, Y, axis, adaptive, rows=range(N))[:N]
    for a in out:
        a.setflags(write=False)
    return out


def fold(obj, m, axis, rows):
    """The histories `rows` of `m`, in that order, as one fold_in call -> [len(rows), vdim]."""
    bounds = [FC.rows_of(m)[r] for r in rows]
    take = np.concatenate([np.arange(b, e) for b, e in bounds] + [np.zeros(0, np.int64)]).astype(np.int64)
    indptr = np.cumsum([e - b for b, e in bounds], dtype=np.int64)
    return obj.fold_in(axis, indptr, np.ascontiguousarray(m.keys[take]), np.ascontiguousarray(m.vals[take]))


@pytest.mark.parametrize("d, adaptive, axis", [(160, False, 0), (192, True, 0), (256, False, 0), (130, False, 0), (200, False, 1), (128, False, 0),
                                               (40, True, 0)])
def test_row_length_edges(d, adaptive, axis):
    cmp_run, f64 = references(d, adaptive, axis)
    case = AC.pattern()
    obj = FC.make_hip(d, adaptive, WIDE)
    FC.bind(obj, case, d)
    X = fold(obj, case.mat(axis), axis, range(N))
    assert X.shape == (N, AC.vdim_of(d)) and np.isfinite(X).all()
    assert not X[0].any()                       # the empty history
    assert not X[:, d:].any()                   # the padding columns
    FC.hold("fold_in d=%d%s axis %d als_fold_solve=2" % (d, " adaptive_reg" if adaptive else "", axis), X[:, :d], cmp_run, f64)


def test_a_row_does_not_depend_on_its_batch():
    d, case = 192, AC.pattern()
    m = case.csr
    assert (AC.lengths_of(m)[:N] > AC.HEAVY).sum() == 3
    obj = FC.make_hip(d, modes=WIDE)
    FC.bind(obj, case, d)
    whole = fold(obj, m, 0, range(N))
    chunked = np.concatenate([fold(obj, m, 0, range(a, b)) for a, b in ((0, 14), (14, 14), (14, N))])
    back = fold(obj, m, 0, range(N - 1, -1, -1))[::-1]
    again = fold(obj, m, 0, range(N))
    assert whole.any()
    for name, other in (("chunked calls", chunked), ("reversed order", back), ("a second run", again)):
        assert np.array_equal(whole.view(np.uint32), other.view(np.uint32)), name


def _training(d, with_folds):
    """One user half-epoch, then the item half-epoch in two calls -- with mode-2 fold_in calls on both axes in between, or without."""
    case = AC.tiny(31)
    obj = FC.make_hip(d, modes=WIDE)
    P, Q = (H.pad(x.copy(), AC.vdim_of(d)) for x in AC.start(case, d))
    AC.bind(obj, case, P, Q, True)
    obj.precompute(0)
    loss = [obj.partial_update(0, case.users, case.csr.indptr, case.csr.keys, case.csr.vals, 0)]
    plans, folds = [AC.plan_of(obj)], []
    obj.precompute(1)
    mid = case.items // 2
    for a, b in ((0, mid), (mid, case.items)):
        if with_folds:
            folds.append(obj.fold_in(0, case.csr.indptr, case.csr.keys, case.csr.vals))
            folds.append(obj.fold_in(1, case.t.indptr, case.t.keys, case.t.vals))
        loss.append(obj.partial_update(a, b, case.t.indptr, *AC.chunk(case.t, a, b), 1))
        plans.append(AC.plan_of(obj))
    return P, Q, loss, plans, folds


def test_training_is_not_disturbed():
    P0, Q0, loss0, plans0, _ = _training(160, False)
    P1, Q1, loss1, plans1, folds = _training(160, True)
    assert np.array_equal(P0.view(np.uint32), P1.view(np.uint32)) and np.array_equal(Q0.view(np.uint32), Q1.view(np.uint32))
    assert loss0 == loss1 and plans0 == plans1
    assert len(folds) == 4 and all(np.isfinite(f).all() and f.any() for f in folds)
    assert not np.array_equal(folds[0], folds[2])     # the second user fold saw the item rows of the first call


def test_fold_in_recommend():
    from buffalo_amd.parallel import NO_BIAS, TopK, fold_in_recommend
    d, k, case = 256, 10, AC.tiny(31)
    m = case.csr
    obj = FC.make_hip(d, modes=WIDE)
    _, Q = FC.bind(obj, case, d)
    pool = np.zeros(0, dtype=np.int32)
    keys, scores = np.zeros((m.num_users, k), np.int32), np.zeros((m.num_users, k), np.float32)
    fold_in_recommend(obj, m.indptr, m.keys, m.vals, keys, scores, pool, k)
    rows = obj.fold_in(0, m.indptr, m.keys, m.vals)
    eng = TopK()
    eng.set_seen(m.indptr, m.keys, m.num_items)
    ek, es = np.zeros_like(keys), np.zeros_like(scores)
    eng.recommend_unseen(np.arange(m.num_users, dtype=np.int32), rows, Q, NO_BIAS, ek, es, pool, k)
    assert np.array_equal(keys, ek) and np.array_equal(scores.view(np.uint32), es.view(np.uint32))
    for u in range(m.num_users):
        assert not np.intersect1d(keys[u], m.row(u)[0]).size
    assert (keys >= 0).all()
