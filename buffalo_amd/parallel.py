"""Top-k selection over factor products on the GPU -- the surface of ``buffalo.parallel``.

* ``dot_topn`` / ``quickselect`` mirror ``buffalo.parallel._core`` (/root/reference/buffalo/parallel/_core.pyx:27-56):
  same positional arguments, results written into the caller's ``out_keys`` / ``out_scores`` / ``result``.
* stock buffalo's own ``ParALS`` / ``ParBPRMF`` (parallel/base.py:77-156) call these two functions; they are not restated here
  (a stand-in for them lives with the test harness, tests/front_harness/buffalo_front/parallel.py).
* ``recommend_unseen`` is ``dot_topn`` that never lists what a user already has: ``TopK.set_seen`` binds the training matrix,
  every call then excludes row ``users[b]`` of it inside the selection (exactly ``k`` slots per user are selected, not
  ``k + max_seen`` candidates filtered in Python).
* ``most_similar`` is cosine top-k that leaves the model alone: ``dot_topn`` over the row-normalised copy of one factor matrix,
  which the library makes on the device with the bits of the reference's ``Algo._normalize`` (``normalize`` returns that copy);
  ``TopK.most_similar_device`` / ``normalize_device`` work on factors in HBM, ``most_similar_vectors`` takes query vectors.
* ``TopK.set_score_func("l2")`` makes the same calls rank by squared distance (a WARP model trained with ``score_func: "L2"``): the
  lists hold the nearest rows, ``out_scores`` their squared distances (smallest first, ``+inf`` in empty slots), no bias is taken and
  ``most_similar`` ranks the rows as given.  ``l2_topn`` / ``l2_recommend_unseen`` / ``l2_most_similar`` run on a default engine of
  their own, so the dot engine's mode is never flipped.
* ``TopK.dot_topn_device`` is the resident variant: it ranks straight from the HBM buffers of a training
  handle (``CyALS`` / ``CyBPR`` / ``CyWARP``), which is what validation right after an epoch wants.

Everything runs in ``libbuffalo_hip.so`` (``bfh_topk_*``); there is no CPU fallback.
"""
import ctypes as C

import numpy as np

from ._lib import Stats, check
from .backend import _arr, _Base, _ptr


SCORE_FUNCS = {"dot": 0, "l2": 1}


def _score_func_value(name):
    try:
        return SCORE_FUNCS[str(name).lower()]
    except KeyError:
        raise ValueError("score_func must be 'dot' or 'l2', not %r" % (name,)) from None


class TopK(_Base):
    _PFX = "bfh_topk_"

    def set_score_func(self, name):
        """``"dot"`` (default): rank by ``p . q (+ Qb)``.  ``"l2"``: rank by ``-|p - q|^2`` (``bfh_topk_set_mode(h, "score_func", 1)``)."""
        self.set_mode("score_func", _score_func_value(name))

    def dot_topn(self, indexes, P, Q, Qb, out_keys, out_scores, pool, k):
        _arr(indexes, np.int32, 1, "indexes"), _arr(P, np.float32, 2, "P"), _arr(Q, np.float32, 2, "Q")
        _arr(Qb, np.float32, 2, "Qb"), _arr(out_keys, np.int32, 2, "out_keys"), _arr(out_scores, np.float32, 2, "out_scores")
        _arr(pool, np.int32, 1, "pool")
        k = int(k)
        if out_keys.shape != (indexes.shape[0], k) or out_scores.shape != (indexes.shape[0], k):
            raise ValueError("out_keys / out_scores must be [len(indexes), k]")
        qb_rows = Qb.shape[0] if Qb.shape[1] != 0 else 0          # _core.pyx:49
        # "same matrix" is pointer identity in the reference (_core.hpp:98); keep that through ctypes
        p_ptr = _ptr(P, C.c_float)
        q_ptr = p_ptr if P.ctypes.data == Q.ctypes.data else _ptr(Q, C.c_float)
        self._call("dot_topn", _ptr(indexes, C.c_int32), indexes.shape[0], p_ptr, P.shape[0], P.shape[1], q_ptr, Q.shape[0], Q.shape[1],
                   _ptr(Qb, C.c_float), qb_rows, _ptr(out_keys, C.c_int32), _ptr(out_scores, C.c_float), _ptr(pool, C.c_int32),
                   pool.shape[0], k)

    def dot_topn_device(self, indexes, dP, p_rows, dQ, q_rows, d, ld, dQb, same, out_keys, out_scores, pool, k):
        """dP / dQ / dQb: device addresses (ints) of row-major [rows, ld] factors, e.g. ``obj.device_buffer("Q")[0]``."""
        _arr(indexes, np.int32, 1, "indexes"), _arr(out_keys, np.int32, 2, "out_keys"), _arr(out_scores, np.float32, 2, "out_scores")
        _arr(pool, np.int32, 1, "pool")
        self._call("dot_topn_device", _ptr(indexes, C.c_int32), indexes.shape[0], C.c_void_p(dP), int(p_rows), C.c_void_p(dQ), int(q_rows),
                   int(d), int(ld), C.c_void_p(dQb or 0), int(q_rows) if dQb else 0, int(bool(same)), _ptr(out_keys, C.c_int32),
                   _ptr(out_scores, C.c_float), _ptr(pool, C.c_int32), pool.shape[0], int(k))

    def set_seen(self, indptr, keys, num_items):
        """The training matrix whose rows are never recommended: int64 END offsets [num_users] (no leading 0), int32 keys ascending
        inside a row.  Kept in HBM on the handle until replaced."""
        _arr(indptr, np.int64, 1, "indptr"), _arr(keys, np.int32, 1, "keys")
        self._call("set_seen", indptr.shape[0], int(num_items), _ptr(indptr, C.c_int64), _ptr(keys, C.c_int32), keys.shape[0])

    def recommend_unseen(self, users, P, Q, Qb, out_keys, out_scores, pool, k):
        """Row b = the ``dot_topn`` row of ``users[b]`` with the user's seen items taken out of the pool (``bfh_topk_recommend_unseen``)."""
        _arr(users, np.int32, 1, "users"), _arr(P, np.float32, 2, "P"), _arr(Q, np.float32, 2, "Q")
        _arr(Qb, np.float32, 2, "Qb"), _arr(out_keys, np.int32, 2, "out_keys"), _arr(out_scores, np.float32, 2, "out_scores")
        _arr(pool, np.int32, 1, "pool")
        k = int(k)
        if out_keys.shape != (users.shape[0], k) or out_scores.shape != (users.shape[0], k):
            raise ValueError("out_keys / out_scores must be [len(users), k]")
        qb_rows = Qb.shape[0] if Qb.shape[1] != 0 else 0
        self._call("recommend_unseen", _ptr(users, C.c_int32), users.shape[0], _ptr(P, C.c_float), P.shape[0], P.shape[1], _ptr(Q, C.c_float),
                   Q.shape[0], Q.shape[1], _ptr(Qb, C.c_float), qb_rows, _ptr(out_keys, C.c_int32), _ptr(out_scores, C.c_float),
                   _ptr(pool, C.c_int32), pool.shape[0], k)

    def recommend_unseen_device(self, users, dP, p_rows, dQ, q_rows, d, ld, dQb, out_keys, out_scores, pool, k):
        """dP / dQ / dQb: device addresses (ints) of row-major [rows, ld] factors, as for ``dot_topn_device``."""
        _arr(users, np.int32, 1, "users"), _arr(out_keys, np.int32, 2, "out_keys"), _arr(out_scores, np.float32, 2, "out_scores")
        _arr(pool, np.int32, 1, "pool")
        k = int(k)
        if out_keys.shape != (users.shape[0], k) or out_scores.shape != (users.shape[0], k):
            raise ValueError("out_keys / out_scores must be [len(users), k]")
        self._call("recommend_unseen_device", _ptr(users, C.c_int32), users.shape[0], C.c_void_p(dP), int(p_rows), C.c_void_p(dQ), int(q_rows),
                   int(d), int(ld), C.c_void_p(dQb or 0), int(q_rows) if dQb else 0, _ptr(out_keys, C.c_int32), _ptr(out_scores, C.c_float),
                   _ptr(pool, C.c_int32), pool.shape[0], k)

    def normalize(self, F):
        """``Algo._normalize`` (algo/base.py:26-28) on the device, the same bits: a new [rows, cols] array, ``F`` is not written."""
        _arr(F, np.float32, 2, "F")
        out = np.empty_like(F)
        self._call("normalize", _ptr(F, C.c_float), F.shape[0], F.shape[1], _ptr(out, C.c_float))
        return out

    def normalize_device(self, dF, rows, d, ld, dOut=None):
        """The same in HBM: dF / dOut are device addresses (ints) of row-major [rows, ld] floats; ``dOut=None`` normalises in place."""
        self._call("normalize_device", C.c_void_p(dF), int(rows), int(d), int(ld), C.c_void_p(dF if dOut is None else dOut))

    @staticmethod
    def _similar_out(n, out_keys, out_scores, pool, k):
        _arr(out_keys, np.int32, 2, "out_keys"), _arr(out_scores, np.float32, 2, "out_scores"), _arr(pool, np.int32, 1, "pool")
        if out_keys.shape != (n, k) or out_scores.shape != (n, k):
            raise ValueError("out_keys / out_scores must be [number of queries, k]")

    def most_similar(self, indexes, F, out_keys, out_scores, pool, k):
        """Row b = the ``dot_topn`` row of ``indexes[b]`` with P = Q = ``normalize(F)`` (``bfh_topk_most_similar``); ``F`` is not written."""
        _arr(indexes, np.int32, 1, "indexes"), _arr(F, np.float32, 2, "F")
        k = int(k)
        self._similar_out(indexes.shape[0], out_keys, out_scores, pool, k)
        self._call("most_similar", _ptr(indexes, C.c_int32), indexes.shape[0], _ptr(F, C.c_float), F.shape[0], F.shape[1],
                   _ptr(out_keys, C.c_int32), _ptr(out_scores, C.c_float), _ptr(pool, C.c_int32), pool.shape[0], k)

    def most_similar_device(self, indexes, dF, rows, d, ld, out_keys, out_scores, pool, k):
        """dF: device address (int) of the row-major [rows, ld] factors, as for ``dot_topn_device``; it is not written."""
        _arr(indexes, np.int32, 1, "indexes")
        k = int(k)
        self._similar_out(indexes.shape[0], out_keys, out_scores, pool, k)
        self._call("most_similar_device", _ptr(indexes, C.c_int32), indexes.shape[0], C.c_void_p(dF), int(rows), int(d), int(ld),
                   _ptr(out_keys, C.c_int32), _ptr(out_scores, C.c_float), _ptr(pool, C.c_int32), pool.shape[0], k)

    def most_similar_vectors(self, V, F, out_keys, out_scores, pool, k):
        """The queries are the rows of ``V`` [n, cols], scored as given against ``normalize(F)``: no self-exclusion."""
        _arr(V, np.float32, 2, "V"), _arr(F, np.float32, 2, "F")
        if V.shape[1] != F.shape[1]:
            raise ValueError("V and F must have the same number of columns")
        k = int(k)
        self._similar_out(V.shape[0], out_keys, out_scores, pool, k)
        self._call("most_similar_vectors", _ptr(V, C.c_float), V.shape[0], _ptr(F, C.c_float), F.shape[0], F.shape[1],
                   _ptr(out_keys, C.c_int32), _ptr(out_scores, C.c_float), _ptr(pool, C.c_int32), pool.shape[0], k)

    def quickselect(self, scores, result, sorted=True):
        _arr(scores, np.float32, 2, "scores"), _arr(result, np.int32, 2, "result")
        if result.shape[0] != scores.shape[0]:
            raise ValueError("result must have one row per row of scores")
        self._call("quickselect", _ptr(scores, C.c_float), scores.shape[0], scores.shape[1], _ptr(result, C.c_int32), result.shape[1],
                   int(bool(sorted)))


NO_BIAS = np.empty((1, 0), dtype=np.float32)
_default = None


def _engine():
    global _default
    if _default is None:
        _default = TopK()
    return _default


def dot_topn(indexes, P, Q, Qb, out_keys, out_scores, pool, k, num_threads=0):
    """buffalo.parallel._core.dot_topn (_core.pyx:39-56); ``num_threads`` is accepted and ignored."""
    _engine().dot_topn(indexes, P, Q, Qb, out_keys, out_scores, pool, k)


def recommend_unseen(users, P, Q, Qb, out_keys, out_scores, pool, k, num_threads=0):
    """``dot_topn`` without the items of ``set_seen`` (call ``_engine().set_seen(indptr, keys, num_items)`` first)."""
    _engine().recommend_unseen(users, P, Q, Qb, out_keys, out_scores, pool, k)


_default_fold = None


def _fold_engine():
    """The engine of ``fold_in_recommend``: a handle of its own, because every call replaces its seen matrix."""
    global _default_fold
    if _default_fold is None:
        _default_fold = TopK()
    return _default_fold


def check_ascending_rows(indptr, keys):
    """``ValueError`` unless the keys of every CSR row (int64 END offsets) ascend strictly -- what ``TopK.set_seen`` wants; nothing is sorted."""
    _arr(indptr, np.int64, 1, "indptr"), _arr(keys, np.int32, 1, "keys")
    if keys.shape[0] < 2:
        return
    bad = np.flatnonzero(keys[1:] <= keys[:-1]) + 1          # positions that do not ascend ...
    bad = bad[~np.isin(bad, indptr)]                         # ... and are not the first entry of a row
    if bad.size:
        row = int(np.searchsorted(indptr, bad[0], side="right"))
        raise ValueError("row %d of the histories is not strictly ascending (position %d); fold_in_recommend does not sort" % (row, int(bad[0])))


def fold_in_recommend(als, indptr, keys, vals, out_keys, out_scores, pool, k):
    """Top-k for users who are not in the model: their rows by ``als.fold_in_device(0, ...)``, ranked against the model's items with the
    histories themselves as the seen matrix -- the rows never leave HBM.  ``als``: a ``CyALS`` with a model; CSR of ``n`` histories with keys
    strictly ascending inside a row; ``out_keys`` / ``out_scores`` [n, k]; ``pool`` as for ``dot_topn``."""
    check_ascending_rows(indptr, keys)
    vdim = als.get_vdim()
    dQ, q_bytes = als.device_buffer("Q")
    num_items = q_bytes // (4 * vdim)
    dP, n = als.fold_in_device(0, indptr, keys, vals)
    eng = _fold_engine()
    eng.set_seen(indptr, keys, num_items)
    eng.recommend_unseen_device(np.arange(n, dtype=np.int32), dP, n, dQ, num_items, vdim, vdim, None, out_keys, out_scores, pool, k)


def plsi_fold_in_recommend(plsi, indptr, keys, vals, iters, alpha1, out_keys, out_scores, pool, k):
    """``fold_in_recommend`` for pLSI: topic rows of ``n`` new documents by ``plsi.fold_in_device(...)`` (``iters`` EM steps from the uniform
    start, smoothing ``alpha1``), ranked against the handle's ``"Q"`` with the histories as the seen matrix.  Scores are ``P . Q`` without a bias
    (plsi.py:113-119).  ``plsi``: a ``CyPLSI`` with a model; keys strictly ascending inside a row; ``out_keys`` / ``out_scores`` [n, k]."""
    check_ascending_rows(indptr, keys)
    vdim = plsi.get_vdim()
    dQ, q_bytes = plsi.device_buffer("Q")
    num_items = q_bytes // (4 * vdim)
    dP, n = plsi.fold_in_device(indptr, keys, vals, iters, alpha1)
    eng = _fold_engine()
    eng.set_seen(indptr, keys, num_items)
    eng.recommend_unseen_device(np.arange(n, dtype=np.int32), dP, n, dQ, num_items, plsi.dim(), vdim, None, out_keys, out_scores, pool, k)


_default_l2 = None


def _l2_engine():
    """The default engine of the L2 calls: a handle of its own, switched once when it is made."""
    global _default_l2
    if _default_l2 is None:
        eng = TopK()
        eng.set_score_func("l2")
        _default_l2 = eng
    return _default_l2


def l2_topn(indexes, P, Q, out_keys, out_scores, pool, k, num_threads=0):
    """``WARP._get_topk_recommendation`` under ``score_func: "L2"`` (warp.py:94-107): row b = the k rows of ``Q`` nearest to
    ``P[indexes[b]]``, ``out_scores`` their squared distances."""
    _l2_engine().dot_topn(indexes, P, Q, NO_BIAS, out_keys, out_scores, pool, k)


def l2_recommend_unseen(users, P, Q, out_keys, out_scores, pool, k, num_threads=0):
    """``l2_topn`` without the items of ``set_seen`` (call ``_l2_engine().set_seen(indptr, keys, num_items)`` first)."""
    _l2_engine().recommend_unseen(users, P, Q, NO_BIAS, out_keys, out_scores, pool, k)


def l2_most_similar(indexes, F, out_keys, out_scores, pool, k, num_threads=0):
    """``WARP._get_most_similar_L2`` (warp.py:115-136) for index queries: the k rows of ``F`` nearest to ``F[indexes[b]]``, itself left out."""
    _l2_engine().most_similar(indexes, F, out_keys, out_scores, pool, k)


def most_similar(indexes, F, out_keys, out_scores, pool, k, num_threads=0):
    """What ``Parallel._most_similar`` (parallel/base.py:21-28) gives after ``algo.normalize(group)`` -- without normalising ``F``."""
    _engine().most_similar(indexes, F, out_keys, out_scores, pool, k)


def normalize(F):
    """``Algo._normalize`` (algo/base.py:26-28): the row-normalised copy of ``F``."""
    return _engine().normalize(F)


def quickselect(scores, result, sorted, num_threads=0):
    """buffalo.parallel._core.quickselect (_core.pyx:27-35); rows always come back sorted."""
    _engine().quickselect(scores, result, sorted)


__all__ = ["TopK", "dot_topn", "recommend_unseen", "most_similar", "normalize", "quickselect", "l2_topn", "l2_recommend_unseen",
           "l2_most_similar", "fold_in_recommend", "Stats", "check"]
