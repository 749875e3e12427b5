# cython: language_level=3, boundscheck=False, wraparound=False
# distutils: language = c
"""buffalo/algo/hip/_evaluate.pyx -- `CyEvaluator`: the validation step of /root/reference/buffalo/evaluate/base.py:44-148 bound to
libbuffalo_hip.so's C ABI (include/buffalo_hip.h, `bfh_eval_*`).  The reference has no native evaluator; an `Evaluable` that holds one of
these overrides `get_validation_results`, `_evaluate_ranking_metrics` and `_evaluate_score_metrics` (INTEGRATION.md)."""
cimport numpy as np
from libc.stdint cimport int32_t, int64_t, uintptr_t
import numpy as np

np.import_array()

cdef extern from "buffalo_hip.h":
    void* bfh_eval_create() nogil
    void  bfh_eval_destroy(void*) nogil
    int   bfh_eval_set_data(void*, int, int, const int64_t*, const int32_t*, int64_t, const int32_t*, const int32_t*, const float*, int64_t) nogil
    int   bfh_eval_num_rows(void*) nogil
    int   bfh_eval_ranking(void*, const float*, int, int, const float*, int, int, const float*, int, const int32_t*, int, int, double*, int32_t*) nogil
    int   bfh_eval_ranking_device(void*, const float*, int, const float*, int, int, int, const float*, int, const int32_t*, int, int, double*,
                                  int32_t*) nogil
    int   bfh_eval_scores(void*, const float*, int, int, const float*, int, int, const float*, int, double*) nogil
    int   bfh_eval_scores_device(void*, const float*, int, const float*, int, int, int, const float*, int, double*) nogil
    int   bfh_eval_set_mode(void*, const char*, int64_t) nogil
    const char* bfh_last_error(const void*) nogil

cdef inline _raise(const void* h):
    cdef const char* msg = bfh_last_error(h)
    raise RuntimeError(msg.decode("utf-8", "replace") if msg != NULL else "libbuffalo_hip: unknown error")


cdef class CyEvaluator:
    """HIP validation object holder"""
    cdef void* obj

    def __cinit__(self):
        self.obj = bfh_eval_create()
        if self.obj == NULL:
            _raise(NULL)

    def __dealloc__(self):
        if self.obj != NULL:
            bfh_eval_destroy(self.obj)
            self.obj = NULL

    def set_data(self, int num_users, int num_items, np.ndarray[np.int64_t, ndim=1] indptr not None, np.ndarray[np.int32_t, ndim=1] keys not None,
                 np.ndarray[np.int32_t, ndim=1] vali_row not None, np.ndarray[np.int32_t, ndim=1] vali_col not None,
                 np.ndarray[np.float32_t, ndim=1] vali_val not None):
        """Data._prepare_validation_data: the rowwise group (END offsets, ascending keys) and the vali group, uploaded once"""
        cdef int64_t nnz = keys.shape[0], n = vali_row.shape[0]
        if indptr.shape[0] != num_users or vali_col.shape[0] != n or vali_val.shape[0] != n:
            raise ValueError("indptr needs one END offset per user, the vali arrays one length")
        if bfh_eval_set_data(self.obj, num_users, num_items, <const int64_t*>indptr.data, <const int32_t*>keys.data, nnz,
                             <const int32_t*>vali_row.data, <const int32_t*>vali_col.data, <const float*>vali_val.data, n) < 0:
            _raise(self.obj)

    def num_rows(self):
        cdef int n = bfh_eval_num_rows(self.obj)
        if n < 0:
            _raise(self.obj)
        return n

    cdef _ranking_result(self, double* out, keys):
        res = {"ndcg": out[0], "map": out[1], "accuracy": out[2], "auc": out[3], "N": out[4]}
        return res if keys is None else (res, keys)

    def ranking(self, np.ndarray[np.float32_t, ndim=2] P not None, np.ndarray[np.float32_t, ndim=2] Q not None,
                np.ndarray[np.float32_t, ndim=1] Qb not None, rows, int topk,
                return_keys=False):
        """evaluate/base.py:44-128; Qb of length 0: no bias; rows None: every user with vali entries"""
        cdef np.ndarray[np.int32_t, ndim=1] r = np.zeros(0, dtype=np.int32) if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
        cdef int n = self.num_rows() if rows is None else <int>r.shape[0]
        cdef np.ndarray[np.int32_t, ndim=2] keys = np.empty((n if return_keys else 0, max(topk, 1)), dtype=np.int32)
        cdef double out[5]
        if bfh_eval_ranking(self.obj, <const float*>P.data, <int>P.shape[0], <int>P.shape[1], <const float*>Q.data, <int>Q.shape[0], <int>Q.shape[1],
                            <const float*>Qb.data if Qb.shape[0] else <const float*>NULL, <int>Qb.shape[0],
                            <const int32_t*>NULL if rows is None else <const int32_t*>r.data, n, topk, out,
                            <int32_t*>keys.data if return_keys else <int32_t*>NULL) < 0:
            _raise(self.obj)
        return self._ranking_result(out, keys if return_keys else None)

    def ranking_device(self, uintptr_t dP, int p_rows, uintptr_t dQ, int q_rows, int d, int ld, uintptr_t dQb, rows, int topk, return_keys=False):
        """the same from HBM: dP / dQ / dQb are device addresses (dQb 0: no bias), e.g. CyBPR.device_buffer"""
        cdef np.ndarray[np.int32_t, ndim=1] r = np.zeros(0, dtype=np.int32) if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
        cdef int n = self.num_rows() if rows is None else <int>r.shape[0]
        cdef np.ndarray[np.int32_t, ndim=2] keys = np.empty((n if return_keys else 0, max(topk, 1)), dtype=np.int32)
        cdef double out[5]
        if bfh_eval_ranking_device(self.obj, <const float*>dP, p_rows, <const float*>dQ, q_rows, d, ld, <const float*>dQb, q_rows if dQb else 0,
                                   <const int32_t*>NULL if rows is None else <const int32_t*>r.data, n, topk, out,
                                   <int32_t*>keys.data if return_keys else <int32_t*>NULL) < 0:
            _raise(self.obj)
        return self._ranking_result(out, keys if return_keys else None)

    def scores(self, np.ndarray[np.float32_t, ndim=2] P not None, np.ndarray[np.float32_t, ndim=2] Q not None,
               np.ndarray[np.float32_t, ndim=1] Qb not None):
        """evaluate/base.py:130-148"""
        cdef double out[2]
        if bfh_eval_scores(self.obj, <const float*>P.data, <int>P.shape[0], <int>P.shape[1], <const float*>Q.data, <int>Q.shape[0], <int>Q.shape[1],
                           <const float*>Qb.data if Qb.shape[0] else <const float*>NULL, <int>Qb.shape[0], out) < 0:
            _raise(self.obj)
        return {"rmse": out[0], "error": out[1]}

    def scores_device(self, uintptr_t dP, int p_rows, uintptr_t dQ, int q_rows, int d, int ld, uintptr_t dQb):
        cdef double out[2]
        if bfh_eval_scores_device(self.obj, <const float*>dP, p_rows, <const float*>dQ, q_rows, d, ld, <const float*>dQb, q_rows if dQb else 0, out) < 0:
            _raise(self.obj)
        return {"rmse": out[0], "error": out[1]}

    def set_mode(self, name, int64_t value):                        # extension: backend knobs
        cdef bytes b = name if isinstance(name, bytes) else str(name).encode("utf-8")
        if bfh_eval_set_mode(self.obj, b, value) < 0:
            _raise(self.obj)
