# cython: language_level=3, boundscheck=False, wraparound=False
# distutils: language = c
"""buffalo/algo/hip/_plsi.pyx -- the `CyPLSI` surface of /root/reference/buffalo/algo/_plsi.pyx:23-67 bound to libbuffalo_hip.so's
C ABI (include/buffalo_hip.h) instead of the CPLSI C++ class."""
cimport numpy as np
from libc.stdint cimport int32_t, int64_t
import numpy as np

np.import_array()

cdef extern from "buffalo_hip.h":
    void* bfh_plsi_create() nogil
    void  bfh_plsi_destroy(void*) nogil
    int   bfh_plsi_init(void*, const char*) nogil
    int   bfh_plsi_initialize_model(void*, float*, int, float*, int) nogil
    int   bfh_plsi_synchronize(void*, int) nogil
    int   bfh_plsi_reset(void*) nogil
    int   bfh_plsi_partial_update(void*, int, int, const int64_t*, const int32_t*, const float*, float*) nogil
    int   bfh_plsi_normalize(void*, float, float) nogil
    int   bfh_plsi_swap(void*) nogil
    int   bfh_plsi_set_mode(void*, const char*, int64_t) nogil
    const char* bfh_last_error(const void*) nogil

cdef inline _raise(const void* h):
    cdef const char* msg = bfh_last_error(h)
    raise RuntimeError(msg.decode("utf-8", "replace") if msg != NULL else "libbuffalo_hip: unknown error")


cdef class CyPLSI:
    """HIP pLSI object holder (_plsi.pyx:23-25)"""
    cdef void* obj
    cdef object _keep        # swap() writes the new model into the caller's arrays

    def __cinit__(self):
        self.obj = bfh_plsi_create()
        self._keep = {}
        if self.obj == NULL:
            _raise(NULL)

    def __dealloc__(self):
        if self.obj != NULL:
            bfh_plsi_destroy(self.obj)
            self.obj = NULL

    def init(self, opt_path):                                       # :34-35
        cdef bytes b = opt_path if isinstance(opt_path, bytes) else str(opt_path).encode("utf-8")
        cdef int rc = bfh_plsi_init(self.obj, b)
        if rc < 0:
            _raise(self.obj)
        return rc == 1

    def swap(self):                                                 # :37-38
        if bfh_plsi_swap(self.obj) < 0:
            _raise(self.obj)

    def release(self):                                              # :40-41 (the handle owns the accumulators until __dealloc__)
        return

    def reset(self):                                                # :43-44
        if bfh_plsi_reset(self.obj) < 0:
            _raise(self.obj)

    def initialize_model(self, np.ndarray[np.float32_t, ndim=2] P, np.ndarray[np.float32_t, ndim=2] Q):   # :46-49
        self._keep.update(P=P, Q=Q)
        if bfh_plsi_initialize_model(self.obj, &P[0, 0], <int>P.shape[0], &Q[0, 0], <int>Q.shape[0]) < 0:
            _raise(self.obj)

    def normalize(self, alpha1, alpha2):                            # :51-52
        if bfh_plsi_normalize(self.obj, alpha1, alpha2) < 0:
            _raise(self.obj)

    def partial_update(self, int start_x, int next_x, np.ndarray[np.int64_t, ndim=1] indptr, np.ndarray[np.int32_t, ndim=1] keys,
                       np.ndarray[np.float32_t, ndim=1] vals):     # :54-58
        cdef float loss = 0
        cdef bint have = keys.shape[0] > 0
        if bfh_plsi_partial_update(self.obj, start_x, next_x, <const int64_t*>&indptr[0], <const int32_t*>&keys[0] if have else <const int32_t*>NULL,
                                   <const float*>&vals[0] if have else <const float*>NULL, &loss) < 0:
            _raise(self.obj)
        return loss

    def synchronize(self, device_to_host):                          # extension: inherit() overwrote rows of P / Q -> synchronize(False)
        if bfh_plsi_synchronize(self.obj, 1 if device_to_host else 0) < 0:
            _raise(self.obj)

    def set_mode(self, name, int64_t value):                        # extension: backend knobs
        cdef bytes b = name if isinstance(name, bytes) else str(name).encode("utf-8")
        if bfh_plsi_set_mode(self.obj, b, value) < 0:
            _raise(self.obj)
