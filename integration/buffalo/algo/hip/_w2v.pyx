# cython: language_level=3, boundscheck=False, wraparound=False
# distutils: language = c
"""buffalo/algo/hip/_w2v.pyx -- the `CyW2V` surface of /root/reference/buffalo/algo/_w2v.pyx:28-69 bound to libbuffalo_hip.so's
C ABI (include/buffalo_hip.h) instead of the CW2V C++ class."""
cimport numpy as np
from libc.stdint cimport int32_t, int64_t, uint32_t
import numpy as np

np.import_array()

cdef extern from "buffalo_hip.h":
    void* bfh_w2v_create() nogil
    void  bfh_w2v_destroy(void*) nogil
    int   bfh_w2v_init(void*, const char*) nogil
    int   bfh_w2v_initialize_model(void*, float*, int, const int32_t*, int, const uint32_t*, const int32_t*, int64_t) nogil
    int   bfh_w2v_launch_workers(void*) nogil
    int   bfh_w2v_add_jobs(void*, int, int, const int64_t*, const int32_t*) nogil
    int   bfh_w2v_join(void*, double*) nogil
    int   bfh_w2v_synchronize(void*, int) nogil
    int   bfh_w2v_set_mode(void*, const char*, int64_t) nogil
    const char* bfh_last_error(const void*) nogil

cdef inline _raise(const void* h):
    cdef const char* msg = bfh_last_error(h)
    raise RuntimeError(msg.decode("utf-8", "replace") if msg != NULL else "libbuffalo_hip: unknown error")


cdef class CyW2V:
    """HIP W2V object holder (_w2v.pyx:28-30)"""
    cdef void* obj
    cdef object _keep        # join() writes the model into the caller's L0

    def __cinit__(self):
        self.obj = bfh_w2v_create()
        self._keep = {}
        if self.obj == NULL:
            _raise(NULL)

    def __dealloc__(self):                                          # :35-37 (release + delete)
        if self.obj != NULL:
            bfh_w2v_destroy(self.obj)
            self.obj = NULL

    def init(self, option_path):                                    # :39-40
        cdef bytes b = option_path if isinstance(option_path, bytes) else str(option_path).encode("utf-8")
        cdef int rc = bfh_w2v_init(self.obj, b)
        if rc < 0:
            _raise(self.obj)
        return rc == 1

    def initialize_model(self, np.ndarray[np.float32_t, ndim=2] L0, np.ndarray[np.int32_t, ndim=1] index, np.ndarray[np.uint32_t, ndim=1] scale,
                         np.ndarray[np.int32_t, ndim=1] dist, int64_t total_word_count):   # :42-53
        if scale.shape[0] != L0.shape[0] or dist.shape[0] != L0.shape[0]:
            raise ValueError("scale and dist must have one entry per row of L0")
        self._keep.update(L0=L0)
        if bfh_w2v_initialize_model(self.obj, &L0[0, 0], <int>L0.shape[0], <const int32_t*>&index[0], <int>index.shape[0], <const uint32_t*>&scale[0],
                                    <const int32_t*>&dist[0], total_word_count) < 0:
            _raise(self.obj)

    def launch_workers(self):                                       # :55-56
        if bfh_w2v_launch_workers(self.obj) < 0:
            _raise(self.obj)

    def add_jobs(self, int start_x, int next_x, np.ndarray[np.int64_t, ndim=1] indptr, np.ndarray[np.int32_t, ndim=1] sequences):   # :58-66
        cdef bint have = sequences.shape[0] > 0
        if bfh_w2v_add_jobs(self.obj, start_x, next_x, <const int64_t*>&indptr[0], <const int32_t*>&sequences[0] if have else <const int32_t*>NULL) < 0:
            _raise(self.obj)

    def join(self):                                                 # :68-69
        cdef double loss = 0
        if bfh_w2v_join(self.obj, &loss) < 0:
            _raise(self.obj)
        return loss

    def release(self):                                              # the handle owns L1 until __dealloc__
        return

    def synchronize(self, device_to_host):                          # extension: copy L0 back without ending the run / upload it again
        if bfh_w2v_synchronize(self.obj, 1 if device_to_host else 0) < 0:
            _raise(self.obj)

    def set_mode(self, name, int64_t value):                        # extension: backend knobs
        cdef bytes b = name if isinstance(name, bytes) else str(name).encode("utf-8")
        if bfh_w2v_set_mode(self.obj, b, value) < 0:
            _raise(self.obj)
