"""The premises of tests/test_eals_fold_in_gpu.py that need no device: the ABI names, the size of the envelope, the closed form."""
import ctypes as C

import numpy as np

import eals_fold_cases as FC
from ref_eals import relerr


def test_the_abi_names_are_declared_and_mirrored():
    from buffalo_amd import _lib
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    pi64, pi32, pf = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_float)
    want = {"bfh_eals_fold_in": (i32, [vp, i32, pi64, pi32, pf, i64, i32, pf, pf]),
            "bfh_eals_device_buffer": (i32, [vp, C.c_char_p, C.POINTER(vp), C.POINTER(C.c_size_t)]),
            "bfh_eals_get_vdim": (i32, [vp]), "bfh_eals_get_dim": (i32, [vp])}
    for name, sig in want.items():
        assert name in _lib.header_symbols() and _lib.SIGNATURES[name] == sig, name


def test_the_float32_restatement_stays_within_1e_6_of_float64():
    _, f32, f64 = FC.references(20, False)
    assert FC.named_lengths(20)[11:14] == (475, 476, 477) and f32.shape == (28, 20)
    assert 0 < relerr(f32, f64) <= 1e-6, relerr(f32, f64)


def test_the_recurrence_converges_to_the_closed_form():
    _, Q, Cw = FC.model(20)
    ip, k, v = FC.csr_of([257, 1025], 3)
    got = FC.fold(Q, Cw, ip, k, v, 30, None, np.float64)
    for (b, e), row in zip(FC.rows_of(ip), got):
        assert relerr(row, FC.solve(Q, Cw, k[b:e], v[b:e])) <= 4e-15
