"""Fold-in yardsticks on the host (no GPU): the float32 restatement and the float32 oracle sit inside each other's envelope against float64, the
envelope bites on one planted defect in one row, and fold_in_recommend refuses unsorted histories before it touches a handle."""
import numpy as np
import pytest

import als_cases as AC
import fold_in_cases as FC
from ref_eals import bound, relerr


@pytest.mark.parametrize("d, adaptive", [(20, False), (40, True), (96, False)])
def test_fold_f32_inside_the_oracles_envelope(d, adaptive):
    """fold_f32 against fold_f64 with the float32 oracle (llt, zeros for P, the histories as its matrix) as the comparison run, on pattern()."""
    orc, f64, Q, rows = FC.references(d, adaptive)
    case = AC.pattern()
    f32 = FC.fold_f32(case.csr, Q, 0, adaptive)
    FC.hold("fold_in cpu d=%d%s fold_f32 vs oracle" % (d, " adaptive_reg" if adaptive else ""), f32, orc, f64, rows)
    # the oracle's rows with entries ARE the fold-in: they equal the yardstick within the oracle's own recorded distance; its empty row is untouched
    eo = relerr(orc, f64)
    assert eo <= 1e-5, eo                      # rounding, not conditioning (the issue's table: 2.7e-6 at d = 20)
    assert relerr(f32, f64) <= 1e-5
    assert not orc[0].any() and not f64[0].any() and not f32[0].any()
    assert np.abs(f64[1:]).max(axis=1).min() > 0


def _row(n):
    return AC.NAMED_LENGTHS.index(n)


@pytest.mark.parametrize("defect, length, adaptive", [("drop_last_entry", 4097, False), ("reg_not_adaptive", 64, True),
                                                      ("y_without_one", 193, False), ("skip_last_diagonal", 17, False)])
def test_one_planted_defect_breaks_the_envelope(defect, length, adaptive):
    """A copy of fold_f32 with one defect in one named row of pattern() at d = 128 leaves that row's envelope; without it the row holds."""
    d, case, r = 128, AC.pattern(), _row(length)
    _, Q = AC.start(case, d)
    rows = [r]
    f64 = FC.fold_f64(case.csr, Q, 0, adaptive, rows)
    good = FC.fold_f32(case.csr, Q, 0, adaptive, rows)
    broken = FC.fold_f32(case.csr, Q, 0, adaptive, rows, defect=defect, defect_row=r)
    eg, eb = relerr(good[r], f64[r]), relerr(broken[r], f64[r])
    AC.record("fold_in cpu d=128 defect %s in the %d-entry row" % (defect, length), ["err(fold_f32, f64) %.3g err(defective, f64) %.3g bound %.3g" % (eg, eb, bound(eg))])
    assert eg <= 1e-5
    assert eb > bound(eg), (defect, eb, bound(eg))


class _StubAls:
    """Stands where the CyALS would: fold_in_recommend must raise before it asks the handle for anything."""
    def __getattr__(self, name):
        raise AssertionError("fold_in_recommend touched the handle (%s) before checking its arguments" % name)


def test_fold_in_recommend_refuses_unsorted_rows():
    from buffalo_amd.parallel import check_ascending_rows, fold_in_recommend
    indptr = np.array([3, 3, 5], dtype=np.int64)
    vals = np.ones(5, dtype=np.float32)
    out_k, out_s, pool = np.zeros((3, 2), np.int32), np.zeros((3, 2), np.float32), np.zeros(0, np.int32)
    for keys in ([0, 2, 1, 4, 7], [0, 1, 1, 4, 7], [0, 1, 2, 7, 7]):      # descending inside a row; a duplicate; a duplicate in the last row
        with pytest.raises(ValueError, match="not strictly ascending"):
            fold_in_recommend(_StubAls(), indptr, np.array(keys, dtype=np.int32), vals, out_k, out_s, pool, 2)
    check_ascending_rows(indptr, np.array([5, 6, 7, 0, 1], dtype=np.int32))       # a new row may start lower than the last one ended
    check_ascending_rows(np.array([0, 0], dtype=np.int64), np.zeros(0, dtype=np.int32))
    with pytest.raises(ValueError):
        check_ascending_rows(indptr.astype(np.int32), np.array([0, 1, 2, 3, 4], dtype=np.int32))    # dtype, in the file's _arr style
