"""What the device parity of bfh_bpr_fold_in rests on: no unsafe step in any instance, the float32 restatement inside the bound.  Conditions, no GPU."""
import numpy as np
import pytest

import bpr_fold_cases as FC


@pytest.mark.parametrize("inst", FC.INSTANCES, ids=lambda i: "d%d-bias%d-nn%d-table%d" % i)
def test_seed_is_safe_and_float32_stays_inside(inst):
    c = FC.instance(*inst)
    assert c["unsafe"] == 0
    f32, _, _ = FC.fold_ref(c["Q"], c["Qb"], c["steps"], c["init"], inst[1], dtype=np.float32)
    frac = (np.abs(f32.astype(np.float64) - c["f64"]) / c["bound"]).max()
    assert f32.dtype == np.float32 and frac <= 1.0
    assert np.array_equal(c["f64"][0], c["init"][0].astype(np.float64))   # the empty history returns its start row
