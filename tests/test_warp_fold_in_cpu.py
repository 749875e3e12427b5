"""What the device parity of bfh_warp_fold_in rests on: no unsafe decision in any instance, every outcome of the trial loop present, the float32
restatement inside the derived bound with the same counts.  Conditions, no GPU."""
import numpy as np
import pytest

import warp_fold_cases as FC


@pytest.mark.parametrize("inst", FC.ALL, ids=lambda i: "d%d-%s-%s-pcn%d-big%d" % i)
def test_seed_is_safe_and_float32_stays_inside(inst):
    c = FC.instance(*inst)
    assert c["unsafe"] == 0 and c["outcomes"] == set(FC.OUTCOMES)
    f32, counts, _, _, _ = FC.fold_ref(c, dtype=np.float32)
    assert f32.dtype == np.float32 and np.array_equal(counts, c["counts"])
    assert (np.abs(f32.astype(np.float64) - c["f64"]) <= c["bound"]).all()
    if not inst[4]:   # the empty history returns its start row; the row of every item scores nothing and accepts nothing
        assert np.array_equal(c["f64"][0], c["init"][0].astype(np.float64)) and not c["counts"][9].any()
