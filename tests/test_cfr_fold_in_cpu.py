"""The rule of bfh_cfr_fold_in as tests/cfr_fold_cases.py states it, against the float64 trainer step (ref_cfr.F64CFR) and against itself in float32."""
import numpy as np
import pytest

import cfr_cases as CC
import cfr_fold_cases as FC
from ref_cfr import F64CFR, relerr


@pytest.mark.parametrize("kind", ["item", "context"])
def test_one_iteration_from_the_rows_bias_is_the_trainer_step(kind):
    d, cs = 20, FC.case()
    arrs = {k: v.copy() for k, v in FC.references(kind, d, 1)[0].items()}
    init = arrs[kind + "_bias"][:cs.n, 0].copy()
    X, b = FC.fold(kind, arrs, cs, 1, init, np.float64)
    ref = FC.init_of(F64CFR(), d, "llt")
    CC.bind(ref, arrs)
    if kind == "item":
        ref.precompute(b"user")
        ref.partial_update_item(0, cs.n, cs.a.indptr, cs.a.keys, cs.a.vals, cs.c.indptr, cs.c.keys, cs.c.vals)
    else:
        ref.partial_update_context(0, cs.n, cs.c.indptr, cs.c.keys, cs.c.vals)
    live = np.array([sum(l) > 0 if kind == "item" else l[1] > 0 for l in cs.lens])
    assert relerr(X[live], ref.F[kind][:cs.n][live]) <= 1e-12 and relerr(b[live], ref.F[kind + "_bias"][:cs.n, 0][live]) <= 1e-12
    assert not X[~live].any() and np.array_equal(b[~live], init[~live].astype(np.float64))


@pytest.mark.parametrize("kind", ["user", "item", "context"])
def test_the_float32_restatement_is_the_rule(kind):
    _, _, (X32, b32), (X64, b64) = FC.references(kind, 33, 3)
    assert relerr(X32, X64) <= 1e-4 and (kind == "user" or relerr(b32, b64) <= 1e-4)
