"""The validation ranking on the fused path: `Evaluator.set_mode("fused" / "fused_c0" / "wave_select")` reach the ranking's engine, and
the filtered lists and the five doubles are the bits of the dense path, for every route and every batching."""
import numpy as np
import pytest

import eval_cases as ec

pytestmark = pytest.mark.gpu

RANK = ("ndcg", "map", "accuracy", "auc", "N")


def _evaluator(train, vali, **modes):
    from buffalo_amd.evaluate import Evaluator
    ev = Evaluator()
    ev.set_data(train.num_users, train.num_items, train.indptr, train.keys, vali["row"], vali["col"], vali["val"])
    for name, value in modes.items():
        ev.set_mode(name, value)
    return ev


@pytest.mark.parametrize("d,bias", [(20, False), (20, True), (128, False), (128, True)])
def test_fused_ranking_gives_the_dense_lists_and_metrics(d, bias):
    """eval_cases.planted with 6,000 items (user 0 without seen items, user 1 with all but 3 seen: no sample bounds its list, so it
    always takes the redo path, whose row -> user mapping comes from the device rows), topk 10 and 25, all validation users and a
    reversed subset.  With 500 items no segment and no list can overflow and the redo path would never run."""
    train, vali, P, Q, Qb = ec.planted(U=300, I=6000, d=d, bias=bias, seed=40 + d)
    all_rows = np.unique(vali["row"])
    subset = all_rows[::-2]
    subset = np.ascontiguousarray(subset if 1 in subset else np.append(subset, 1), dtype=np.int32)
    dense = _evaluator(train, vali, fused=0)
    for topk in (10, 25):
        for rows in (None, subset):
            n = len(all_rows) if rows is None else len(rows)
            want, want_keys = dense.ranking(P, Q, Qb, rows=rows, topk=topk, return_keys=True)
            assert want["N"] > 100
            for c0 in (0, 32):
                for wave in (1, 0):
                    for batch in (0, 128):
                        ev = _evaluator(train, vali, fused=1, fused_c0=c0, wave_select=wave, batch=batch)
                        got, keys = ev.ranking(P, Q, Qb, rows=rows, topk=topk, return_keys=True)
                        merges = ev.stats()["merges"]
                        print(d, bias, topk, n, "c0", c0, "wave", wave, "batch", batch, "merges", merges, "exchanges", ev.stats()["exchanges"])
                        assert np.array_equal(keys, want_keys), (topk, c0, wave, batch)
                        for k in RANK:
                            assert got[k] == want[k], (k, topk, c0, wave, batch, got[k], want[k])
                        if c0 == 32:
                            assert merges > 0            # the redo path ran (user 1 at the least)
                        else:
                            assert merges < n            # the fused path itself produced rows
    assert dense.stats()["merges"] == 0


def test_engine_modes_pass_through_and_unknown_ones_are_refused():
    from buffalo_amd._lib import BuffaloHipError
    train, vali, P, Q, _ = ec.planted(d=20, seed=6)
    ev = _evaluator(train, vali)
    base = ev.ranking(P, Q, topk=10)
    for name, value in (("fused", 1), ("fused_c0", 64), ("wave_select", 0), ("fused", -1), ("fused", 0)):
        ev.set_mode(name, value)
        assert ev.ranking(P, Q, topk=10) == base, (name, value)
    with pytest.raises(BuffaloHipError, match="unknown mode"):
        ev.set_mode("fused_c1", 1)
