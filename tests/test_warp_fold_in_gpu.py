"""bfh_warp_fold_in on the device (csrc/warp_fold_kernels.hpp behind CyWARP.fold_in) against the float64 restatement of its rule (warp_fold_cases.py)."""
import numpy as np
import pytest

import helpers as H
import warp_fold_cases as FC
from conftest import tiny_csr, warp_opt

pytestmark = pytest.mark.gpu
I64, I32 = (lambda *v: np.array(v, np.int64)), (lambda *v: np.array(v, np.int32))
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
ids = lambda i: "d%d-%s-%s-pcn%d-big%d" % i


def make(opt, Q=None):   # a CyWARP whose item side is Q -- without it: no model yet; P is three rows nobody folds into
    from buffalo_amd.backend import CyWARP
    g = CyWARP()
    assert g.init(H.write_opt(warp_opt(accelerator=True, **opt)))
    if Q is not None:
        g.initialize_model(np.full((3, g.get_vdim()), 0.1, np.float32), H.pad(Q, g.get_vdim()), np.zeros((Q.shape[0], 1), np.float32), 10, True)
    return g


def fold(g, c, rows=None, counts=None):   # fold_in over `rows` of the instance's histories, in that order, under their own row ids
    rows, beg = np.arange(c["indptr"].shape[0]) if rows is None else np.asarray(rows), np.concatenate([[0], c["indptr"]])
    keys = np.concatenate([c["keys"][beg[b]:beg[b + 1]] for b in rows]).astype(np.int32)
    return g.fold_in(np.cumsum(beg[rows + 1] - beg[rows]), keys, FC.ITERS, FC.LR, row_ids=rows.astype(np.int32), init=np.ascontiguousarray(c["init"][rows]),
                     counts=counts)


@pytest.mark.parametrize("inst", FC.ALL, ids=ids)
def test_parity_against_float64(inst):
    """The counts are the restatement's integers; |p_k - p64_k| <= the bound tracked beside the float64 run (derived in warp_fold_cases)."""
    c = FC.instance(*inst)
    counts = np.zeros((c["indptr"].shape[0], 2), np.int64)
    out = fold(make(c["opt"], c["Q"]), c, counts=counts)
    err = np.abs(out.astype(np.float64) - c["f64"])
    print("warp fold_in parity %s: worst error / bound %.4f, counts %s" % (inst, (err / np.maximum(c["bound"], 1e-300)).max(), counts.sum(axis=0)))
    assert np.array_equal(counts, c["counts"])
    assert (err <= c["bound"]).all()
    assert inst[4] or np.array_equal(bits(out[0]), bits(c["init"][0]))   # the empty history (not in the BIG instances) returns its start row


@pytest.mark.parametrize("inst", [(20, "l2", "adam", 1, False), (96, "dot", "adagrad", 1, False), (256, "l2", "adagrad", 0, False)], ids=["G16", "G32", "G64"])
def test_rows_do_not_depend_on_their_batch_or_block(inst):
    """Reversed, split in two, run again: the same bits.  And the histories 600 times under the same row ids, the launch held to 4 waves per CU, far
    fewer blocks than rows: every block takes further rows from the counter."""
    c = FC.instance(*inst)
    g, n = make(c["opt"], c["Q"]), c["indptr"].shape[0]
    whole = fold(g, c)
    for rows in (range(n - 1, -1, -1), [0, 2, 4, 8, 9], [1, 3, 5, 6, 7, 10], range(n)):
        assert np.array_equal(bits(fold(g, c, rows)), bits(whole[list(rows)]))
    g.set_mode("waves_per_cu", 4)
    many = fold(g, c, np.tile(np.arange(n), 600))
    assert np.array_equal(bits(many).reshape(600, n, -1), np.broadcast_to(bits(whole), (600, n, inst[0])))


def test_the_model_and_the_next_epoch_do_not_notice():
    c = FC.instance(64, "dot", "adam", 1, False)
    csr = tiny_csr(U=3, I=FC.ITEMS, density=0.02, seed=4)
    state = lambda h: np.concatenate([bits(h.device_tensor(n).cpu().numpy()).ravel() for n in ("P", "Q", "Qb", "gradP", "gradQ", "velP", "momP", "countP")])
    g, twin = (make(c["opt"], c["Q"]) for _ in range(2))
    before = state(g)
    fold(g, c)
    assert np.array_equal(before, state(g))
    for h in (g, twin):
        h.set_mode("sequential", 1)
        h.set_placeholder(csr.indptr, csr.nnz + 1)
        h.add_jobs(0, 3, csr.indptr, csr.keys)
        h.update_parameters()
    assert np.array_equal(state(g), state(twin)) and not np.array_equal(state(g), before)   # the epoch did move the model


def refusal(n_rows=2, indptr=I64(2, 4), keys=I32(1, 5, 2, 9), nnz=4, iters=2, status=-1, model=True, good=True, **opt):
    return (n_rows, indptr, keys, nnz, iters), status, model, good, dict(dict(d=20, random_seed=1), **opt)


# a refused call: its arguments, the status, whether a model is bound, whether a good call can go first
REFUSALS = {
    "before initialize_model": refusal(model=False, good=False), "negative n_rows": refusal(n_rows=-1), "negative iters": refusal(iters=-1),
    "iters above 10000": refusal(iters=10001), "negative nnz": refusal(nnz=-4), "decreasing indptr": refusal(indptr=I64(4, 2)),
    "indptr[-1] != nnz": refusal(indptr=I64(2, 3)), "null keys": refusal(keys=None), "null indptr": refusal(indptr=None),
    "key below 0": refusal(keys=I32(-1, 5, 2, 9)), "key = num_items": refusal(keys=I32(1, 5, 2, FC.ITEMS)),
    "keys descend": refusal(keys=I32(5, 1, 2, 9)), "a key twice": refusal(keys=I32(1, 1, 2, 9)),
    "d = 288": refusal(status=-3, good=False, d=288),
}


@pytest.mark.parametrize("name", REFUSALS)
def test_refusals(name):
    """Every refusal of the header, through the C ABI: the status, a message, and the rows of an earlier good call still in "fold"."""
    from buffalo_amd import _lib
    (n_rows, indptr, keys, nnz, iters), status, model, good, opt = REFUSALS[name]
    g = make(opt, FC.model(opt["d"], "dot", 0, 3, FC.ITEMS)[0] if model else None)
    if good:
        rows = g.fold_in(I64(2), I32(400, 500), 2, 0.05, init=np.full((1, opt["d"]), 0.05, np.float32))
        kept = bits(g.device_tensor("fold").cpu().numpy())
        assert np.array_equal(kept.ravel()[:opt["d"]], bits(rows[0])) and rows.any()
    ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)
    assert _lib.lib().bfh_warp_fold_in(g._h, n_rows, ptr(indptr, _lib._pi64), ptr(keys, _lib._pi32), nnz, None, iters, 0.05, None, None, None, None) == status
    assert b"fold_in" in _lib.lib().bfh_last_error(g._h)
    assert not good or np.array_equal(bits(g.device_tensor("fold").cpu().numpy()), kept)


@pytest.mark.parametrize("score", ["dot", "l2"])
def test_recommend_from_the_folded_rows(score):
    from buffalo_amd import parallel
    c = FC.instance(64, score, "adagrad", 0, False)
    g, n = make(c["opt"], c["Q"]), c["indptr"].shape[0]
    pool = np.arange(FC.ITEMS, dtype=np.int32)
    keys, scores, k2, s2 = (np.zeros((n, 10), t) for t in (np.int32, np.float32, np.int32, np.float32))
    parallel.warp_fold_in_recommend(g, c["indptr"], c["keys"], FC.ITERS, FC.LR, keys, scores, pool, 10, score_func=score)
    rows = g.fold_in(c["indptr"], c["keys"], FC.ITERS, FC.LR)        # zero start rows, as the helper folds
    eng = parallel.TopK()
    eng.set_score_func(score)
    eng.set_seen(c["indptr"], c["keys"], FC.ITEMS)
    eng.recommend_unseen(np.arange(n, dtype=np.int32), rows, c["Q"], parallel.NO_BIAS, k2, s2, pool, 10)
    assert np.array_equal(keys, k2) and np.array_equal(bits(scores), bits(s2))
