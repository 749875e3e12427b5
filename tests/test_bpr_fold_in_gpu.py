"""bfh_bpr_fold_in on the device (csrc/bpr_fold_kernels.hpp behind CyBPR.fold_in) against the float64 restatement of its rule (bpr_fold_cases.py)."""
import numpy as np
import pytest

import bpr_fold_cases as FC
import helpers as H
from conftest import bpr_opt, tiny_csr

pytestmark = pytest.mark.gpu
I64, I32 = (lambda *v: np.array(v, np.int64)), (lambda *v: np.array(v, np.int32))
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)


def make(opt, Q=None, Qb=None, table=None):   # a CyBPR whose item side is (Q, Qb) -- without them: no model yet; P is three rows nobody folds into
    from buffalo_amd.backend import CyBPR
    g = CyBPR()
    assert g.init(H.write_opt(bpr_opt(accelerator=True, **opt)))
    if Q is not None:
        g.initialize_model(np.full((3, g.get_vdim()), 0.1, np.float32), H.pad(Q, g.get_vdim()), Qb.copy(), 10, True)
    if table is not None:
        g.set_cumulative_table(table, table.shape[0])
    return g


def fold(g, c, rows=range(12)):   # fold_in over `rows` of the instance's histories, in that order, under their own row ids
    rows, beg = np.asarray(rows), np.concatenate([[0], c["indptr"]])
    keys = np.concatenate([c["keys"][beg[b]:beg[b + 1]] for b in rows]).astype(np.int32)
    return g.fold_in(np.cumsum(beg[rows + 1] - beg[rows]), keys, FC.ITERS, FC.LR, FC.MIN_LR, row_ids=rows.astype(np.int32), init=np.ascontiguousarray(c["init"][rows]))


@pytest.mark.parametrize("inst", FC.INSTANCES, ids=lambda i: "d%d-bias%d-nn%d-table%d" % i)
def test_parity_against_float64(inst):
    """|p_k - p64_k| <= (5 S_b + 1) 2^-24 M_bk (derived in bpr_fold_cases).  Measured on an MI355X: profiles/bpr_fold_in_first_contact.txt."""
    c = FC.instance(*inst)
    out = fold(make(c["opt"], c["Q"], c["Qb"], c["table"]), c)
    frac = np.abs(out.astype(np.float64) - c["f64"]) / c["bound"]
    print("bpr fold_in parity %s: worst error / bound %.4f (history %d)" % (inst, frac.max(), int(frac.max(axis=1).argmax())))
    assert frac.max() <= 1.0 and np.array_equal(bits(out[0]), bits(c["init"][0]))   # the empty history returns its start row


@pytest.mark.parametrize("inst", [(20, 1, 3, 1), (96, 1, 3, 1), (256, 1, 1, 0)], ids=["G16", "G32", "G64"])
def test_rows_do_not_depend_on_their_batch_or_group(inst):
    """Reversed, split in two, run again: the same bits.  And the dozen 600 times under the same row ids, the launch held to 4 waves per CU, far
    fewer groups than rows: every group takes further rows from the counter (global keys first, LDS keys after, at every phase of the ring)."""
    c = FC.instance(*inst)
    g = make(c["opt"], c["Q"], c["Qb"], c["table"])
    whole = fold(g, c)
    for rows in (range(11, -1, -1), [0, 2, 4, 8, 9], [1, 3, 5, 6, 7, 10, 11], range(12)):
        assert np.array_equal(bits(fold(g, c, rows)), bits(whole[list(rows)]))
    g.set_mode("waves_per_cu", 4)
    many = fold(g, c, np.tile(np.arange(12), 600))
    assert np.array_equal(bits(many).reshape(600, 12, -1), np.broadcast_to(bits(whole), (600, 12, inst[0])))


def test_the_model_and_the_next_epoch_do_not_notice():
    c = FC.instance(64, 1, 1, 0)
    csr = tiny_csr(U=3, I=FC.ITEMS, density=0.02, seed=4)
    state = lambda h: np.concatenate([bits(h.device_tensor(n).cpu().numpy()) for n in ("P", "Q", "Qb")])
    g, twin = (make(c["opt"], c["Q"], c["Qb"]) for _ in range(2))
    before = state(g)
    fold(g, c)
    assert np.array_equal(before, state(g))
    for h in (g, twin):
        h.set_mode("sequential", 1)
        h.set_placeholder(csr.indptr, csr.nnz + 1)
        h.add_jobs(0, 3, csr.indptr, csr.keys)
    assert np.array_equal(state(g), state(twin)) and not np.array_equal(state(g), before)   # the epoch did move the model


def refusal(n_rows=2, indptr=I64(2, 4), keys=I32(1, 5, 2, 9), nnz=4, iters=2, status=-1, model=True, good=True, mass=None, **opt):
    return (n_rows, indptr, keys, nnz, iters), status, model, good, mass, dict(dict(d=20, random_seed=1), **opt)


# a refused call: its arguments, the status, whether a model is bound, whether a good call can go first, the items that carry the table's mass
REFUSALS = {
    "before initialize_model": refusal(model=False, good=False), "negative n_rows": refusal(n_rows=-1), "negative iters": refusal(iters=-1),
    "negative nnz": refusal(nnz=-4), "decreasing indptr": refusal(indptr=I64(4, 2)), "indptr[-1] != nnz": refusal(indptr=I64(2, 3)),
    "null keys": refusal(keys=None), "key below 0": refusal(keys=I32(-1, 5, 2, 9)), "key = num_items": refusal(keys=I32(1, 5, 2, FC.ITEMS)),
    "keys descend": refusal(keys=I32(5, 1, 2, 9)), "a key twice": refusal(keys=I32(1, 1, 2, 9)),
    "every item in a row": refusal(1, I64(FC.ITEMS), np.arange(FC.ITEMS, dtype=np.int32), FC.ITEMS, 1),
    "2^31 steps in a row": refusal(1, I64(900), np.arange(900, dtype=np.int32), 900, 10000, num_negative_samples=255),
    "sampling_power without a table": refusal(good=False, sampling_power=1.0),
    # lower_bound sends the draw 0 to item 0 whatever its weight: only a row that holds item 0 can hold all the mass
    "no table mass outside the row": refusal(1, I64(2), I32(0, 7), 2, 1, mass=(0, 7), sampling_power=1.0),
    "d = 288": refusal(status=-3, good=False, d=288),
}


@pytest.mark.parametrize("name", REFUSALS)
def test_refusals(name):
    """Every refusal of the header, through the C ABI: the status, a message, and the rows of an earlier good call still in "fold"."""
    from buffalo_amd import _lib
    (n_rows, indptr, keys, nnz, iters), status, model, good, mass, opt = REFUSALS[name]
    table = None if mass is None else np.cumsum(np.isin(np.arange(FC.ITEMS), mass) * 5).astype(np.int64)
    g = make(opt, *(FC.model(opt["d"], 1, 0)[:2] if model else (None, None)), table=table)
    if good:
        rows = g.fold_in(I64(1), I32(500), 2, 0.05, 0.01)
        kept = bits(g.device_tensor("fold").cpu().numpy())
        assert np.array_equal(kept[:opt["d"]], bits(rows[0])) and rows.any()
    ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)
    assert _lib.lib().bfh_bpr_fold_in(g._h, n_rows, ptr(indptr, _lib._pi64), ptr(keys, _lib._pi32), nnz, None, iters, 0.05, 0.01, None, None, None) == status
    assert b"fold_in" in _lib.lib().bfh_last_error(g._h)
    assert not good or np.array_equal(bits(g.device_tensor("fold").cpu().numpy()), kept)


def test_recommend_from_the_folded_rows():
    from buffalo_amd import parallel
    c = FC.instance(64, 1, 1, 0)
    g = make(c["opt"], c["Q"], c["Qb"])
    pool = np.arange(FC.ITEMS, dtype=np.int32)
    keys, scores, k2, s2 = (np.zeros((12, 10), t) for t in (np.int32, np.float32, np.int32, np.float32))
    parallel.bpr_fold_in_recommend(g, c["indptr"], c["keys"], FC.ITERS, FC.LR, FC.MIN_LR, keys, scores, pool, 10)
    rows = g.fold_in(c["indptr"], c["keys"], FC.ITERS, FC.LR, FC.MIN_LR)        # zero start rows, as the helper folds
    eng = parallel.TopK()
    eng.set_seen(c["indptr"], c["keys"], FC.ITEMS)
    eng.recommend_unseen(np.arange(12, dtype=np.int32), rows, c["Q"], c["Qb"], k2, s2, pool, 10)
    assert np.array_equal(keys, k2) and np.array_equal(bits(scores), bits(s2))
