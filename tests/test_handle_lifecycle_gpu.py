"""The lifecycle every handle kind shares (csrc/abi.hpp): a fresh handle may be given a device, a handle that has allocated stays on the
device it lives on and refuses any other one -- before any HIP call, so one GPU is enough -- without being changed by the refusal; stats
come with every key and reset to zero; a destroyed handle leaves nothing behind that keeps a second one from working."""
import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

D = 8


def _trainer(cls, opt):
    """(fresh object, place, one further cheap call): `init` creates the stream and the option-sized buffers."""
    obj = cls()
    path = H.write_opt(opt)

    def init():
        assert obj.init(path)
    return obj, init, init


def _bpr():
    from conftest import bpr_opt
    from buffalo_amd.backend import CyBPR
    return _trainer(CyBPR, bpr_opt(d=D))


def _warp():
    from conftest import warp_opt
    from buffalo_amd.backend import CyWARP
    return _trainer(CyWARP, warp_opt(d=D))


def _als():
    from conftest import als_opt
    from buffalo_amd.backend import CyALS
    return _trainer(CyALS, als_opt(d=D))


def _cfr():
    import cfr_cases as CC
    from buffalo_amd.backend import CyCFR
    return _trainer(CyCFR, CC.opt(D, "llt"))


def _eals():
    import eals_cases as EC
    from buffalo_amd.backend import CyEALS
    return _trainer(CyEALS, EC.opt(D))


def _plsi():
    from buffalo_amd.backend import CyPLSI
    return _trainer(CyPLSI, {"d": D, "random_seed": 0, "num_workers": 1, "num_iters": 10, "alpha1": 1.0, "alpha2": 1.0, "eps": 1e-10})


def _w2v():
    from buffalo_amd.backend import CyW2V
    return _trainer(CyW2V, {"d": D, "window": 5, "num_negative_samples": 5, "num_iters": 1, "lr": 0.025, "min_lr": 0.001, "random_seed": 1,
                            "batch_size": -1})


def _topk():
    from buffalo_amd.parallel import TopK
    rng = np.random.default_rng(5)
    P, Q = rng.normal(size=(6, 4)).astype(np.float32), rng.normal(size=(9, 4)).astype(np.float32)
    idx, Qb, pool = np.arange(6, dtype=np.int32), np.zeros((0, 0), np.float32), np.zeros(0, np.int32)
    want = np.argsort(-(P.astype(np.float64) @ Q.astype(np.float64).T), axis=1, kind="stable")[:, :3]
    obj = TopK()

    def rank():
        keys, scores = np.empty((6, 3), np.int32), np.empty((6, 3), np.float32)
        obj.dot_topn(idx, P, Q, Qb, keys, scores, pool, 3)
        assert np.array_equal(keys, want)
    return obj, rank, rank


def _eval():
    import eval_cases as ec
    from buffalo_amd.evaluate import Evaluator
    train, vali, _, _, _ = ec.planted(d=20, seed=16)
    obj = Evaluator()

    def bind():
        obj.set_data(train.num_users, train.num_items, train.indptr, train.keys, vali["row"], vali["col"], vali["val"])

    def rows():
        assert obj.num_rows() == np.unique(vali["row"]).shape[0]
    return obj, bind, rows


def _stream():
    from buffalo_amd.ingest import StreamBuilder
    obj = StreamBuilder()

    def build():
        obj.set_vocabulary(["apple", "mango", "pie", "juice", "coke", "grape"])
        res = obj.build(b"apple mango mango apple pie juice coke\npie\njuice coke grape", vali_n=1)
        assert res.events()[0].tolist() == [6, 7, 9]
    return obj, build, build


def _mm():
    from buffalo_amd.ingest import MatrixMarketBuilder
    obj = MatrixMarketBuilder()

    def build():
        mm = obj.build(b"%%MatrixMarket matrix coordinate integer general\n%\n%\n5 3 5\n1 1 1\n2 1 3\n3 3 1\n4 2 1\n5 2 2")
        assert mm.group(1)["indptr"].tolist() == [1, 2, 3, 4, 5]
    return obj, build, build


KINDS = {"CyBPR": _bpr, "CyWARP": _warp, "CyALS": _als, "CyCFR": _cfr, "CyEALS": _eals, "CyPLSI": _plsi, "CyW2V": _w2v, "TopK": _topk,
         "Evaluator": _eval, "StreamBuilder": _stream, "MatrixMarketBuilder": _mm}


@pytest.mark.parametrize("kind", list(KINDS))
def test_one_lifecycle_for_every_kind(kind):
    from buffalo_amd._lib import BuffaloHipError, Stats
    obj, place, further = KINDS[kind]()
    obj.set_device(0)                     # a fresh handle may be placed
    place()
    obj.set_device(0)                      # the device it lives on: nothing to move
    with pytest.raises(BuffaloHipError, match="create a new handle"):
        obj.set_device(1)
    further()                              # the refused call left the handle as it was
    stats = obj.stats()
    assert set(stats) == {name for name, _ in Stats._fields_}
    obj.reset_stats()
    stats = obj.stats()
    assert stats["launches"] == 0 and stats["samples"] == 0
    del obj, place, further
    again, place, _ = KINDS[kind]()
    place()
    assert set(again.stats()) == {name for name, _ in Stats._fields_}
