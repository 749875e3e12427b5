"""Host logic of the validation evaluator (buffalo_amd/evaluate.py): the ctypes mirror covers the `bfh_eval_*` section of the header,
the mixin routes the reference's three methods through an evaluator, and nothing works without a GPU."""
import numpy as np
import pytest

from conftest import has_gpu


def test_mirror_covers_the_eval_section_of_the_header():
    from buffalo_amd import _lib, evaluate
    names = [n for n in _lib.header_symbols() if n.startswith("bfh_eval_")]
    assert set(names) == {"bfh_eval_" + n for n in ("create", "destroy", "set_device", "set_data", "num_rows", "ranking", "ranking_device", "scores",
                                                    "scores_device", "set_mode", "get_stats", "reset_stats")}
    assert all(n in _lib.SIGNATURES for n in names)
    for method in ("set_data", "num_rows", "ranking", "ranking_device", "scores", "scores_device", "set_mode", "stats", "reset_stats", "set_device"):
        assert callable(getattr(evaluate.Evaluator, method))
    # the five doubles / the lists are the last two arguments of both ranking forms, as the header says
    for n in ("bfh_eval_ranking", "bfh_eval_ranking_device"):
        assert _lib.SIGNATURES[n][1][-2:] == [_lib._pf64, _lib._pi32]


def test_typed_arguments_are_checked_before_the_library_is_reached():
    from buffalo_amd.evaluate import Evaluator
    ev = Evaluator.__new__(Evaluator)           # no handle: the checks below never reach it
    i64, i32, f32 = np.zeros(3, np.int64), np.zeros(3, np.int32), np.zeros(3, np.float32)
    with pytest.raises(ValueError):
        ev.set_data(3, 3, i32, i32, i32, i32, f32)                   # indptr must be int64
    with pytest.raises(ValueError):
        ev.set_data(4, 3, i64, i32, i32, i32, f32)                   # one END offset per user
    with pytest.raises(ValueError):
        ev.set_data(3, 3, i64, i32, i32, i32[:2].copy(), f32)        # vali arrays of one length
    with pytest.raises(ValueError):
        ev.ranking(np.zeros((3, 4), np.float64), np.zeros((3, 4), np.float32))
    with pytest.raises(ValueError):
        Evaluator._bias(np.zeros((2, 1), np.float32), 3)


def test_sample_rows_is_the_reference_draw():
    from buffalo_amd.evaluate import sample_rows
    rows = np.arange(100, dtype=np.int32)
    assert sample_rows(rows, 0) is not None and np.array_equal(sample_rows(rows, 0), rows)
    np.random.seed(5)
    got = sample_rows(rows, 30)
    np.random.seed(5)
    assert np.array_equal(got, np.random.choice(rows, size=30, replace=False))     # evaluate/base.py:58-60
    assert len(sample_rows(rows, 1000)) == 100


def test_mixin_routes_the_three_methods(monkeypatch):
    from buffalo_amd import evaluate

    class Fake:
        calls = []

        def set_data(self, *a):
            Fake.calls.append(("set_data", a[0], a[1]))

        def ranking(self, P, Q, Qb, rows=None, topk=10):
            Fake.calls.append(("ranking", P.shape, Q.shape, Qb is not None, None if rows is None else len(rows), topk))
            return {"ndcg": 0.5, "map": 0.25, "accuracy": 0.75, "auc": 0.9, "N": 0.0 if topk == 99 else 7.0}

        def scores(self, P, Q, Qb):
            Fake.calls.append(("scores", P.shape))
            return {"rmse": 1.5, "error": 1.0}
    monkeypatch.setattr(evaluate, "Evaluator", Fake)

    class Data:
        groups = {"rowwise": {"indptr": np.array([1, 2, 3], np.int64), "key": np.array([0, 1, 0], np.int32)},
                  "vali": {"row": np.array([2, 0, 2], np.int32), "col": np.array([1, 1, 0], np.int32), "val": np.ones(3, np.float32)}}

        def get_header(self):
            return {"num_users": 3, "num_items": 2}

        def get_group(self, name):
            return self.groups[name]

        def has_group(self, name):
            return name in self.groups

    class Opt(dict):
        __getattr__ = dict.get

    class Front(evaluate.DeviceEvaluable):
        pass
    f = Front()
    f.data, f.opt = Data(), Opt(d=4, use_bias=True, validation={"topk": 5})
    f.P, f.Q, f.Qb = np.zeros((3, 32), np.float32), np.zeros((2, 32), np.float32), np.zeros((2, 1), np.float32)
    assert f.get_validation_results() == {"ndcg": 0.5, "map": 0.25, "accuracy": 0.75, "auc": 0.9, "rmse": 1.5, "error": 1.0}
    assert Fake.calls == [("set_data", 3, 2), ("ranking", (3, 4), (2, 4), True, None, 5), ("scores", (3, 4))]      # bound once, factors cut to d
    assert f._evaluate_ranking_metrics(topk=99) == {}                     # N == 0: nothing to report
    f.opt["validation"]["eval_samples"] = 1
    f._evaluate_ranking_metrics()
    assert Fake.calls[-1] == ("ranking", (3, 4), (2, 4), True, 1, 5)        # the draw is made here, over the users with vali entries
    data = Data()
    data.groups = dict(Data.groups)
    del data.groups["vali"]
    f.data = data
    assert f.get_validation_results() == {}


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU failure mode")
def test_no_gpu_fails_loudly():
    from buffalo_amd import _build
    from buffalo_amd._lib import BuffaloHipError
    from buffalo_amd.evaluate import Evaluator
    _build.build()
    with pytest.raises(BuffaloHipError):
        Evaluator()
