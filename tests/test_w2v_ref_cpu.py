"""Word2Vec without a GPU: the ABI is declared, exported and mirrored; the library's sigmoid table; the restatement (tests/ref_w2v.py) against
hand cases of the job rule and the learning-rate schedule, against the reference's own vocabulary (tests/golden/w2v_vocab_*.npz) and against
itself (vector draws = scalar draws); and the condition the GPU parity tests rest on: EVERY dot product of EVERY parity case is safe, so no dot has
to be left out of the comparison on the device."""
import ctypes as C
import os

import numpy as np
import pytest

import ref_numpy as rn
import ref_w2v as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

W2V_ABI = ["create", "destroy", "set_device", "init", "get_vdim", "initialize_model", "launch_workers", "add_jobs", "join", "synchronize", "set_mode",
           "device_buffer", "stream", "get_stats", "reset_stats", "exp_table", "update_pairs"]


@pytest.fixture(scope="module")
def table():
    from buffalo_amd import _build
    from buffalo_amd.backend import CyW2V
    _build.build()
    return CyW2V.exp_table()       # host-only call


def test_abi_is_declared_exported_and_mirrored():
    from buffalo_amd import _build, _lib
    L = C.CDLL(_build.build())
    names = ["bfh_w2v_" + n for n in W2V_ABI]
    assert [n for n in _lib.header_symbols() if n.startswith("bfh_w2v_")] == sorted(names)
    assert all(hasattr(L, n) for n in names)
    assert all(n in _lib.SIGNATURES for n in names)
    from buffalo_amd.backend import CyW2V
    for m in ("init", "initialize_model", "launch_workers", "add_jobs", "join", "release", "update_pairs", "device_tensor"):
        assert callable(getattr(CyW2V, m))


def test_table_is_the_reference_expression(table):
    i = np.arange(1000, dtype=np.float32)
    e = np.exp(((i / np.float32(1000) * np.float32(2) - np.float32(1)) * np.float32(6)).astype(np.float64)).astype(np.float32)
    want = e / (e + np.float32(1))
    assert table.dtype == np.float32 and table.shape == (1000,)
    assert (np.abs(table.astype(np.float64) - want.astype(np.float64)) <= np.spacing(want)).all()
    assert table[0] < 0.0025 and abs(table[500] - 0.5) < 1e-7 and table[999] > 0.9974 and (np.diff(table) > 0).all()


def test_job_rule_hand_cases():
    # a sentence that overflows the job closes it and opens the next one
    assert R.cut_jobs([3, 4, 5, 2], 8) == [[0, 1], [2, 3]]
    # ... even when it is larger than batch_size on its own; the first overflow queues the (empty) job before it
    assert R.cut_jobs([9, 1, 1], 8) == [[], [0], [1, 2]]
    # the size that fits exactly stays in the job
    assert R.cut_jobs([4, 4, 1], 8) == [[0, 1], [2]]
    # empty sentences belong to no job
    assert R.cut_jobs([0, 2, 0, 2, 0], 10) == [[1, 3]]
    assert R.cut_jobs([0, 0], 10) == []
    # batch_size 0 (a missing key): one sentence per job, after one empty job
    assert R.effective_batch_size({}) == 0 and R.effective_batch_size({"batch_size": 0}) == 0
    assert R.cut_jobs([2, 3, 1], 0) == [[], [0], [1], [2]]
    # batch_size -1 -> 10000
    assert R.effective_batch_size({"batch_size": -1}) == 10000 and R.effective_batch_size({"batch_size": -7}) == 10000
    assert R.cut_jobs([6000, 4000, 1], R.effective_batch_size({"batch_size": -1})) == [[0, 1], [2]]


def test_alpha_schedule():
    lr, lo = 0.025, 0.001
    assert R.alpha_at(0, 100, 2, lr, lo) == lr
    assert R.alpha_at(50, 100, 2, lr, lo) == lr - (lr - lo) * 0.25
    assert R.alpha_at(200, 100, 2, lr, lo) == pytest.approx(lo, abs=1e-18) and R.alpha_at(200, 100, 2, lr, lo) >= lo
    assert R.alpha_at(10 ** 6, 100, 2, lr, lo) == lo          # the floor
    # a run: a job's alpha is the schedule at the words of all EARLIER jobs, counted before subsampling
    sents = [[0, 1, 2], [3], [0, 1, 2, 3, 0], [1, 2]]
    indptr, seq = R.make_stream(sents)
    vocab = R.vocab_of_stream(seq, 4)
    opt = {"d": 4, "window": 2, "num_negative_samples": 0, "num_iters": 1, "lr": lr, "min_lr": lo, "random_seed": 0, "batch_size": 4}
    seen = []

    class Spy(R.Trainer):
        def update_pair(self, inp, outs, alpha):
            seen.append(alpha)
    t = Spy(opt, vocab, np.zeros((4, 4), np.float32), np.zeros(1000, np.float32))
    t.add_jobs(0, 4, indptr, seq)
    jobs = R.cut_jobs([3, 1, 5, 2], 4)
    assert jobs == [[0, 1], [2], [3]]
    want = [R.alpha_at(p, 11, 1, lr, lo) for p in (0, 4, 9)]
    assert sorted(set(seen), reverse=True) == want and t.processed == 11
    assert t.processed // vocab["total_word_count"] == 1       # the next call draws with epoch 1


def test_vector_draws_equal_scalar_draws():
    pos = np.array([0, 5, 2 ** 33 + 7, 123456])
    slot = np.array([0, 3, 254, 17])
    att = np.array([0, 1 << 16, (4 << 16) | 3, 9])
    got = R._o0_many(7, R.STREAM_NEG, pos, slot, 3, att)
    assert [int(x) for x in got] == [rn.counter_draw(7, R.STREAM_NEG, int(p), int(s), 3, int(a))[0] for p, s, a in zip(pos, slot, att)]
    vocab = R.vocab_of_stream(np.array([0, 0, 0, 0, 0, 0, 1, 2], dtype=np.int32), 3)
    many, redraws = R.negatives_many(vocab, 3, 1, [4, 9, 11], [1, 2, 5], [0, 0, 1], 4)
    one = [R.negatives(vocab, 3, 1, p, s, t, 4) for p, s, t in zip([4, 9, 11], [1, 2, 5], [0, 0, 1])]
    assert many.tolist() == [w for w, _ in one] and redraws == sum(r for _, r in one) and redraws > 0
    assert all(w != t for row, t in zip(many.tolist(), [0, 0, 1]) for w in row)


@pytest.mark.parametrize("name", ["w2v_vocab_small", "w2v_vocab_no_sample"])
def test_vocabulary_is_the_references(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    v = R.build_vocab(z["counts"], int(z["min_count"]), float(z["sample"]))
    for k in ("index", "scale", "dist"):
        assert v[k].dtype == z[k].dtype and np.array_equal(v[k], z[k]), k
    assert v["total_word_count"] == int(z["total_word_count"]) and v["size"] == z["scale"].shape[0]
    assert (np.diff(v["dist"].astype(np.int64)) >= 0).all() and abs(int(v["dist"][-1]) - 0x7FFFFFFF) < 3


@pytest.mark.parametrize("d", R.PARITY_DIMS)
@pytest.mark.parametrize("num_neg", R.PARITY_NEGS)
def test_every_dot_of_the_parity_cases_is_safe(table, d, num_neg):
    case = R.parity_case(d, num_neg)
    t = R.run_case(case, table, np.float64)
    print("d=%d neg=%d: %d dots, %d unsafe, V=%d, %s" % (d, num_neg, t.dots, t.unsafe, case["vocab"]["size"], t.stats))
    assert t.unsafe == 0
    assert 30 <= t.dots <= 500                                  # the dot budget of the issue
    assert 20 <= case["vocab"]["size"] <= 26
    words = case["seq"].shape[0] * case["epochs"]
    assert t.stats["accepted"] < words and (case["vocab"]["index"][case["seq"]] == 0).any()    # subsampling and OOV words take part


@pytest.mark.parametrize("d", sorted(R.PAIRS_SEEDS))
def test_every_dot_of_the_explicit_pairs_is_safe(table, d):
    case = R.pairs_case(d)
    t = R.run_pairs_case(case, table, np.float64)
    assert t.unsafe == 0 and t.dots == case["outputs"].size
    # the case holds what it is there for: a repeated output row, a dot above 6 and one below -6
    assert any(len(set(r)) < len(r) for r in case["outputs"].tolist())
    l0 = case["L0"][0].astype(np.float64)
    assert case["L1"][1].astype(np.float64) @ l0 > 6.5 and case["L1"][2].astype(np.float64) @ l0 < -6.5
