"""Word2Vec on the device (csrc/w2v.hip behind bfh_w2v_* / CyW2V) against the numpy restatement of tests/ref_w2v.py.

Integer stage (subsampling, windows, counts): exact.  Float stage: the project's envelope -- the device may be no further from the float64 run than
2.5 x the float32 restatement is, floor 1e-5 (the BPRMF sequential figure) -- on cases whose every dot product is safe (tests/test_w2v_ref_cpu.py
proves that for the same cases), so no dot is left out.  Schedules without conflicts: identical bits.  Hogwild: the planted-stream quality of the
restatement, less its own spread over the seeds."""
import os

import numpy as np
import pytest

import helpers as H
import ref_w2v as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def table():
    from buffalo_amd.backend import CyW2V
    return CyW2V.exp_table()


def _obj(opt, vocab=None, L0=None, L1=None, **modes):
    import torch
    from buffalo_amd.backend import CyW2V
    g = CyW2V()
    path = H.write_opt(opt)
    try:
        assert g.init(path)
    finally:
        os.unlink(path)
    for k, v in modes.items():
        g.set_mode(k, v)
    if vocab is not None:
        g.initialize_model(L0, vocab["index"], vocab["scale"], vocab["dist"], vocab["total_word_count"])
        if L1 is not None:
            g.device_tensor("L1", (L0.shape[0], g.get_vdim()))[:, :L0.shape[1]] = torch.from_numpy(L1).cuda()
            torch.cuda.synchronize()
    return g


def _L1(g, V, d):
    return g.device_tensor("L1", (V, g.get_vdim())).cpu().numpy()[:, :d].copy()


def _feed(g, indptr, seq, batches):
    for a, b in batches:
        beg = 0 if a == 0 else int(indptr[a - 1])
        g.add_jobs(a, b, indptr, np.ascontiguousarray(seq[beg:int(indptr[b - 1])]))


def _run_device(case, batches=None, **modes):
    """launch_workers, the epochs, join -> (L0, L1, loss, stats)"""
    L0 = case["L0"].copy()
    g = _obj(case["opt"], case["vocab"], L0, case["L1"], **modes)
    g.launch_workers()
    for _ in range(case["epochs"]):
        _feed(g, case["indptr"], case["seq"], batches or [(0, len(case["indptr"]))])
    loss = g.join()
    return L0, _L1(g, *L0.shape), loss, g.stats()


def _envelope(name, dev, t64, t32):
    e_dev, e_32 = H.relerr(dev, t64), H.relerr(t32, t64)
    print("%s: relerr device %.3e, float32 restatement %.3e" % (name, e_dev, e_32))
    assert e_dev <= max(2.5 * e_32, 1e-5), (name, e_dev, e_32)


# ------------------------------------------------------------------------------------------------
# integer stage
# ------------------------------------------------------------------------------------------------
def _integer_case():
    counts = np.array([5000] + [20 + 3 * i for i in range(23)] + [1, 1], dtype=np.int64)     # word 0 is hot; words 24, 25 are below min_count
    vocab = R.build_vocab(counts, min_count=2, sample=0.001)
    sents = [[], [3], [0, 0], [24, 5, 25, 6, 7, 24], [2, 9, 10, 11, 12, 13, 14, 15], [], [0, 4, 0, 8, 0, 16, 17], [25], [18, 19, 20, 21, 22, 23, 1, 2], []]
    indptr, seq = R.make_stream(sents)
    vocab["total_word_count"] = int(seq.shape[0])
    opt = {"d": 20, "window": 3, "num_negative_samples": 2, "num_iters": 2, "lr": 0.05, "min_lr": 0.01, "random_seed": 5, "batch_size": 8,
           "compute_loss_on_training": False, "num_workers": 1}
    return opt, vocab, sents, indptr, seq


@pytest.mark.parametrize("n_batches", [1, 3])
def test_integer_stage_is_exact(table, n_batches):
    opt, vocab, sents, indptr, seq = _integer_case()
    L0 = R.init_L0(1, vocab["size"], opt["d"])
    ref = R.Trainer(opt, vocab, L0, table, np.float64, fast=True)
    g = _obj(opt, vocab, L0.copy(), sequential=1)
    g.launch_workers()
    batches = R.uneven_batches(len(sents), n_batches)
    assert len(batches) == n_batches
    seen = {"nothing_left": False, "one_word": False, "oov": False, "clipped_left": False, "clipped_right": False}
    for epoch in range(2):
        for a, b in batches:
            _feed(g, indptr, seq, [(a, b)])
            ref.add_jobs(a, b, indptr, seq)
            shifted = 0 if a == 0 else int(indptr[a - 1])
            if int(indptr[b - 1]) == shifted:          # a batch of empty rows: nothing is queued, there are no buffers to read
                assert g.device_buffer("kept")[1] == 0 and g.device_buffer("sent_end")[1] == 0
                continue
            kept, kept_pos, window_b, sent_end = (g.device_tensor(n).cpu().numpy() for n in ("kept", "kept_pos", "window_b", "sent_end"))
            assert kept.shape[0] == int(indptr[b - 1]) - shifted and sent_end.shape[0] == b - a
            for s in range(a, b):
                kb = (0 if s == 0 else int(indptr[s - 1])) - shifted
                ke = int(sent_end[s - a])
                want = [ref.last[k][s - a] for k in ("kept", "kept_pos", "window_b")]
                assert kept[kb:ke].tolist() == want[0], (epoch, s)
                assert kept_pos[kb:ke].tolist() == want[1], (epoch, s)
                assert window_b[kb:ke].tolist() == want[2], (epoch, s)
                n, w = len(want[0]), opt["window"]
                seen["nothing_left"] |= len(sents[s]) > 0 and n == 0 and all(vocab["index"][x] for x in sents[s])
                seen["one_word"] |= len(sents[s]) == 1 and n == 1
                seen["oov"] |= any(vocab["index"][x] == 0 for x in sents[s]) and n > 0
                seen["clipped_left"] |= any(i - w + want[2][i] < 0 for i in range(n))
                seen["clipped_right"] |= any(i + w + 1 - want[2][i] > n for i in range(n))
    st = g.stats()
    print({k: st[k] for k in ref.stats}, seen)
    assert {k: st[k] for k in ref.stats} == ref.stats
    assert st["samples"] > 0 and st["loaded_rows"] > 0 and st["accepted"] < 2 * seq.shape[0]
    assert all(seen.values()), seen          # the case holds what it is there for (an empty row is in `sents` itself)


# ------------------------------------------------------------------------------------------------
# float stage, sequential
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_neg", R.PARITY_NEGS)
@pytest.mark.parametrize("d", R.PARITY_DIMS)
def test_sequential_parity(table, d, num_neg):
    case = R.parity_case(d, num_neg)
    t64, t32 = R.run_case(case, table, np.float64), R.run_case(case, table, np.float32)
    assert t64.unsafe == 0 and t32.stats == t64.stats
    L0, L1, loss, st = _run_device(case, sequential=1)
    assert {k: st[k] for k in t64.stats} == t64.stats
    tag = "d=%d neg=%d epochs=%d dots=%d" % (d, num_neg, case["epochs"], t64.dots)
    _envelope(tag + " L0", L0, t64.L0, t32.L0)
    _envelope(tag + " L1", L1, t64.L1, t32.L1)
    _envelope(tag + " loss", loss, t64.loss, t32.loss)


@pytest.mark.parametrize("atomic", [1, 0])
@pytest.mark.parametrize("d", sorted(R.PAIRS_SEEDS))
def test_update_pairs(table, d, atomic):
    case = R.pairs_case(d)
    t64, t32 = R.run_pairs_case(case, table, np.float64), R.run_pairs_case(case, table, np.float32)
    assert t64.unsafe == 0
    L0 = case["L0"].copy()
    g = _obj(case["opt"], case["vocab"], L0, case["L1"], hogwild_atomic=atomic)
    g.update_pairs(case["inputs"], case["outputs"], case["alpha"])
    g.synchronize(True)
    _envelope("pairs d=%d L0" % d, L0, t64.L0, t32.L0)
    _envelope("pairs d=%d L1" % d, _L1(g, *L0.shape), t64.L1, t32.L1)
    assert not np.array_equal(L0, case["L0"])


def test_split_into_batches_changes_no_bit(table):
    """With lr == min_lr every job has the same alpha; the draws hang on global positions: one batch and three uneven ones give the same model."""
    case = R.parity_case(20, 2)
    case["opt"] = dict(case["opt"], min_lr=case["opt"]["lr"])
    one = _run_device(case, sequential=1)
    three = _run_device(case, R.uneven_batches(len(case["indptr"]), 3), sequential=1)
    assert np.array_equal(one[0], three[0]) and np.array_equal(one[1], three[1])
    assert {k: one[3][k] for k in ("samples", "accepted", "loaded_rows")} == {k: three[3][k] for k in ("samples", "accepted", "loaded_rows")}
    assert abs(one[2] - three[2]) <= 1e-12 * abs(one[2])      # the same terms, added per call
    assert not np.array_equal(one[0], case["L0"])


@pytest.mark.parametrize("atomic", [1, 0])
@pytest.mark.parametrize("d", [20, 128, 200])
def test_without_conflicts_hogwild_is_sequential_bit_for_bit(d, atomic):
    """Sentences over disjoint vocabularies, no negatives, a sentence per work item: concurrent groups never touch the same row."""
    rng = np.random.default_rng(d)
    sents = [[int(4 * s + w) for w in rng.integers(0, 4, size=8)] for s in range(12)]
    indptr, seq = R.make_stream(sents)
    vocab = R.build_vocab(np.bincount(seq, minlength=48) + 1, 1, 0.0)      # every word is in the vocabulary, nothing is subsampled
    vocab["total_word_count"] = int(seq.shape[0])
    assert vocab["size"] == 48
    opt = {"d": d, "window": 3, "num_negative_samples": 0, "num_iters": 2, "lr": 0.05, "min_lr": 0.01, "random_seed": 3, "batch_size": 16,
           "compute_loss_on_training": True, "num_workers": 1}
    case = {"opt": opt, "vocab": vocab, "indptr": indptr, "seq": seq, "epochs": 2,
            "L0": rng.normal(scale=0.1, size=(48, d)).astype(np.float32), "L1": rng.normal(scale=0.1, size=(48, d)).astype(np.float32)}
    seq_run = _run_device(case, sequential=1, hogwild_atomic=atomic, chunk=0)
    hog_run = _run_device(case, sequential=0, hogwild_atomic=atomic, chunk=0)
    assert np.array_equal(seq_run[0], hog_run[0]) and np.array_equal(seq_run[1], hog_run[1])
    assert seq_run[2] == hog_run[2] and seq_run[3]["samples"] == hog_run[3]["samples"] > 0
    assert not np.array_equal(seq_run[0], case["L0"])


# ------------------------------------------------------------------------------------------------
# Hogwild quality on a planted stream
# ------------------------------------------------------------------------------------------------
QUALITY_SEEDS = (0, 1, 2, 3, 4)


def _quality_case(seed):
    sents = R.planted_stream(seed)
    indptr, seq = R.make_stream(sents)
    vocab = R.vocab_of_stream(seq, 64)
    opt = {"d": 20, "window": 5, "num_negative_samples": 5, "num_iters": 1, "lr": 0.05, "min_lr": 0.005, "random_seed": seed, "batch_size": -1,
           "compute_loss_on_training": False, "num_workers": 1}
    return {"opt": opt, "vocab": vocab, "indptr": indptr, "seq": seq, "epochs": 1, "L0": R.init_L0(seed, 64, 20), "L1": None}


@pytest.fixture(scope="module")
def restatement_quality(table):
    out = []
    for seed in QUALITY_SEEDS:
        c = _quality_case(seed)
        assert c["vocab"]["size"] == 64
        out.append(R.group_share(R.train(c["opt"], c["vocab"], c["indptr"], c["seq"], c["L0"], table, np.float64, None, 1, fast=True).L0))
    return out


def test_hogwild_quality_on_a_planted_stream(restatement_quality):
    """The default schedule and the default "hogwild_atomic" (1, atomic adds): all 200 sentences are in flight at once.
    Measured on an MI355X: device mean 0.9875 against the restatement's 0.9906 with a spread of 0.0312.  "hogwild_atomic" = 0 (plain stores,
    colliding updates are lost) reached 0.9469 on this stream -- below the bound, which is why it is not the default (profiles/w2v_first_contact.txt)."""
    ref = restatement_quality
    assert np.mean(ref) >= 0.5, ref            # otherwise the case is too weak to tell anything
    dev = []
    for seed in QUALITY_SEEDS:
        L0 = _run_device(_quality_case(seed))[0]
        assert np.isfinite(L0).all()
        dev.append(R.group_share(L0))
    print("device %s mean %.4f; restatement %s mean %.4f spread %.4f" % (dev, np.mean(dev), ref, np.mean(ref), max(ref) - min(ref)))
    assert np.mean(dev) >= np.mean(ref) - (max(ref) - min(ref)), (dev, ref)


# ------------------------------------------------------------------------------------------------
# refusals and call order
# ------------------------------------------------------------------------------------------------
def _base_opt(**kw):
    return dict({"d": 20, "window": 5, "num_negative_samples": 5, "num_iters": 1, "lr": 0.025, "min_lr": 0.001, "random_seed": 1, "batch_size": -1}, **kw)


def _tiny_vocab(V):
    return {"index": np.arange(1, V + 1, dtype=np.int32), "scale": np.full(V, 0xFFFFFFFF, dtype=np.uint32),
            "dist": np.linspace(100, 0x7FFFFFFF, V).astype(np.int32), "total_word_count": 10}


def test_refusals():
    from buffalo_amd._lib import BuffaloHipError
    with pytest.raises(BuffaloHipError, match=r"window > 127.*status -1"):
        _obj(_base_opt(window=128))
    _obj(_base_opt(window=127))
    with pytest.raises(BuffaloHipError, match=r"d > 256.*status -3"):
        _obj(_base_opt(d=257))
    _obj(_base_opt(d=256))
    v1 = _tiny_vocab(1)
    with pytest.raises(BuffaloHipError, match=r"at least 2 words.*status -1"):
        _obj(_base_opt(), v1, np.zeros((1, 20), np.float32))
    _obj(_base_opt(num_negative_samples=0), v1, np.zeros((1, 20), np.float32))       # no negatives: one word is a vocabulary
    v = _tiny_vocab(6)
    v["dist"][3] = v["dist"][2] - 1
    with pytest.raises(BuffaloHipError, match=r"non-decreasing.*status -1"):
        _obj(_base_opt(), v, np.zeros((6, 20), np.float32))
    g = _obj(_base_opt())
    with pytest.raises(BuffaloHipError, match="unknown mode"):
        g.set_mode("no_such_mode", 1)
    with pytest.raises(BuffaloHipError, match="unknown device buffer"):
        g.device_buffer("Q")


def test_call_order():
    from buffalo_amd._lib import BuffaloHipError
    v = _tiny_vocab(6)
    indptr, seq = R.make_stream([[0, 1, 2, 3], [4, 5]])
    g = _obj(_base_opt())
    with pytest.raises(BuffaloHipError, match="before initialize_model"):
        g.launch_workers()
    L0 = R.init_L0(0, 6, 20)
    g = _obj(_base_opt(), v, L0)
    with pytest.raises(BuffaloHipError, match="add_jobs before launch_workers"):
        g.add_jobs(0, 2, indptr, seq)
    with pytest.raises(BuffaloHipError, match="join before launch_workers"):
        g.join()
    g.launch_workers()
    g.add_jobs(0, 2, indptr, seq)
    with pytest.raises(BuffaloHipError, match="outside"):
        g.add_jobs(0, 2, indptr, np.array([0, 1, 2, 6, 4, 5], dtype=np.int32))      # a word the index does not cover
    assert g.join() == 0.0                                                             # compute_loss_on_training is off
    with pytest.raises(BuffaloHipError, match="add_jobs before launch_workers"):
        g.add_jobs(0, 2, indptr, seq)
    assert g.stats()["samples"] > 0 and np.isfinite(L0).all()
