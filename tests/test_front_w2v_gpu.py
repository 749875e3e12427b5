"""Word2Vec end to end through the buffalo-compatible front (tests/front_harness/buffalo_front/algo/w2v.py): a stream file -> vocabulary ->
training on the device -> get_feature / most_similar.  Yardsticks: the vocabulary restated in tests/ref_w2v.py (itself held to the reference's
arrays by tests/golden/w2v_vocab_*.npz), the SAME front driving the float64 restatement, and the reference's own test07_oov_by_mincut."""
import os

import numpy as np
import pytest

import ref_w2v as R

pytestmark = pytest.mark.gpu

SEEDS = (1, 2, 3)


def _stream_files(tmp_path, sents, names):
    main, iid = str(tmp_path / "main"), str(tmp_path / "iid")
    with open(main, "w") as f:
        f.write("".join(" ".join(names[w] for w in s) + "\n" for s in sents))
    with open(iid, "w") as f:
        f.write("".join(n + "\n" for n in names))
    return main, iid


def _front(tmp_path, sents, names, backend=None, **kw):
    from buffalo_front.algo import w2v as M
    from buffalo_front.data import StreamOptions
    data_opt = StreamOptions().get_default_option()
    data_opt.input.main, data_opt.input.iid = _stream_files(tmp_path, sents, names)
    data_opt.data.internal_data_type = "stream"          # one record per event, order kept: the reference's default layout
    data_opt.data.validation = {}
    opt = M.W2VOption().get_default_option()
    opt.update(kw)
    cls = M.W2V if backend is None else type("W2VOn" + backend.__name__, (M.W2V,), {"backend": backend})
    m = cls(opt, data_opt=data_opt)
    m.initialize()
    return m


def _share(m, names, groups=8):
    """group_share over the WORDS (w % groups), through the front's own get_feature."""
    return R.group_share(np.stack([m.get_feature(n) for n in names]), groups)


def test_planted_stream_end_to_end(tmp_path):
    names = ["w%02d" % i for i in range(64)]
    dev, ref = [], []
    for seed in SEEDS:
        sents = R.planted_stream(seed)
        kw = dict(d=20, num_iters=1, min_count=1, sample=0.0, lr=0.05, min_lr=0.005, random_seed=seed, batch_size=-1)
        m = _front(tmp_path, sents, names, **kw)
        # the vocabulary the front hands to the device is the restated one, bit for bit
        _, seq = R.make_stream(sents)
        want = R.vocab_of_stream(seq, 64, 1, 0.0)
        for k in ("index", "scale", "dist"):
            assert np.array_equal(m._vocab[k], want[k]) and m._vocab[k].dtype == want[k].dtype
        assert m._vocab.total_word_count == seq.shape[0] and m.L0.shape == (64, 20)
        L0 = m.L0.copy()
        m.batch_rows = 70                                  # three uneven batches
        assert m.train() == {}
        assert np.isfinite(m.L0).all() and not np.array_equal(m.L0, L0)
        st = m.obj.stats()
        assert st["accepted"] == seq.shape[0] and st["samples"] > 4 * seq.shape[0] and st["scored_negatives"] == 5 * st["samples"]
        dev.append(_share(m, names))
        r = _front(tmp_path, sents, names, R.RefW2V, **kw)
        r.L0[:] = L0
        r.obj.t.L0[:] = L0                                 # the same start
        r.batch_rows = 70
        r.train()
        ref.append(_share(r, names))
        if seed == SEEDS[0]:                               # most_similar agrees with the features it is computed from
            top = m.most_similar("w05", topk=3)
            X = m.L0 / np.linalg.norm(m.L0, axis=1, keepdims=True)
            cos = X @ X[m.get_index("w05")]
            order = [i for i in np.argsort(-cos) if i != m.get_index("w05")][:3]
            assert [k for k, _ in top] == [names[int(m._vocab.inv_index[i])] for i in order]
            np.testing.assert_allclose([s for _, s in top], cos[order], rtol=1e-5)
            assert m.most_similar("no such word") == []
    print("planted stream through the front: device %s, float64 front %s" % (dev, ref))
    assert np.mean(ref) >= 0.5, ref
    # Hogwild may claim the restatement's own seed noise and nothing more (the bound of tests/test_w2v_gpu.py)
    assert np.mean(dev) >= np.mean(ref) - (max(ref) - min(ref)), (dev, ref)


def test_oov_by_mincut(tmp_path):
    """tests/algo/test_w2v.py:test07_oov_by_mincut of the reference: the word below min_count has no feature."""
    from buffalo_front.algo import w2v as M
    from buffalo_front.data import StreamOptions
    opt = M.W2VOption().get_default_option()
    opt.update(num_iters=5, num_workers=1, d=10, min_count=2)
    data_opt = StreamOptions().get_default_option()
    main, iid = str(tmp_path / "main"), str(tmp_path / "iid")
    with open(main, "w") as f:
        f.write("1 2 1 2 1 2 1 2\n3\n")
    with open(iid, "w") as f:
        f.write("1\n2\n3\n")
    data_opt.input.main, data_opt.input.iid = main, iid
    data_opt.data.internal_data_type = "stream"
    model = M.W2V(opt, data_opt=data_opt)
    model.initialize()
    model.train()
    for k in ["1", "2", "3"]:
        vec = model.get_feature(k)
        if k == "3":
            assert vec is None
        else:
            assert isinstance(vec, np.ndarray) and vec.shape == (10,) and np.isfinite(vec).all()
    assert model.L0.shape == (2, 10) and model.most_similar("3") == []


def test_save_and_load(tmp_path):
    from buffalo_front.algo import w2v as M
    names = ["w%02d" % i for i in range(64)]
    m = _front(tmp_path, R.planted_stream(9, num_sents=20), names, d=20, num_iters=1, min_count=2, random_seed=3)
    m.train()
    path = str(tmp_path / "w2v.bin")
    m.save(path)
    back = M.W2V.instantiate(M.W2VOption, path)
    assert back.L0.tobytes() == m.L0.tobytes() and np.array_equal(back._vocab.index, m._vocab.index) and back.opt.d == 20
    some = names[int(m._vocab.inv_index[0])]
    assert np.array_equal(back.get_feature(some), m.get_feature(some))


def test_compiled_binding_equals_the_ctypes_mirror():
    """integration/buffalo/algo/hip/_w2v.pyx and buffalo_amd.backend.CyW2V drive one library: in sequential mode the same bits."""
    import sys
    import helpers as H
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "integration"))
    import build_binding
    build_binding.build()
    from buffalo_amd.backend import CyW2V
    case = R.parity_case(20, 2)
    out = []
    for cls in (build_binding.import_w2v(), CyW2V):
        L0 = case["L0"].copy()
        g = cls()
        path = H.write_opt(case["opt"])
        assert g.init(path) is True
        os.unlink(path)
        g.set_mode("sequential", 1)
        g.initialize_model(L0, case["vocab"]["index"], case["vocab"]["scale"], case["vocab"]["dist"], case["vocab"]["total_word_count"])
        g.launch_workers()
        for _ in range(case["epochs"]):
            g.add_jobs(0, len(case["indptr"]), case["indptr"], case["seq"])
        out.append((L0, g.join()))
        assert g.release() is None
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1] == out[1][1] != 0.0
    assert not np.array_equal(out[0][0], case["L0"])
    with pytest.raises(RuntimeError, match="add_jobs before launch_workers"):
        g2 = build_binding.import_w2v()()
        path = H.write_opt(case["opt"])
        assert g2.init(path)
        os.unlink(path)
        g2.initialize_model(case["L0"].copy(), case["vocab"]["index"], case["vocab"]["scale"], case["vocab"]["dist"], 10)
        g2.add_jobs(0, 1, case["indptr"], case["seq"])
