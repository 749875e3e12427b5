"""Golden L2 scores, made by the REFERENCE's own `WARP` methods with `score_func` forced to "L2" (TEST INFRASTRUCTURE).

    python tests/golden/make_l2_vectors.py [--out FILE]        # needs /root/reference; default: tests/golden/l2_vectors.npz

`buffalo/algo/warp.py` is imported unchanged from where the reference lies (make_front_traces.install_reference supplies the compiled
modules this image lacks).  `WARP._get_topk_recommendation` (warp.py:94-107), `_get_most_similar_L2` (:115-136) and `_get_scores`
(:145-150) are called unbound on a stub -- a `WARP` made without `__init__` that carries only P, Q and `opt.score_func = "L2"` (the
spelling the methods compare with; through `WARP.__init__` the option would be lower-cased and the dot branch taken, SURVEY Q-23).  The one
compiled function they reach, `parallel._core.quickselect`, is stood in for by a stable numpy argsort that also keeps the score matrix it
was given: the scores are the reference's, the order of equal scores is the stand-in's and is not stored for ties (there are none here).
The inputs are rebuilt by tests/l2_cases.golden_input(d) -- seed 9100 + d -- so only the seeds and the reference's OUTPUT are stored."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import l2_cases as lc  # noqa: E402
import make_front_traces as G  # noqa: E402

OUT = os.path.join(HERE, "l2_vectors.npz")
TOPK = 10


def reference_outputs():
    G.install_reference()
    import buffalo.evaluate.base as evaluate_base
    from buffalo.algo.warp import WARP
    from buffalo.misc import aux

    seen_scores = []

    def quickselect(scores, result, sorted, num_threads):
        seen_scores.append(np.array(scores, copy=True))
        result[:] = np.argsort(-scores, axis=1, kind="stable")[:, :result.shape[1]]
    evaluate_base.quickselect = quickselect

    out = {"ds": np.array(lc.DS, np.int32), "seeds": np.array([9100 + d for d in lc.DS], np.int32), "numpy": np.array(np.__version__)}
    for d in lc.DS:
        P, Q, rows, cols = lc.golden_input(d)
        stub = WARP.__new__(WARP)
        stub.P, stub.Q = P, Q
        stub.opt = aux.Option({"score_func": "L2", "num_workers": 1})
        users = np.arange(P.shape[0])
        del seen_scores[:]
        lists = np.array([t for _, t in WARP._get_topk_recommendation(stub, users, TOPK)], dtype=np.int32)
        neg = seen_scores[-1]                                  # -((p - q) ** 2).sum(-1), warp.py:99
        assert neg.dtype == np.float32 and neg.shape == (P.shape[0], Q.shape[0]) and lists.shape == (P.shape[0], TOPK)
        sim_keys, sim_dist = [], []
        for item in range(4):                                  # index queries: topk + 1 entries, the item itself first (warp.py:121)
            t, s = WARP._get_most_similar_L2(stub, item, TOPK, None)
            assert t[0] == item and s[0] == 0 and s.dtype == np.float32
            sim_keys.append(t)
            sim_dist.append(s)
        vt, vs = WARP._get_most_similar_L2(stub, P[0], TOPK, None)  # a query vector: no self entry
        pred = WARP._get_scores(stub, rows, cols)
        assert pred.dtype == np.float32 and pred.shape == rows.shape
        out.update({"topn_dist_%d" % d: -neg, "topn_keys_%d" % d: lists, "sim_keys_%d" % d: np.array(sim_keys, np.int32),
                    "sim_dist_%d" % d: np.array(sim_dist, np.float32), "vec_keys_%d" % d: np.asarray(vt, np.int32),
                    "vec_dist_%d" % d: np.asarray(vs, np.float32), "pred_%d" % d: pred})
    return out


if __name__ == "__main__":
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else OUT
    vec = reference_outputs()
    np.savez_compressed(path, **vec)
    print("wrote", path, os.path.getsize(path), "bytes,", len(vec), "arrays")
