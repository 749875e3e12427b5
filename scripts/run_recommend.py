"""Serving at the ML-20M shape: `recommend_unseen` (the k best unseen items of every user) against the path it replaces.
    python scripts/run_recommend.py [mode=device|old] [repeats=5] [warmup=1] [users=4096] [topk=10] [fused=-1] [out=FILE]
138,493 x 27,278, 20 M entries (bench.py's synthetic matrix, the training matrix of scripts/run_eval.py), seeded factors at d = 128.
  device    TopK.set_seen once, then per repeat recommend_unseen for ALL users from host arrays (host-to-host wall time, factor upload
            included) and recommend_unseen_device from factors resident in HBM; merges / exchanges from bfh_topk_get_stats.
  old       dot_topn of topk + |seen| candidates plus the host filter (tests/eval_cases.old_path_candidates / filtered) for `users`
            random users, once after one warm-up call; the full user set is an extrapolation by users."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import eval_cases as ec  # noqa: E402
from buffalo_amd import synth  # noqa: E402
from buffalo_amd.parallel import TopK  # noqa: E402

modes = dict(kv.split("=") for kv in sys.argv[1:])
mode = modes.pop("mode", "device")
repeats = int(modes.pop("repeats", 5))
warmup = int(modes.pop("warmup", 1))
n_sub = int(modes.pop("users", 4096))
TOPK = int(modes.pop("topk", 10))
FUSED = int(modes.pop("fused", -1))
out_path = modes.pop("out", "")
assert not modes, "unknown arguments: %s" % modes

U, I, nnz = synth.SHAPES["ml20m"]
train, _ = ec.hold_out(synth.generate(U, I, nnz, seed=7), seed=11)
d = 128
rng = np.random.default_rng(20)
P = 0.5 * rng.standard_normal((U, d), dtype=np.float32)
Q = 0.5 * rng.standard_normal((I, d), dtype=np.float32)
NO_BIAS, NO_POOL = np.zeros((1, 0), np.float32), np.zeros(0, np.int32)
users = np.arange(U, dtype=np.int32)
subset = np.sort(np.random.default_rng(3).choice(U, size=min(n_sub, U), replace=False)).astype(np.int32)
result = {"mode": mode, "U": U, "I": I, "nnz": int(train.nnz), "d": d, "topk": TOPK, "fused": FUSED}
eng = TopK()

if mode == "device":
    import torch
    tP, tQ = torch.from_numpy(P).cuda(), torch.from_numpy(Q).cuda()
    eng.set_mode("fused", FUSED)
    t0 = time.perf_counter()
    eng.set_seen(train.indptr, train.keys, I)
    result["set_seen_wall_ms"] = (time.perf_counter() - t0) * 1e3
    keys, scores = np.empty((U, TOPK), np.int32), np.empty((U, TOPK), np.float32)
    runs = {"host": [], "device": []}
    for r in range(warmup + repeats):
        for form in ("host", "device"):
            eng.reset_stats()
            t0 = time.perf_counter()
            if form == "host":
                eng.recommend_unseen(users, P, Q, NO_BIAS, keys, scores, NO_POOL, TOPK)
            else:
                eng.recommend_unseen_device(users, tP.data_ptr(), U, tQ.data_ptr(), I, d, d, None, keys, scores, NO_POOL, TOPK)
            wall = (time.perf_counter() - t0) * 1e3
            st = eng.stats()
            run = {"wall_ms": wall, "scores_ms": st["kernel_ms"], "other_kernels_ms": st["aux_ms"], "merges": st["merges"], "exchanges": st["exchanges"]}
            print("run_recommend", form, r, json.dumps(run), flush=True)
            if r >= warmup:
                runs[form].append(run)
    for form, kept in runs.items():
        result[form] = {k: {"median": float(np.median([x[k] for x in kept])), "min": float(min(x[k] for x in kept)),
                            "max": float(max(x[k] for x in kept))} for k in kept[0]}
    result["repeats"], result["warmup"] = repeats, warmup
    seen = set(ec.seen_of(train, int(subset[0])).tolist())
    assert not seen & set(keys[subset[0]].tolist())
elif mode == "old":
    eng.set_mode("flt_min_rule", 1)

    def dot_topn(rows, k):
        ok, os_ = np.empty((len(rows), k), np.int32), np.empty((len(rows), k), np.float32)
        eng.dot_topn(rows, P, Q, NO_BIAS, ok, os_, NO_POOL, k)
        return ok, os_
    dot_topn(subset[:128], TOPK + 100)                                        # warm-up: library load, first launches, engine buffers
    t0 = time.perf_counter()
    lists = ec.filtered(ec.old_path_candidates(dot_topn, train, subset, TOPK), train, subset, TOPK)
    wall = (time.perf_counter() - t0) * 1e3
    result.update(users=int(len(subset)), wall_ms=wall, ms_per_user=wall / len(subset), extrapolated_full_ms=wall / len(subset) * U,
                  listed=int((lists >= 0).sum()))
else:
    raise SystemExit("mode must be device or old")

print("run_recommend", json.dumps(result), flush=True)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
