"""Validation at the ML-20M shape: the timing behind the validation row of the README and the target of a rocprofv3 pass.
    python scripts/run_eval.py [mode=device|old|precheck] [repeats=10] [warmup=2] [users=4096] [topk=10] [fused=0] [out=FILE]
138,493 x 27,278, 20 M entries (bench.py's synthetic matrix), one held-out entry per user with >= 2 entries (tests/eval_cases.hold_out,
seed 11), seeded factors at d = 128 -- the input of tests/test_eval_scale_gpu.py.
  device    bfh_eval_*: full validation (ranking + score metrics) from factors resident in HBM; per repeat the host-to-host wall time
            and the split from bfh_eval_get_stats (ranking / ranking metrics / score metrics, HIP events); then the same over a random
            subset of `users` rows.  `fused`: the ranking engine's rule (bfh_eval_set_mode: 0 dense, -1 by size, 1 forced); the
            split then also holds the rows handed back to the dense path (merges) and the rows with ties at the last place (exchanges).
  old       the path before the evaluator: the front harness `Evaluable` (tests/front_harness) over dot_topn, host loop and all, on the
            vali entries of the SAME random subset of `users` users (the full set takes minutes); wall time, once after one warm-up
            batch.
  precheck  no GPU: numpy fp32 scores of `users` random users; counts the rows in which the old path's list could depend on the
            number of candidates asked for -- a bit-equal pair of scores among the first topk + 1 unseen items or across the cut at
            `need` = topk + max |seen| of the row's batch of 4096 users sorted by history length."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "front_harness"))
import eval_cases as ec  # noqa: E402
from buffalo_amd import synth  # noqa: E402

modes = dict(kv.split("=") for kv in sys.argv[1:])
mode = modes.pop("mode", "device")
repeats = int(modes.pop("repeats", 10))
warmup = int(modes.pop("warmup", 2))
n_sub = int(modes.pop("users", 4096))
TOPK = int(modes.pop("topk", 10))
FUSED = modes.pop("fused", None)
out_path = modes.pop("out", "")
assert not modes, "unknown arguments: %s" % modes

U, I, nnz = synth.SHAPES["ml20m"]
train, vali = ec.hold_out(synth.generate(U, I, nnz, seed=7), seed=11)
d = 128
rng = np.random.default_rng(20)
P = 0.5 * rng.standard_normal((U, d), dtype=np.float32)
Q = 0.5 * rng.standard_normal((I, d), dtype=np.float32)
rows_all = np.unique(vali["row"])
subset = np.sort(np.random.default_rng(3).choice(rows_all, size=min(n_sub, len(rows_all)), replace=False)).astype(np.int32)
beg = np.concatenate([[0], train.indptr[:-1]])
deg = train.indptr - beg
result = {"mode": mode, "U": U, "I": I, "nnz": int(train.nnz), "n_vali": int(len(vali["row"])), "vali_users": int(len(rows_all)), "d": d,
          "topk": TOPK, "subset_users": int(len(subset)), "max_seen": int(deg.max()), "median_seen": float(np.median(deg[rows_all]))}

if mode == "precheck":
    order = rows_all[np.argsort(deg[rows_all], kind="stable")]
    need_of = np.empty(U, np.int64)
    for a in range(0, len(order), 4096):
        need_of[order[a:a + 4096]] = min(TOPK + deg[order[a:a + 4096]].max(), I)
    at_risk = 0
    for a in range(0, len(subset), 256):
        us = subset[a:a + 256]
        S = P[us] @ Q.T                                                  # fp32
        for i, u in enumerate(us):
            s = S[i]
            srt = np.sort(s)[::-1]
            need = int(need_of[u])
            cut_tie = need < I and srt[need - 1] == srt[need]
            unseen = np.ones(I, bool)
            unseen[ec.seen_of(train, int(u))] = False
            top = np.sort(s[unseen])[::-1][:TOPK + 1]
            at_risk += bool(cut_tie or (top[1:] == top[:-1]).any())
    result.update(rows_checked=int(len(subset)), rows_with_a_tie=int(at_risk), fraction=at_risk / len(subset), cap=0.01)
elif mode == "device":
    import torch
    from buffalo_amd.evaluate import Evaluator
    tP, tQ = torch.from_numpy(P).cuda(), torch.from_numpy(Q).cuda()
    ev = Evaluator()
    t0 = time.perf_counter()
    ev.set_data(U, I, train.indptr, train.keys, vali["row"], vali["col"], vali["val"])
    result["set_data_wall_ms"] = (time.perf_counter() - t0) * 1e3
    result["set_data_device_ms"] = ev.stats()["aux_ms"]
    result["device"] = torch.cuda.get_device_name(0)
    if FUSED is not None:
        ev.set_mode("fused", int(FUSED))
        result["fused"] = int(FUSED)

    def timed(rows):
        runs = []
        for r in range(warmup + repeats):
            ev.reset_stats()
            t0 = time.perf_counter()
            res = ev.ranking_device(tP.data_ptr(), U, tQ.data_ptr(), I, d, d, rows=rows, topk=TOPK)
            res.update(ev.scores_device(tP.data_ptr(), U, tQ.data_ptr(), I, d, d))
            wall = (time.perf_counter() - t0) * 1e3
            st = ev.stats()
            runs.append({"wall_ms": wall, "ranking_ms": st["kernel_ms"], "rank_metrics_ms": st["optimizer_ms"], "score_metrics_ms": st["aux_ms"],
                         "merges": st["merges"], "exchanges": st["exchanges"]})
            print("run_eval device", "all" if rows is None else len(rows), r, json.dumps(runs[-1]), flush=True)
        kept = runs[warmup:]
        return {k: {"median": float(np.median([x[k] for x in kept])), "min": float(min(x[k] for x in kept)),
                    "max": float(max(x[k] for x in kept))} for k in kept[0]}, res

    result["full"], result["full_metrics"] = timed(None)
    result["subset"], result["subset_metrics"] = timed(subset)
    result["repeats"], result["warmup"] = repeats, warmup
elif mode == "old":
    import torch
    from buffalo_front.algo.base import Algo, Evaluable
    from buffalo_front.data import Data, MatrixMarketOptions
    from buffalo_front.misc import Option

    class Model(Algo, Evaluable):
        pass

    keep = np.isin(vali["row"], subset)
    sub_vali = {k: np.ascontiguousarray(v[keep]) for k, v in vali.items()}
    data = Data(MatrixMarketOptions().get_default_option())
    data.groups = {"rowwise": {"indptr": train.indptr, "key": train.keys, "val": train.vals}, "vali": sub_vali}
    data.header = {"num_nnz": train.nnz, "num_users": U, "num_items": I, "completed": 1}
    m = Model()
    m.data, m.P, m.Q, m.Qb = data, P, Q, None
    m.opt = Option({"d": d, "use_bias": False, "validation": {"topk": TOPK, "batch": 128}})
    m._get_topk_recommendation(subset[:128], topk=TOPK + 100)               # warm-up: library load, first launches, engine buffers
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = m.get_validation_results()
    wall = (time.perf_counter() - t0) * 1e3
    result.update(device=torch.cuda.get_device_name(0), wall_ms=wall, ms_per_user=wall / len(subset),
                  extrapolated_full_ms=wall / len(subset) * len(rows_all), metrics={k: float(v) for k, v in res.items()})
else:
    raise SystemExit("mode must be device, old or precheck")

print("run_eval", json.dumps(result), flush=True)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
