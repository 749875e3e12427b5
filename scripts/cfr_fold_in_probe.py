"""First contact of bfh_cfr_fold_in on the ML-20M shape: every item folded in from its users and its SPPMI row (iters = 1), and every user
from its items, d = 32 and 128, one process.  The context matrix is built with bfh_sppmi_* from the users' histories taken as sequences.

Per d, alternated `--runs` (3) times after one untimed visit each:
  fold   CyCFR.fold_in("item", iters=1, init_bias=the model's) / fold_in("user"): bfh_stats kernel_ms (HIP events around the one launch) and
         the whole call, host arrays in to host arrays out
  train  the path there was before, through a second handle: precompute + partial_update_item / partial_update_user of the same rows --
         kernel_ms (both Gramian passes into HBM slots, the solve, the bias kernel) and the whole call, which writes the model's arrays

    python scripts/cfr_fold_in_probe.py [--out FILE] [--runs 3] [--ds 32,128] [--window 5] [--k 1]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OPT = {"num_workers": 1, "num_cg_max_iters": 3, "alpha": 8.0, "l": 0.1, "eps": 1e-10, "reg_u": 0.1, "reg_i": 0.1, "reg_c": 0.1, "compute_loss": False,
       "optimizer": "llt", "cg_tolerance": 1e-10, "num_iters": 1, "model_path": "", "data_opt": {}}
ARRAYS = ("user", "item", "context", "item_bias", "context_bias")


def handle(d, arrs):
    import bench
    from buffalo_amd.backend import CyCFR
    g = CyCFR()
    path = bench.write_opt(dict(OPT, d=d))
    assert g.init(path)
    os.unlink(path)
    for name in ARRAYS:
        g.set_embedding(arrs[name], name)
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--ds", default="32,128")
    ap.add_argument("--window", type=int, default=5)
    ap.add_argument("--k", type=int, default=1)
    args = ap.parse_args()
    import bench
    from buffalo_amd.ingest import build_sppmi
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    csr = bench.load_matrix("ml20m", 7)
    t = csr.transpose()
    U, I, nnz = csr.num_users, csr.num_items, csr.nnz
    vals = (1 + np.random.default_rng(7).poisson(1.0, size=nnz)).astype(np.float32)
    tvals = vals[np.lexsort((csr.rows(), csr.keys))]
    sp = build_sppmi(csr.indptr, csr.keys, I, args.window, args.k)
    cip, ck, cv = sp["indptr"], sp["key"], sp["val"]
    say("CFR fold-in first contact: ML-20M shape (buffalo_amd/synth.py, seed 7): %d users, %d items, %d rating entries, values 1 + Poisson(1); "
        "SPPMI (window %d, k %d) %d entries; all rows per call; ms" % (U, I, nnz, args.window, args.k, ck.shape[0]))
    for d in [int(x) for x in args.ds.split(",")]:
        rng = np.random.default_rng(9)
        arrs = {n: rng.normal(scale=0.1, size=(r, c)).astype(np.float32) for n, r, c in
                (("user", U, d), ("item", I, d), ("context", I, d), ("item_bias", I, 1), ("context_bias", I, 1))}
        g = handle(d, arrs)
        tr_arrs = {n: a.copy() for n, a in arrs.items()}
        tr = handle(d, tr_arrs)
        init = arrs["item_bias"][:, 0].copy()
        out_i, out_b, out_u = np.zeros((I, d), np.float32), np.zeros(I, np.float32), np.zeros((U, d), np.float32)

        def timed(obj, fn):
            obj.reset_stats()
            t0 = time.perf_counter()
            fn()
            return obj.stats()["kernel_ms"], (time.perf_counter() - t0) * 1e3

        def train_item():
            tr.precompute(b"user")
            tr.partial_update_item(0, I, t.indptr, t.keys, tvals, cip, ck, cv)

        def train_user():
            tr.precompute(b"item")
            tr.partial_update_user(0, U, csr.indptr, csr.keys, vals)
        runs = {"fold_in(item, iters=1)": lambda: timed(g, lambda: g.fold_in("item", t.indptr, t.keys, tvals, cip, ck, cv, iters=1, init_bias=init, out=out_i, out_bias=out_b)),
                "precompute + partial_update_item": lambda: timed(tr, train_item),
                "fold_in(user)": lambda: timed(g, lambda: g.fold_in("user", csr.indptr, csr.keys, vals, out=out_u)),
                "precompute + partial_update_user": lambda: timed(tr, train_user)}
        for fn in runs.values():
            fn()      # untimed
        rec = {name: [] for name in runs}
        for _ in range(args.runs):
            for name, fn in runs.items():
                rec[name].append(fn())
        for name, r in rec.items():
            say("d=%d %-34s kernel_ms %s | host to host %s" % (d, name, " ".join("%.3f" % x[0] for x in r), " ".join("%.1f" % x[1] for x in r)))
        del g, tr


if __name__ == "__main__":
    main()
