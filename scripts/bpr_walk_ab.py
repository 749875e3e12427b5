"""In-process A/B of the BPRMF item-major walk on the headline workload (ML-20M shape, seed 7, d = 128, option defaults).

Two handles of one build differ by +-5 % in two modes while the walk inside ONE handle repeats to 0.01 ms, so variants are
compared inside one handle: the knob settings are alternated `--rounds` times, each visit runs `--warmup` epochs (the first epoch after a
switch redraws its negatives on the main stream) and then `--epochs` timed ones.  Per visit: walk kernel ms per launch, aux ms per epoch
(presample on the main stream, drain, merges) and wall ms per epoch.  The learning rate is held at the option default (lr = min_lr = 0.002):
the flush intervals follow the learning rate, and a decaying schedule would put a trend under the alternation.

    python scripts/bpr_walk_ab.py --variants "p1:im_presample=1;p2:im_presample=2" [--rounds 3] [--epochs 20] [--warmup 5] [--out FILE] [--lib SO]

`--lib`: load this shared library instead of the package's (an experimental build next to the product build).
Prints one line per visit and a summary per variant: mean, and the spread (max - min) of the visits' means -- the handle's own repeat spread.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", required=True, help='"name:knob=v,knob=v;name:..." (knobs of bfh_bpr_set_mode)')
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    variants = []
    for part in args.variants.split(";"):
        name, _, knobs = part.partition(":")
        variants.append((name, [(kv.split("=")[0], int(kv.split("=")[1])) for kv in knobs.split(",") if kv]))
    if args.lib:
        from buffalo_amd import _lib
        _lib.LIB_PATH = os.path.abspath(args.lib)
    import bench
    from buffalo_amd import synth
    from buffalo_amd.backend import CyBPR

    csr = bench.load_matrix("ml20m", 7)
    U, I, nnz = csr.num_users, csr.num_items, csr.nnz
    opt = bench.bpr_options(num_iters=1, seed=7, min_lr=0.002)
    P, Q, Qb = synth.init_factors(U, I, bench.D, seed=7)
    obj = CyBPR()
    path = bench.write_opt(opt)
    assert obj.init(path)
    os.unlink(path)
    obj.sync_every_epoch = False
    obj.initialize_model(P, Q, Qb, nnz, True)
    obj.set_cumulative_table(np.zeros(I, np.int64), I)
    obj.set_resident_csr(csr.indptr, csr.keys)

    def epochs(n):
        obj.reset_stats()
        t0 = time.perf_counter()
        for _ in range(n):
            obj.add_jobs(0, U, csr.indptr, None)
            obj.update_parameters()
        obj.wait_until_done()
        dt = time.perf_counter() - t0
        st = obj.stats()
        return {"kernel_ms_per_launch": st["kernel_ms"] / max(st["launches"], 1), "launches_per_epoch": st["launches"] / n,
                "aux_ms_per_epoch": st["aux_ms"] / n, "wall_ms_per_epoch": dt / n * 1e3}

    visits = []
    for r in range(args.rounds):
        for name, knobs in variants:
            for k, v in knobs:
                obj.set_mode(k, v)
            epochs(args.warmup)
            row = dict(epochs(args.epochs), variant=name, round=r)
            visits.append(row)
            print("round %d %-10s walk %.4f ms/launch (%.1f launches/epoch)  aux %.4f ms/epoch  wall %.4f ms/epoch"
                  % (r, name, row["kernel_ms_per_launch"], row["launches_per_epoch"], row["aux_ms_per_epoch"], row["wall_ms_per_epoch"]), flush=True)
    summary = {}
    for name, _ in variants:
        rows = [v for v in visits if v["variant"] == name]
        summary[name] = {}
        for key in ("kernel_ms_per_launch", "aux_ms_per_epoch", "wall_ms_per_epoch"):
            x = [v[key] for v in rows]
            summary[name][key] = {"mean": float(np.mean(x)), "spread": float(max(x) - min(x))}
        s = summary[name]
        print("%-10s walk %.4f ms/launch (spread %.4f)  aux %.4f (spread %.4f)  wall %.4f (spread %.4f)"
              % (name, s["kernel_ms_per_launch"]["mean"], s["kernel_ms_per_launch"]["spread"], s["aux_ms_per_epoch"]["mean"], s["aux_ms_per_epoch"]["spread"],
                 s["wall_ms_per_epoch"]["mean"], s["wall_ms_per_epoch"]["spread"]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"variants": args.variants, "rounds": args.rounds, "epochs": args.epochs, "warmup": args.warmup, "visits": visits, "summary": summary}, f, indent=1)


if __name__ == "__main__":
    main()
