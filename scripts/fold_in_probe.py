"""First contact of bfh_als_fold_in on the ML-20M shape: every user's history folded in against a fixed item factor, at d = 32, 96, 128.

The solve of the folded-in rows has two kernels behind one knob ("als_fold_solve": 1 = als_fold_solve_kernel, the Cholesky all four waves of a
block take part in; 0 = als_solve_kernel with the llt solver, one wave factors), both on the same slots.  They are timed alternately inside ONE
handle, as the walk A/B is (scripts/bpr_walk_ab.py): visits 0 0 1 0 1 0 1, each visit one untimed call and `--runs` (3) recorded ones.  The first
two visits are both knob 0: the difference of their means is the run-to-run spread every comparison is held against.  Per run: the solve
kernel's HIP-event time (bfh_stats optimizer_ms), all kernels of the call (kernel_ms: row pass + solve) and the wall time of the whole call,
host arrays in to host arrays out.

The rule (printed with its verdict): keep the new kernel if it beats knob 0 at d = 128 by more than the spread and is not slower than knob 0
beyond the spread at d = 32.

Also timed: what a user has without this call, for the first `--host-rows` (4,096) users -- the system built in numpy, float32 `cholesky` and two
`solve`s per row on the host; the figure for all users is that time scaled by the row count and labelled "extrapolated, not run".

    python scripts/fold_in_probe.py [--out FILE] [--runs 3] [--host-rows 4096] [--ds 32,96,128]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VISITS = (0, 0, 1, 0, 1, 0, 1)


def host_rows(csr, vals, Q, opt, n_rows):
    """numpy on the host: seconds for the first n_rows users."""
    alpha, reg = np.float32(opt["alpha"]), np.float32(opt["reg_u"])
    d = Q.shape[1]
    t0 = time.perf_counter()
    FF = Q.T @ Q
    out = np.zeros((n_rows, d), dtype=np.float32)
    beg = 0
    for u in range(n_rows):
        end = int(csr.indptr[u])
        if end > beg:
            Yk, w = Q[csr.keys[beg:end]], alpha * vals[beg:end]
            A = FF + (Yk * w[:, None]).T @ Yk
            A[np.arange(d), np.arange(d)] += reg
            y = ((1 + w)[:, None] * Yk).sum(axis=0)
            L = np.linalg.cholesky(A)
            out[u] = np.linalg.solve(L.T, np.linalg.solve(L, y))
        beg = end
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--host-rows", type=int, default=4096)
    ap.add_argument("--ds", default="32,96,128")
    args = ap.parse_args()
    import bench
    from buffalo_amd.backend import CyALS

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    csr = bench.load_matrix("ml20m", 7)
    U, I, nnz = csr.num_users, csr.num_items, csr.nnz
    vals = (1 + np.random.default_rng(7).poisson(1.0, size=nnz)).astype(np.float32)
    say("fold-in first contact: ML-20M shape (buffalo_amd/synth.py, seed 7): %d users, %d items, %d entries, values 1 + Poisson(1); all users folded in per call" % (U, I, nnz))
    say("visits (knob als_fold_solve) %s, 1 untimed + %d recorded calls each; ms" % (" ".join(map(str, VISITS)), args.runs))
    verdict = {}
    for d in [int(x) for x in args.ds.split(",")]:
        vdim = ((d + 31) // 32) * 32
        rng = np.random.default_rng(9)
        Q = np.zeros((I, vdim), dtype=np.float32)
        Q[:, :d] = rng.normal(scale=0.1, size=(I, d))
        P = np.zeros((U, vdim), dtype=np.float32)
        opt = dict(bench.ALS_OPT, d=d)
        g = CyALS()
        path = bench.write_opt(opt)
        assert g.init(path)
        os.unlink(path)
        g.initialize_model(P, Q)
        out = np.zeros((U, vdim), dtype=np.float32)
        means = []
        for v, knob in enumerate(VISITS):
            g.set_mode("als_fold_solve", knob)
            g.fold_in(0, csr.indptr, csr.keys, vals, out)
            rec = []
            for _ in range(args.runs):
                g.reset_stats()
                t0 = time.perf_counter()
                g.fold_in(0, csr.indptr, csr.keys, vals, out)
                wall = (time.perf_counter() - t0) * 1e3
                st = g.stats()
                rec.append((st["optimizer_ms"], st["kernel_ms"], wall))
            m = np.mean(rec, axis=0)
            means.append((knob, m))
            say("d=%d visit %d knob %d: solve kernel %s (mean %.3f) | all kernels mean %.3f | whole call mean %.1f" %
                (d, v, knob, " ".join("%.3f" % r[0] for r in rec), m[0], m[1], m[2]))
        spread = abs(means[0][1][0] - means[1][1][0])
        k0 = np.mean([m[0] for k, m in means if k == 0])
        k1 = np.mean([m[0] for k, m in means if k == 1])
        k0_all = [m[0] for k, m in means if k == 0]
        say("d=%d summary: solve kernel knob 0 %.3f ms, knob 1 %.3f ms (%.2fx); spread of the two leading knob-0 visits %.3f ms (all knob-0 visits max - min %.3f); "
            "whole call knob 0 %.1f ms, knob 1 %.1f ms; all kernels knob 0 %.3f, knob 1 %.3f" %
            (d, k0, k1, k0 / max(k1, 1e-9), spread, max(k0_all) - min(k0_all), np.mean([m[2] for k, m in means if k == 0]),
             np.mean([m[2] for k, m in means if k == 1]), np.mean([m[1] for k, m in means if k == 0]), np.mean([m[1] for k, m in means if k == 1])))
        verdict[d] = (k0, k1, spread)
        n = min(args.host_rows, U)
        sec, ref = host_rows(csr, vals, Q[:, :d].copy(), opt, n)
        err = float(np.abs(out[:n, :d] - ref).max() / np.abs(ref).max())
        say("d=%d host path (numpy float32 cholesky + two solves per row): %d users in %.2f s = %.3f ms per user; all %d users "
            "%.1f s extrapolated, not run; device rows against these: max abs difference / largest entry %.2g" % (d, n, sec, sec / n * 1e3, U, sec / n * U, err))
        del g
    if 128 in verdict and 32 in verdict:
        a0, a1, asp = verdict[128]
        b0, b1, bsp = verdict[32]
        keep = (a0 - a1 > asp) and (b1 - b0 <= bsp)
        say("rule: keep als_fold_solve_kernel if it beats knob 0 at d = 128 by more than the spread (%.3f - %.3f = %.3f ms against %.3f) and is not slower than "
            "knob 0 beyond the spread at d = 32 (%.3f - %.3f = %.3f ms against %.3f): %s" %
            (a0, a1, a0 - a1, asp, b1, b0, b1 - b0, bsp, "KEEP" if keep else "REMOVE"))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
