"""First contact of bfh_eals_fold_in on the ML-20M shape: every user's history folded in against a fixed item factor, d = 32 and 128,
iters = 1 and 5, one process.

Per (d, iters), alternated `--runs` (3) times after one untimed visit each:
  fold   CyEALS.fold_in of all histories: bfh_stats kernel_ms (HIP events around the fold kernels) and the whole call, host arrays in to
         host arrays out
  train  the only device path there was before: a second CyEALS whose P are the new users (zero rows), precompute_cache on both axes, then
         iters x update(0): the kernel_ms of the updates, and host to host including the caches
Then kernel_ms per class: the histories of each class (classified here with the constants of csrc/eals_fold_kernels.hpp, as the host does)
folded in a call of their own.  The numpy float32 loop runs on the first `--host-rows` (4,096) users; the figure for all users is that
time scaled by the row count and labelled "extrapolated, not run".  Bytes: what staging gathers per history (n_b rows of 4 vdim bytes,
once) against a gather per sweep.

    python scripts/eals_fold_in_probe.py [--out FILE] [--runs 3] [--host-rows 4096] [--ds 32,128] [--iters 1,5]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EALS_FOLD_LDS, EALS_FOLD_BLOCK_MAX, EALS_HEAVY = 64 * 1024, 512, 4096      # csrc/eals_fold_kernels.hpp, csrc/eals_kernels.hpp
OPT = {"num_workers": 1, "alpha": 2.0, "reg_u": 0.1, "reg_i": 0.2, "num_iters": 1, "c0": 0.5, "exponent": 0.5, "model_path": "", "data_opt": {}}


def class_of(n, vdim):
    """eals_fold_class: the kernel instance a history of n entries runs on."""
    for G in (16, 32, 64):
        if n <= G and (64 // G) * (vdim * (G | 1) + 2 * G + 4 * vdim + 8) * 4 <= EALS_FOLD_LDS:
            return "resident G=%d" % G
    if n <= min(EALS_FOLD_BLOCK_MAX, (EALS_FOLD_LDS // 4 - 5 * vdim - 8) // (vdim + 2)):
        return "resident block"
    return "streamed 256" if n <= EALS_HEAVY else "streamed 1024"


def handle(d, P, Q, Cw):
    import bench
    from buffalo_amd.backend import CyEALS
    g = CyEALS()
    path = bench.write_opt(dict(OPT, d=d))
    assert g.init(path)
    os.unlink(path)
    g.initialize_model(P, Q, Cw)
    return g


def host_rows(indptr, keys, vals, Q, Cw, iters, n_rows):
    """The rule in numpy float32 on the host: seconds for the first n_rows users."""
    alpha, reg = np.float32(OPT["alpha"]), np.float32(OPT["reg_u"])
    t0 = time.perf_counter()
    CQ = np.sqrt(Cw)[:, None] * Q
    S = CQ.T @ CQ
    out = np.zeros((n_rows, Q.shape[1]), np.float32)
    beg = 0
    for b in range(n_rows):
        end = int(indptr[b])
        q, v = Q[keys[beg:end]], vals[beg:end]
        w = 1 + alpha * v
        m, wv, p, vhat = w - Cw[keys[beg:end]], w * v, out[b], np.zeros(end - beg, np.float32)
        for _ in range(iters):
            for d in range(Q.shape[1]):
                qd = q[:, d]
                f = vhat - p[d] * qd
                p[d] = (((wv - m * f) * qd).sum() - p @ S[d] + p[d] * S[d, d]) / ((m * qd * qd).sum() + S[d, d] + reg)
                vhat = f + p[d] * qd
        beg = end
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--host-rows", type=int, default=4096)
    ap.add_argument("--ds", default="32,128")
    ap.add_argument("--iters", default="1,5")
    args = ap.parse_args()
    import bench
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
    lens = np.diff(np.concatenate([[0], csr.indptr]))
    pop = np.bincount(csr.keys, minlength=I).astype(np.float64) ** 0.5
    Cw = (0.5 * pop / pop.sum()).astype(np.float32)
    say("eALS fold-in first contact: ML-20M shape (buffalo_amd/synth.py, seed 7): %d users, %d items, %d entries, values 1 + Poisson(1); all users per call; ms" % (U, I, nnz))
    for d in [int(x) for x in args.ds.split(",")]:
        vdim = (d + 31) // 32 * 32
        Q = np.random.default_rng(9).normal(scale=0.1, size=(I, d)).astype(np.float32)
        names = np.array([class_of(int(n), vdim) for n in lens])
        g = handle(d, np.zeros((2, d), np.float32), Q.copy(), Cw)
        out = np.zeros((U, d), np.float32)
        for iters in [int(x) for x in args.iters.split(",")]:
            def fold():
                g.reset_stats()
                t0 = time.perf_counter()
                g.fold_in(csr.indptr, csr.keys, vals, iters, out=out)
                return g.stats()["kernel_ms"], (time.perf_counter() - t0) * 1e3

            def train():
                t0 = time.perf_counter()
                tr = handle(d, np.zeros((U, d), np.float32), Q.copy(), Cw)
                tr.precompute_cache(nnz, csr.indptr, csr.keys, 0)
                tr.precompute_cache(nnz, t.indptr, t.keys, 1)
                tr.reset_stats()
                for _ in range(iters):
                    assert tr.update(csr.indptr, csr.keys, vals, 0)
                return tr.stats()["kernel_ms"], (time.perf_counter() - t0) * 1e3

            fold(), train()      # untimed
            rec = [(fold(), train()) for _ in range(args.runs)]
            say("d=%d iters=%d fold_in: kernel_ms %s | host to host %s" % (d, iters, " ".join("%.3f" % r[0][0] for r in rec), " ".join("%.1f" % r[0][1] for r in rec)))
            say("d=%d iters=%d second CyEALS, 2 x precompute_cache, %d x update(0): kernel_ms %s | host to host %s" %
                (d, iters, iters, " ".join("%.3f" % r[1][0] for r in rec), " ".join("%.1f" % r[1][1] for r in rec)))
            for name in sorted(set(names)):
                rows = np.flatnonzero(names == name)
                k = np.concatenate([csr.keys[(csr.indptr[r] - lens[r]):csr.indptr[r]] for r in rows])
                v = np.concatenate([vals[(csr.indptr[r] - lens[r]):csr.indptr[r]] for r in rows])
                ip = np.cumsum(lens[rows], dtype=np.int64)
                g.fold_in(ip, k, v, iters)
                ms = []
                for _ in range(args.runs):
                    g.reset_stats()
                    g.fold_in(ip, k, v, iters)
                    ms.append(g.stats()["kernel_ms"])
                say("d=%d iters=%d class %-15s %6d histories %9d entries: kernel_ms %s" % (d, iters, name, rows.size, k.shape[0], " ".join("%.3f" % x for x in ms)))
        n = min(args.host_rows, U)
        sec, ref = host_rows(csr.indptr, csr.keys, vals, Q, Cw, 1, n)
        g.fold_in(csr.indptr, csr.keys, vals, 1, out=out)
        say("d=%d numpy float32 loop, iters=1: %d users in %.2f s = %.3f ms per user; all %d users %.1f s extrapolated, not run; device rows against these: "
            "max abs difference / largest entry %.2g" % (d, n, sec, sec / n * 1e3, U, sec / n * U, float(np.abs(out[:n] - ref).max() / np.abs(ref).max())))
        say("d=%d bytes: staging gathers 4 x vdim = %d bytes per entry once = %.1f MB per call (mean %.0f per history); a gather per sweep moves that "
            "times iters (x5 at iters = 5); the trainer's update(0) re-gathers it every sweep in 64-byte segments" % (d, 4 * vdim, 4e-6 * vdim * nnz, 4.0 * vdim * nnz / U))
        del g


if __name__ == "__main__":
    main()
