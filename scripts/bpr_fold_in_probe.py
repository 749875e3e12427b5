"""First contact of bfh_bpr_fold_in on the ML-20M shape: every user's history folded in against a fixed Q / Qb, `--iters` (5) passes, one negative,
at d = 20, 128.

Per d, one process, one untimed call and `--runs` (3) recorded ones:
  * fold_in with host arrays in and out: wall time of the call (host to host) and the HIP-event time of its kernel (`fold_kernel_ms`); the bytes the
    kernel gathers (steps x 2 rows x 4 vdim) per second, to be set beside the bare gather rate of profiles/r04_micro_gather_rate.txt (10.7 TB/s for
    512-byte rows of a 14 MB item table);
  * the host path it replaces: the same rule in numpy float32 (one user after the other, the negatives drawn by numpy's own generator -- the cost
    of a step, not the library's draws) on the first `--slice` (4,096) users, and that time scaled to all users by their entries (labelled so).

    python scripts/bpr_fold_in_probe.py [--out FILE] [--runs 3] [--iters 5] [--ds 20,128] [--slice 4096]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LR, MIN_LR, REG_U = 0.05, 0.001, 0.025


def numpy_fold(Q, Qb, indptr, keys, n_users, iters, table):
    """The rule of bfh_bpr_fold_in in float32 numpy for users [0, n_users), negatives from numpy's generator (rejected while in the history)."""
    rng = np.random.default_rng(0)
    I, d = Q.shape
    out = np.zeros((n_users, d), np.float32)
    lrs = [np.float32(LR - (LR - MIN_LR) * t / iters) for t in range(iters)]
    reg = np.float32(REG_U)
    for b in range(n_users):
        row = keys[(indptr[b - 1] if b else 0):indptr[b]]
        seen, p = set(row.tolist()), out[b]
        for t in range(iters):
            negs = rng.integers(0, I, size=row.shape[0])
            for pos, neg in zip(row.tolist(), negs.tolist()):
                while neg in seen:
                    neg = int(rng.integers(0, I))
                dq = Q[pos] - Q[neg]
                x = np.float32(np.dot(p, dq) + (Qb[pos, 0] - Qb[neg, 0]))
                g = np.float32(0) if x > 6 else np.float32(1) if x < -6 else table[int((x + np.float32(6)) * np.float32(83))]
                p += lrs[t] * (g * dq - reg * p)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--ds", default="20,128")
    ap.add_argument("--slice", type=int, default=4096)
    args = ap.parse_args()
    import bench
    from buffalo_amd.backend import CyBPR

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    csr = bench.load_matrix("ml20m", 7)
    U, I, nnz = csr.num_users, csr.num_items, csr.nnz
    lengths = np.diff(np.concatenate([[0], csr.indptr]))
    say("BPRMF fold-in first contact: ML-20M shape (buffalo_amd/synth.py, seed 7): %d users, %d items, %d entries; all users folded in per call, %d passes, "
        "1 negative (uniform, verify_neg), use_bias, lr %g -> %g; longest history %d, histories above the LDS key limit (128 / 256 keys at d = 20 / 128): %d / %d"
        % (U, I, nnz, args.iters, LR, MIN_LR, int(lengths.max()), int((lengths > 128).sum()), int((lengths > 256).sum())))
    say("1 untimed + %d recorded calls each; ms" % args.runs)
    table = np.array([1.0 / (np.float32(np.exp((i / np.float32(1000) * 2 - 1) * 6)) + 1.0) for i in range(1000)], np.float32)
    for d in [int(x) for x in args.ds.split(",")]:
        vdim = (d + 31) // 32 * 32
        rng = np.random.default_rng(9)
        Q = np.zeros((I, vdim), np.float32)
        Q[:, :d] = rng.normal(scale=0.1, size=(I, d))
        Qb = rng.normal(scale=0.1, size=(I, 1)).astype(np.float32)
        P = np.zeros((1, vdim), np.float32)
        g = CyBPR()
        path = bench.write_opt(dict(d=d, num_negative_samples=1, use_bias=True, verify_neg=True, sampling_power=0.0, random_seed=3, reg_u=REG_U, reg_i=REG_U,
                                    reg_j=REG_U, reg_b=REG_U, optimizer="sgd", lr=LR, min_lr=MIN_LR, num_iters=args.iters, update_i=True, update_j=True,
                                    per_coordinate_normalize=False, compute_loss_on_training=False, num_workers=1, beta1=0.9, beta2=0.999, eps=1e-10))
        assert g.init(path)
        os.unlink(path)
        g.initialize_model(P, Q, Qb, nnz, True)
        out = np.zeros((U, d), np.float32)
        g.fold_in(csr.indptr, csr.keys, args.iters, LR, MIN_LR, out=out)
        rec = []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            g.fold_in(csr.indptr, csr.keys, args.iters, LR, MIN_LR, out=out)
            rec.append(((time.perf_counter() - t0) * 1e3, g.fold_kernel_ms))
        wall, ker = np.mean(rec, axis=0)
        steps = float(nnz) * args.iters
        gathered = steps * 2 * 4 * vdim
        say("d=%d fold_in: whole call %s (mean %.1f) | kernel %s (mean %.3f; %.1f M steps -> %.2f G steps/s; %.2f GB gathered -> %.2f TB/s; finite rows: %s)" %
            (d, " ".join("%.1f" % r[0] for r in rec), wall, " ".join("%.3f" % r[1] for r in rec), ker, steps / 1e6, steps / (ker * 1e-3) / 1e9,
             gathered / 1e9, gathered / (ker * 1e-3) / 1e12, bool(np.isfinite(out).all())))
        n = min(args.slice, U)
        t0 = time.perf_counter()
        numpy_fold(Q[:, :d].copy(), Qb, csr.indptr, csr.keys, n, args.iters, table)
        host = (time.perf_counter() - t0) * 1e3
        part = float(csr.indptr[n - 1]) / nnz
        say("d=%d numpy float32, the first %d users (%.2f %% of the entries): %.0f ms; EXTRAPOLATED to all users by entries: %.0f s -> fold_in is %.0fx host to host" %
            (d, n, 100 * part, host, host / part / 1e3, host / part / wall))
        del g
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
