"""First contact of bfh_warp_fold_in on the ML-20M shape: every user's history folded in against a fixed Q, `--iters` (5) passes, at d = 128, 256.

Per d, one process, one untimed call and `--runs` (3) recorded ones:
  * fold_in with host arrays in and out: wall time of the call (host to host) and the HIP-event time of its kernel (`fold_kernel_ms`); the scored
    candidates per positive (from `counts`); the bytes the kernel gathers for the rows it needs -- (positives + scored candidates) x 4 vdim; the rows
    the 1 / 2 / 4 speculation fetches beyond the deciding candidate are not counted by the kernel, so this is a lower bound -- per second, to be set
    beside the bare gather rate of profiles/r04_micro_gather_rate.txt (10.7 TB/s for 512-byte rows of a 14 MB item table);
  * the host path it replaces: the same rule in numpy float32 (one user after the other, a pass vectorised over the user's positives, candidates
    from numpy's own generator -- the cost of a pass, not the library's draws) on the first `--slice` (4,096) users, scaled to all users by their
    entries (labelled so).

    python scripts/warp_fold_in_probe.py [--out FILE] [--runs 3] [--iters 5] [--ds 128,256] [--slice 4096]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LR, MAX_TRIALS = 0.05, 500
threshold_of = lambda d: -0.4 * np.sqrt(2.0 / d)   # 0.4 sigma below the mean of ui - uj for unit rows: about a third of the candidates violate it


def numpy_fold(Q, init, threshold, indptr, keys, n_users, iters, kmax=8):
    """The rule of bfh_warp_fold_in (dot, adagrad, reg_u = 0) in float32 numpy for users [0, n_users): up to `kmax` unseen candidates per positive."""
    rng = np.random.default_rng(0)
    I, d = Q.shape
    out = init[:n_users].copy()
    for b in range(n_users):
        row = keys[(indptr[b - 1] if b else 0):indptr[b]]
        n = row.shape[0]
        if n == 0:
            continue
        seen, p, vel = np.isin(np.arange(I), row), out[b], np.zeros(d, np.float32)
        for t in range(iters):
            cand = rng.integers(0, I, size=(n, 2 * kmax))
            order = np.argsort(seen[cand], axis=1, kind="stable")[:, :kmax]        # the unseen draws first, in draw order
            cand = np.take_along_axis(cand, order, axis=1)
            ui, uj = Q[row] @ p, Q[cand] @ p
            viol = ((ui[:, None] - uj) < threshold) & ~seen[cand]
            found, first = viol.any(axis=1), viol.argmax(axis=1)
            phi = np.log(np.maximum(1, (I - n - 1) // (2 * (first[found] + 1)))).astype(np.float32)
            g = (phi[:, None] * (Q[row[found]] - Q[cand[found, first[found]]])).sum(axis=0)
            vel += g * g
            p += np.float32(LR) * g / (np.sqrt(vel) + np.float32(1e-10))
            p /= max(np.float32(1), np.sqrt((p * p).sum()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--ds", default="128,256")
    ap.add_argument("--slice", type=int, default=4096)
    args = ap.parse_args()
    import bench
    from buffalo_amd.backend import CyWARP

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    csr = bench.load_matrix("ml20m", 7)
    U, I, nnz = csr.num_users, csr.num_items, csr.nnz
    lengths = np.diff(np.concatenate([[0], csr.indptr]))
    say("WARP fold-in first contact: ML-20M shape (buffalo_amd/synth.py, seed 7): %d users, %d items, %d entries; all users folded in per call, %d passes, "
        "dot score, adagrad, item and start rows of norm about 1, threshold -0.4 sqrt(2 / d), max_trials %d, lr %g; longest history %d (LDS key bound 8192)" % (U, I, nnz, args.iters, MAX_TRIALS, LR, int(lengths.max())))
    say("1 untimed + %d recorded calls each; ms" % args.runs)
    for d in [int(x) for x in args.ds.split(",")]:
        vdim = (d + 31) // 32 * 32
        rng = np.random.default_rng(9)
        Q = np.zeros((I, vdim), np.float32)
        Q[:, :d] = rng.normal(scale=1.0 / np.sqrt(d), size=(I, d))
        g = CyWARP()
        init = rng.normal(scale=1.0 / np.sqrt(d), size=(U, d)).astype(np.float32)
        path = bench.write_opt(dict(d=d, threshold=float(threshold_of(d)), max_trials=MAX_TRIALS, score_func="dot", random_seed=3, reg_u=0.0, reg_i=0.0, reg_j=0.0,
                                    optimizer="adagrad", lr=LR, min_lr=0.0001, num_iters=args.iters, update_i=True, update_j=True,
                                    per_coordinate_normalize=False, compute_loss_on_training=False, num_workers=1, beta1=0.9, beta2=0.999, eps=1e-10))
        assert g.init(path)
        os.unlink(path)
        g.initialize_model(np.zeros((1, vdim), np.float32), Q, np.zeros((I, 1), np.float32), nnz, True)
        out, counts = np.zeros((U, d), np.float32), np.zeros((U, 2), np.int64)
        g.fold_in(csr.indptr, csr.keys, args.iters, LR, init=init, out=out, counts=counts)
        rec = []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            g.fold_in(csr.indptr, csr.keys, args.iters, LR, init=init, out=out, counts=counts)
            rec.append(((time.perf_counter() - t0) * 1e3, g.fold_kernel_ms))
        wall, ker = np.mean(rec, axis=0)
        positives, scored, accepted = float(nnz) * args.iters, float(counts[:, 0].sum()), float(counts[:, 1].sum())
        gathered = (positives + scored) * 4 * vdim
        say("d=%d fold_in: whole call %s (mean %.1f) | kernel %s (mean %.3f) | %.1f M positives, %.2f scored candidates per positive, %.1f %% accepted | "
            ">= %.2f GB gathered -> >= %.2f TB/s | finite rows: %s" %
            (d, " ".join("%.1f" % r[0] for r in rec), wall, " ".join("%.3f" % r[1] for r in rec), ker, positives / 1e6, scored / positives,
             100 * accepted / positives, gathered / 1e9, gathered / (ker * 1e-3) / 1e12, bool(np.isfinite(out).all())))
        n = min(args.slice, U)
        t0 = time.perf_counter()
        numpy_fold(Q[:, :d].copy(), init, threshold_of(d), csr.indptr, csr.keys, n, args.iters)
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
