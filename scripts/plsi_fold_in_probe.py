"""First contact of bfh_plsi_fold_in on the ML-20M shape: every user's history folded in against a fixed Q, `--iters` (10) EM steps, at d = 20, 128.

Per d, one process, one untimed call and `--runs` (3) recorded ones of each path:
  * fold_in with host arrays in and out: wall time of the call and the HIP-event time of its kernel (`kernel_ms`), with and without the loss;
    algorithmic bytes of one step (entries x (8 + 4 vdim): key, value and the gathered row of Q) over kernel_ms / iters, to be set beside the P
    half-step's figure in profiles/plsi_first_contact.txt (which also reads and writes the owner's rows: + 2 x 4 vdim per row);
  * what a caller has without the call: the trainer with the rows bound as P, reset -> partial_update -> normalize -> swap per step, the frozen Q
    written back and uploaded again after every swap (tests/test_plsi_fold_in_gpu.py::test_equals_the_trainer_bitwise is that loop);
  * the two results compared as bits.

    python scripts/plsi_fold_in_probe.py [--out FILE] [--runs 3] [--iters 10] [--ds 20,128]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make(d, P, Q):
    import bench
    from buffalo_amd.backend import CyPLSI
    g = CyPLSI()
    path = bench.write_opt({"d": d, "random_seed": 0, "num_workers": 1})
    assert g.init(path)
    os.unlink(path)
    g.set_mode("keep_init", 1)
    g.initialize_model(P, Q)
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--ds", default="20,128")
    args = ap.parse_args()
    import bench

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    csr = bench.load_matrix("ml20m", 7)
    U, I, nnz = csr.num_users, csr.num_items, csr.nnz
    vals = np.ones(nnz, dtype=np.float32)
    beg = np.concatenate([[0], csr.indptr[:-1]])
    lengths = csr.indptr - beg
    say("pLSI fold-in first contact: ML-20M shape (buffalo_amd/synth.py, seed 7): %d users, %d items, %d entries, values 1.0; all users folded in per call, "
        "%d steps, alpha1 = 1; rows above one segment of 2048 entries: %d (longest %d)" % (U, I, nnz, args.iters, int((lengths > 2048).sum()), int(lengths.max())))
    say("1 untimed + %d recorded calls each; ms" % args.runs)
    for d in [int(x) for x in args.ds.split(",")]:
        vdim = (d + 31) // 32 * 32
        rng = np.random.default_rng(9)
        Q0 = np.abs(rng.normal(scale=1.0 / d, size=(I, d)))
        Q0 = np.ascontiguousarray(Q0 / Q0.sum(axis=0, keepdims=True), dtype=np.float32)
        start = np.full((U, d), np.float32(1.0) / np.float32(d), dtype=np.float32)
        g = make(d, start.copy(), Q0.copy())
        out, loss = np.zeros((U, d), dtype=np.float32), np.zeros(U)
        step_bytes = nnz * (8.0 + 4.0 * vdim)
        for name, L in (("without the loss", None), ("with the loss", loss)):
            g.fold_in(csr.indptr, csr.keys, vals, args.iters, 1.0, out=out, loss=L)
            rec = []
            for _ in range(args.runs):
                t0 = time.perf_counter()
                g.fold_in(csr.indptr, csr.keys, vals, args.iters, 1.0, out=out, loss=L)
                rec.append(((time.perf_counter() - t0) * 1e3, g.fold_kernel_ms))
            wall, ker = np.mean(rec, axis=0)
            say("d=%d fold_in %s: whole call %s (mean %.1f) | kernel %s (mean %.3f = %.3f per step; %.2f GB per step -> %.2f TB/s)" %
                (d, name, " ".join("%.1f" % r[0] for r in rec), wall, " ".join("%.3f" % r[1] for r in rec), ker, ker / args.iters, step_bytes / 1e9,
                 step_bytes / (ker / args.iters * 1e-3) / 1e12))
        fold_wall = wall
        del g
        P, Q = start.copy(), Q0.copy()
        t = make(d, P, Q)

        def loop():
            P[:] = start
            t.synchronize(False)
            t0 = time.perf_counter()
            for _ in range(args.iters):
                t.reset()
                t.partial_update(0, U, csr.indptr, csr.keys, vals)
                t.normalize(1.0, 1.0)
                t.swap()
                Q[:] = Q0
                t.synchronize(False)
            return (time.perf_counter() - t0) * 1e3

        loop()
        rec = []
        for _ in range(args.runs):
            t.reset_stats()
            wall = loop()
            st = t.get_stats()
            rec.append((wall, st["kernel_ms"], st["optimizer_ms"], st["aux_ms"], st["exchange_kernel_ms"], st["allreduce_ms"]))
        m = np.mean(rec, axis=0)
        say("d=%d frozen-Q trainer loop: whole loop %s (mean %.1f) | per loop: P half-steps %.3f, Q half-steps %.3f, transposes %.3f, normalise %.3f, copy-back %.3f" %
            (d, " ".join("%.1f" % r[0] for r in rec), m[0], m[1], m[2], m[3], m[4], m[5]))
        same = np.array_equal(P.view(np.uint32), out.view(np.uint32))
        say("d=%d summary: fold_in %.1f ms against the trainer loop %.1f ms host to host (%.1fx); rows identical as bits: %s" % (d, fold_wall, m[0], m[0] / fold_wall, same))
        del t
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
