"""First timing of the L2 mode ("score_func" = 1; csrc/topk.hip: half_norms, rescore_distances) at the ML-20M shape, d = 128.

    python scripts/l2_probe.py [--runs 3] [--rows-cap N] > profiles/l2_first_contact.txt

138,493 users x 27,278 items, factors inside the unit ball (as WARP projects them), resident in HBM; top-10 of ALL users (`dot_topn_device`)
and `recommend_unseen_device` against the training matrix of scripts/run_recommend.py, each under L2 and under dot ON THE SAME HANDLE (the mode
is switched between the calls), one warm-up round and then `--runs` rounds, the modes alternating.  Times: host clock around the call (it ends
in a stream synchronise) and the HIP-event sums of bfh_topk_get_stats -- kernel_ms = the score kernels, aux_ms = everything else, which
under L2 holds the two new steps:
  hb + rescoring   aux_ms(L2) - aux_ms(dot twin: "flt_min_rule" = 0 and Qb = hb, so pack and selection do the same work)
  hb alone         the same difference for ONE query (rescoring 10 rows is nothing)
The expectation from the code: the dot time plus one pass over Q (14 MB) plus nq * k gathered rows (1.4 M rows of 512 B).  `--rows-cap`
cuts both matrices (rehearsals at a small size)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

D, K = 128, 10
NO_POOL = np.zeros(0, np.int32)


def ball(rng, rows):
    X = rng.standard_normal((rows, D), dtype=np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    return np.ascontiguousarray(X * rng.uniform(0.15, 1.0, size=(rows, 1)).astype(np.float32))


def line(name, runs):
    r = np.array(runs)
    return "  %-34s wall %8.2f [%8.2f .. %8.2f]   score kernels %8.2f   everything else %8.3f [%8.3f .. %8.3f]   handed back %d" % (
        name, np.median(r[:, 0]), r[:, 0].min(), r[:, 0].max(), np.median(r[:, 1]), np.median(r[:, 2]), r[:, 2].min(), r[:, 2].max(), int(r[-1, 3]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--rows-cap", type=int, default=0)
    args = ap.parse_args()
    import torch
    import eval_cases as ec
    import l2_cases as lc
    from buffalo_amd import synth
    from buffalo_amd.parallel import TopK
    U, I, nnz = synth.SHAPES["ml20m"]
    if args.rows_cap:
        nnz = int(nnz * (min(U, args.rows_cap) / U) * (min(I, args.rows_cap) / I))
        U, I = min(U, args.rows_cap), min(I, args.rows_cap)
    train, _ = ec.hold_out(synth.generate(U, I, nnz, seed=7), seed=11)
    rng = np.random.default_rng(20)
    P, Q = ball(rng, U), ball(rng, I)
    tP, tQ = torch.from_numpy(P).cuda(), torch.from_numpy(Q).cuda()
    tHb = torch.from_numpy(lc.half_norms(Q)).cuda()
    torch.cuda.synchronize()
    eng = TopK()
    eng.set_seen(train.indptr, train.keys, I)
    users = np.arange(U, dtype=np.int32)
    keys = {m: np.empty((U, K), np.int32) for m in ("l2", "twin", "dot")}
    scores = {m: np.empty((U, K), np.float32) for m in ("l2", "twin", "dot")}

    def call(what, mode, idx):
        eng.set_score_func("l2" if mode == "l2" else "dot")
        eng.set_mode("flt_min_rule", 0 if mode == "twin" else 1)
        qb = tHb.data_ptr() if mode == "twin" else None
        n = len(idx)
        eng.reset_stats()
        t0 = time.perf_counter()
        if what == "topn":
            eng.dot_topn_device(idx, tP.data_ptr(), U, tQ.data_ptr(), I, D, D, qb, False, keys[mode][:n], scores[mode][:n], NO_POOL, K)
        else:
            eng.recommend_unseen_device(idx, tP.data_ptr(), U, tQ.data_ptr(), I, D, D, qb, keys[mode][:n], scores[mode][:n], NO_POOL, K)
        wall = (time.perf_counter() - t0) * 1e3
        st = eng.stats()
        return wall, st["kernel_ms"], st["aux_ms"], st["merges"]

    print("# L2 mode (csrc/topk.hip: topk_half_sqnorm_kernel, topk_sqdist_kernel) -- first device run, one MI355X.  Box-to-box caveat as everywhere")
    print("# in this directory: times of one box, one process.  %d x %d, d = %d, k = %d, %d training entries; factors in HBM; ms, median [min .. max]"
          % (U, I, D, K, train.nnz))
    print("# of %d runs after one warm-up round; dot, its twin (flt_min_rule = 0, Qb = hb) and L2 alternate on one handle." % args.runs)
    for what, label in (("topn", "top-%d of all users (dot_topn_device)" % K), ("unseen", "recommend_unseen_device")):
        runs = {(m, n): [] for m in ("dot", "twin", "l2") for n in ("all", "one")}
        for r in range(args.runs + 1):
            for m in ("dot", "twin", "l2"):
                for n, idx in (("all", users), ("one", users[:1])):
                    got = call(what, m, idx)
                    if r:
                        runs[(m, n)].append(got)
        assert np.array_equal(keys["l2"], keys["twin"]), "the L2 lists differ from the dot twin's"
        sample = np.random.default_rng(1).choice(U, size=min(U, 256), replace=False)
        for b in sample:
            assert np.array_equal(scores["l2"][b].view(np.uint32), lc.sqdist32(Q[keys["l2"][b]], P[b]).view(np.uint32)), "distance bits"
        print(label)
        for m, name in (("dot", "dot"), ("twin", "dot twin (Qb = hb, all admissible)"), ("l2", "L2")):
            print(line(name, runs[(m, "all")]))
        aux = {k: float(np.median(np.array(v)[:, 2])) for k, v in runs.items()}
        wall = {k: float(np.median(np.array(v)[:, 0])) for k, v in runs.items()}
        both, hb = aux[("l2", "all")] - aux[("twin", "all")], aux[("l2", "one")] - aux[("twin", "one")]
        print("  hb + rescoring %.3f ms; hb alone (one query) %.3f ms -> rescoring %.3f ms = %d rows of %d B at %.2f TB/s; L2 wall / dot wall = %.3f"
              % (both, hb, both - hb, U * K, D * 4, U * K * D * 4 / max(both - hb, 1e-9) / 1e9, wall[("l2", "all")] / wall[("dot", "all")]))
        print("  checked: L2 keys == the twin's; out_scores == numpy ((Q[key] - p) ** 2).sum(-1) bits on 256 random rows")


if __name__ == "__main__":
    main()
