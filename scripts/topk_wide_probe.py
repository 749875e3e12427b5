"""First timing of the fused sweep for 128 < d <= 256 (csrc/topk_kernels.hpp: topk_scores_wide_kernel) at the ML-20M shape.

    python scripts/topk_wide_probe.py [--runs 3] [--rows-cap N] > profiles/topk_wide_first_contact.txt

138,493 users x 27,278 items, random normal factors resident in HBM, k = 10: top-10 of ALL users (`dot_topn_device`) and
`recommend_unseen_device` against the training matrix of scripts/run_recommend.py, at d = 256 (the straight-line instance) and d = 192
(a guarded chunk 1), with "fused" = 0 (the dense path: two score launches through the [batch, items] buffer) and the wide sweep -- "fused"
= 1 for dot_topn, the default rule "fused" = -1 for recommend_unseen, which a forced call fuses up to d = 128 only -- ALTERNATING on one
handle: one warm-up round, then `--runs` rounds.  d = 128 on the same handle gives the one-chunk fused sweep:
the d = 256 sweep issues twice its MFMAs (the last lines print the ratios).  Times: host clock around the call (host
to host: it uploads the ids, ends in the download of the lists and a stream synchronise) and the HIP-event sums of bfh_topk_get_stats --
kernel_ms = the score kernels (sample + sweep [+ redo], or the dense launches), aux_ms = pack, thresholds, selection.  The lists and
score bits of the two paths are compared on every round.  `--rows-cap` cuts both matrices (rehearsals at a small size)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

K = 10
NO_POOL = np.zeros(0, np.int32)


def line(name, runs):
    r = np.array(runs)
    return "  %-22s wall %8.2f [%8.2f .. %8.2f]   score kernels %8.2f [%8.2f .. %8.2f]   everything else %7.2f   handed back %d" % (
        name, np.median(r[:, 0]), r[:, 0].min(), r[:, 0].max(), np.median(r[:, 1]), r[:, 1].min(), r[:, 1].max(), np.median(r[:, 2]), int(r[-1, 3]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--rows-cap", type=int, default=0)
    args = ap.parse_args()
    import torch
    import eval_cases as ec
    from buffalo_amd import synth
    from buffalo_amd.parallel import TopK
    U, I, nnz = synth.SHAPES["ml20m"]
    if args.rows_cap:
        nnz = int(nnz * (min(U, args.rows_cap) / U) * (min(I, args.rows_cap) / I))
        U, I = min(U, args.rows_cap), min(I, args.rows_cap)
    train, _ = ec.hold_out(synth.generate(U, I, nnz, seed=7), seed=11)
    eng = TopK()
    eng.set_seen(train.indptr, train.keys, I)
    users = np.arange(U, dtype=np.int32)
    keys = {f: np.empty((U, K), np.int32) for f in (0, 1)}
    scores = {f: np.empty((U, K), np.float32) for f in (0, 1)}
    print("# fused sweep for 128 < d <= 256 -- first device run, one MI355X; times of one box, one process.  %d x %d, k = %d, %d training entries;"
          % (U, I, K, train.nnz))
    print("# factors in HBM; ms, median [min .. max] of %d runs after one warm-up round; \"fused\" = 0 and 1 (recommend_unseen: -1, the default rule) alternate on one handle." % args.runs)
    sweep = {}
    for d in (256, 192, 128):
        rng = np.random.default_rng(20 + d)
        tP = torch.from_numpy(rng.standard_normal((U, d), dtype=np.float32)).cuda()
        tQ = torch.from_numpy(rng.standard_normal((I, d), dtype=np.float32)).cuda()
        torch.cuda.synchronize()

        def call(what, fused):
            eng.set_mode("fused", 0 if not fused else (1 if what == "topn" else -1))
            eng.reset_stats()
            t0 = time.perf_counter()
            if what == "topn":
                eng.dot_topn_device(users, tP.data_ptr(), U, tQ.data_ptr(), I, d, d, None, False, keys[fused], scores[fused], NO_POOL, K)
            else:
                eng.recommend_unseen_device(users, tP.data_ptr(), U, tQ.data_ptr(), I, d, d, None, keys[fused], scores[fused], NO_POOL, K)
            wall = (time.perf_counter() - t0) * 1e3
            st = eng.stats()
            return wall, st["kernel_ms"], st["aux_ms"], st["merges"]

        for what, label in (("topn", "dot_topn_device"), ("unseen", "recommend_unseen_device")):
            runs = {0: [], 1: []}
            for r in range(args.runs + 1):
                for fused in (0, 1):
                    got = call(what, fused)
                    if r:
                        runs[fused].append(got)
                assert np.array_equal(keys[0], keys[1]), "the fused lists differ from the dense path's"
                assert np.array_equal(scores[0].view(np.uint32), scores[1].view(np.uint32)), "score bits"
            print("d = %d, %s (lists and score bits of the two paths equal on every round)" % (d, label))
            print(line("dense  (\"fused\" = 0)", runs[0]))
            print(line("fused  (\"fused\" = %d)" % (1 if what == "topn" else -1), runs[1]))
            med = {f: np.median(np.array(runs[f]), axis=0) for f in (0, 1)}
            sweep[(d, what)] = med[1][1]
            print("  fused / dense: wall %.3f, score kernels %.3f, score kernels + everything else %.3f"
                  % (med[1][0] / med[0][0], med[1][1] / med[0][1], (med[1][1] + med[1][2]) / (med[0][1] + med[0][2])))
    for what in ("topn", "unseen"):
        print("%s: fused score kernels d = 256 / d = 128 = %.2f (twice the MFMAs), d = 192 / d = 128 = %.2f (1.5 times); d = 256: %.1f TFLOP/s over kernel_ms"
              % (what, sweep[(256, what)] / sweep[(128, what)], sweep[(192, what)] / sweep[(128, what)], 2.0 * U * I * 256 / sweep[(256, what)] / 1e9))


if __name__ == "__main__":
    main()
