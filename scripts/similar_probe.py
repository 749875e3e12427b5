"""First timing of `most_similar` (`bfh_topk_most_similar[_device]`, `bfh_topk_normalize_device`; csrc/topk.hip) at the ML-20M shape, d = 128.

    python scripts/similar_probe.py [--repeats 3] [--rows-cap N] > profiles/similar_first_contact.txt

Factors: seeded normal matrices of the ML-20M shape (27,278 items, 138,493 users), 128 columns.  Two cases, the "neighbours of everything"
call (indexes = arange(rows), k = 10, no pool): (a) items, (b) users -- 138,493 x 138,493 on the fused path, no score buffer.
Per case, in one process, new and old call alternating, the first run of each (allocations) reported apart:
  new, host-to-host     most_similar(indexes, F): upload, normalise kernel, sweep, lists back; host clock around the call (it ends in a
                        stream synchronise), HIP-event times from bfh_stats (kernel_ms = score kernels, aux_ms = everything else)
  new, from HBM         most_similar_device on a torch tensor that holds F
  normalise alone       normalize_device, out of place: its own HIP-event time (aux_ms), as a fraction of the sweep it precedes
  old, host-to-host     what the call replaces: numpy `_normalize` (algo/base.py:26-28) on the host, then dot_topn(indexes, Fn, Fn)
  old, from HBM         the same when the factors live in HBM: copy back, numpy, dot_topn
Checked on the way: the new lists equal the old ones, keys and score bits.  `--rows-cap` cuts both matrices (rehearsals at a small size)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, K = 128, 10
EMPTY_POOL = np.array([], dtype=np.int32)
NO_BIAS = np.array([[]], dtype=np.float32)


def numpy_normalize(feat):
    return feat / np.sqrt((feat ** 2).sum(-1) + 1e-8)[..., np.newaxis]


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def med(xs):
    xs = list(xs)
    return "first %.1f ms, then median %.1f ms (min %.1f, max %.1f, %d runs)" % (xs[0], np.median(xs[1:]), min(xs[1:]), max(xs[1:]), len(xs) - 1)


def case(label, rows, seed, repeats):
    import torch
    from buffalo_amd import parallel as par
    rng = np.random.default_rng(seed)
    F = rng.normal(scale=0.1, size=(rows, D)).astype(np.float32)
    idx = np.arange(rows, dtype=np.int32)
    eng = par.TopK()
    dF = torch.from_numpy(F).cuda()
    dOut = torch.empty_like(dF)
    torch.cuda.synchronize()
    new = (np.empty((rows, K), np.int32), np.empty((rows, K), np.float32))
    dev = (np.empty((rows, K), np.int32), np.empty((rows, K), np.float32))
    old = (np.empty((rows, K), np.int32), np.empty((rows, K), np.float32))

    def stats_of(fn):
        eng.reset_stats()
        ms, _ = timed(fn)
        s = eng.stats()
        return ms, s["kernel_ms"], s["aux_ms"], s["merges"]

    def old_host(src):
        t_np, Fn = timed(lambda: np.ascontiguousarray(numpy_normalize(src())))
        ms, k_ms, a_ms, _ = stats_of(lambda: eng.dot_topn(idx, Fn, Fn, NO_BIAS, old[0], old[1], EMPTY_POOL, K))
        return t_np + ms, t_np, k_ms, a_ms

    runs = {"new_host": [], "new_hbm": [], "norm": [], "old_host": [], "old_hbm": []}
    for rep in range(repeats + 1):
        runs["new_host"].append(stats_of(lambda: eng.most_similar(idx, F, new[0], new[1], EMPTY_POOL, K)))
        runs["old_host"].append(old_host(lambda: F))
        runs["new_hbm"].append(stats_of(lambda: eng.most_similar_device(idx, dF.data_ptr(), rows, D, D, dev[0], dev[1], EMPTY_POOL, K)))
        runs["old_hbm"].append(old_host(lambda: dF.cpu().numpy()))
        runs["norm"].append(stats_of(lambda: eng.normalize_device(dF.data_ptr(), rows, D, D, dOut.data_ptr())))
        if rep == 0:
            for got, name in ((new, "host"), (dev, "HBM")):
                assert np.array_equal(got[0], old[0]) and np.array_equal(got[1].view(np.uint32), old[1].view(np.uint32)), \
                    "%s: most_similar (%s) differs from numpy _normalize + dot_topn" % (label, name)
            assert np.array_equal(dOut.cpu().numpy().view(np.uint32), np.ascontiguousarray(numpy_normalize(F)).view(np.uint32))
    print("%s: %d x %d, d = %d, k = %d; factor matrix %.1f MB; rows the fused path handed back: %d"
          % (label, rows, rows, D, K, rows * D * 4 / 1e6, runs["new_host"][-1][3]))
    print("  checked: most_similar (host and HBM) == numpy _normalize + dot_topn, keys and score bits; normalize_device == numpy _normalize, bits")
    for key, name in (("new_host", "new, host-to-host"), ("new_hbm", "new, from HBM    ")):
        r = np.array(runs[key])
        print("  %s  %s; HIP events, medians: score kernels %.2f ms | everything else (normalise, pack, select) %.2f ms"
              % (name, med(r[:, 0]), np.median(r[1:, 1]), np.median(r[1:, 2])))
    r = np.array(runs["norm"])
    sweep = float(np.median(np.array(runs["new_hbm"])[1:, 1]))
    n_ms = float(np.median(r[1:, 2]))
    print("  normalise alone    HIP events: first %.3f ms, then median %.3f ms (min %.3f, max %.3f) = %.4f of the score kernels it precedes;"
          " read + write %.1f MB -> %.2f TB/s" % (r[0, 2], n_ms, r[1:, 2].min(), r[1:, 2].max(), n_ms / sweep, 2 * rows * D * 4 / 1e6,
                                                  2 * rows * D * 4 / (n_ms * 1e-3) / 1e12))
    for key, name in (("old_host", "old, host-to-host"), ("old_hbm", "old, from HBM    ")):
        r = np.array(runs[key])
        print("  %s  %s; of it numpy _normalize%s median %.1f ms; HIP events, medians: score kernels %.2f ms | everything else %.2f ms"
              % (name, med(r[:, 0]), " (+ copy back)" if key == "old_hbm" else "", np.median(r[1:, 1]), np.median(r[1:, 2]), np.median(r[1:, 3])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rows-cap", type=int, default=0)
    args = ap.parse_args()
    from buffalo_amd import synth
    U, I, _ = synth.SHAPES["ml20m"]
    if args.rows_cap:
        U, I = min(U, args.rows_cap), min(I, args.rows_cap)
    print("# most_similar (csrc/topk.hip, topk_normalize_kernel) -- first device run, one MI355X.  Box-to-box caveat as everywhere in this")
    print("# directory: times of one box, one process.  New and old calls alternate; every time is a host clock around a call that ends in a")
    print("# stream synchronise, or a HIP-event sum from bfh_stats.")
    case("(a) items", I, 1, args.repeats)
    case("(b) users", U, 2, args.repeats)


if __name__ == "__main__":
    main()
