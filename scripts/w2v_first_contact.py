"""First device figures of Word2Vec (csrc/w2v.hip): the ML-20M-shaped synthetic of buffalo_amd/synth.py read as one sentence per user, window 5,
5 negatives, d = 20 and d = 128, both "hogwild_atomic" settings, alternating.  Per setting: one warm-up epoch, then `epochs` timed ones;
words/s and pairs/s per epoch from a host clock around add_jobs (which ends in a device synchronise), ms of steps a + b (aux_ms) and c
(kernel_ms, HIP events), and the byte model of step c: (num_negative_samples + 2) rows read and as many written per pair at vdim * 4 bytes.
Then the planted-stream quality of tests/test_w2v_gpu.py for both settings.  No CPU baseline: the reference's trainer is not built here.

    python scripts/w2v_first_contact.py [users=138493 items=27278 nnz=20000000 epochs=3 out=FILE]     (out: also write the lines to FILE)
"""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ATOMIC_RATE = 1.3e12       # chip-wide float-atomic rate, bytes added per second (MI355X_MICROARCH.md, "Global float atomics")
STORE_RATE = 4.5 * 1.3e12  # plain stores of the same shape: "about 4-5 times the atomic rate" (same section)


def new_object(opt, **modes):
    from buffalo_amd.backend import CyW2V
    g = CyW2V()
    with tempfile.NamedTemporaryFile("w", suffix=".json", delete=False) as f:
        json.dump(opt, f)
    try:
        assert g.init(f.name)
    finally:
        os.unlink(f.name)
    for k, v in modes.items():
        g.set_mode(k, v)
    return g


def measure(lines, csr, vocab, d, atomic, epochs):
    opt = {"d": d, "window": 5, "num_negative_samples": 5, "num_iters": epochs + 1, "lr": 0.025, "min_lr": 0.0001, "random_seed": 1, "batch_size": -1,
           "compute_loss_on_training": False, "num_workers": 1}
    L0 = np.abs(np.random.default_rng(3).normal(scale=1.0 / d ** 2, size=(vocab["size"], d))).astype(np.float32)
    g = new_object(opt, hogwild_atomic=atomic)
    g.initialize_model(L0, vocab["index"], vocab["scale"], vocab["dist"], vocab["total_word_count"])
    g.launch_workers()
    vdim, words = g.get_vdim(), int(csr.keys.shape[0])
    for e in range(epochs + 1):
        g.reset_stats()
        t0 = time.perf_counter()
        g.add_jobs(0, csr.num_users, csr.indptr, csr.keys)
        wall = time.perf_counter() - t0
        st = g.stats()
        moved = st["samples"] * 7 * vdim * 4
        rate = ATOMIC_RATE if atomic else STORE_RATE
        lines.append("d=%3d vdim=%3d hogwild_atomic=%d %s: wall %8.1f ms  %7.2f M words/s  %7.2f M pairs/s | a+b %7.2f ms  c %8.2f ms | kept %d pairs %d redraws %d | "
                     "c moves %.2f GB read + %.2f GB written = %.3f TB/s written; written bytes / %s rate %.1f TB/s = %.1f ms = %.0f %% of c"
                     % (d, vdim, atomic, "warm-up" if e == 0 else "epoch %d" % e, wall * 1e3, words / wall / 1e6, st["samples"] / wall / 1e6, st["aux_ms"], st["kernel_ms"],
                        st["accepted"], st["samples"], st["loaded_rows"], moved / 1e9, moved / 1e9, moved / (st["kernel_ms"] * 1e-3) / 1e12,
                        "atomic" if atomic else "plain-store", rate / 1e12, moved / rate * 1e3, 100.0 * (moved / rate * 1e3) / st["kernel_ms"]))
        print(lines[-1], flush=True)
    g.join()
    assert np.isfinite(L0).all()


def quality(lines):
    import ref_w2v as R
    for atomic in (1, 0):
        out = []
        for seed in range(5):
            indptr, seq = R.make_stream(R.planted_stream(seed))
            vocab = R.vocab_of_stream(seq, 64)
            opt = {"d": 20, "window": 5, "num_negative_samples": 5, "num_iters": 1, "lr": 0.05, "min_lr": 0.005, "random_seed": seed, "batch_size": -1, "num_workers": 1}
            L0 = R.init_L0(seed, 64, 20)
            g = new_object(opt, hogwild_atomic=atomic)
            g.initialize_model(L0, vocab["index"], vocab["scale"], vocab["dist"], vocab["total_word_count"])
            g.launch_workers()
            g.add_jobs(0, len(indptr), indptr, seq)
            g.join()
            out.append(R.group_share(L0))
        lines.append("planted stream (64 words in 8 groups, 200 sentences of 12, 1 epoch), hogwild_atomic=%d: share of words with 3 own-group neighbours %s mean %.4f"
                     % (atomic, out, float(np.mean(out))))
        print(lines[-1], flush=True)


def main():
    args = dict(a.split("=", 1) for a in sys.argv[1:])
    users, items, nnz = int(args.get("users", 138493)), int(args.get("items", 27278)), int(args.get("nnz", 20000000))
    epochs, out = int(args.get("epochs", 3)), args.get("out")
    import torch
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    import ref_w2v as R
    from buffalo_amd import synth
    t0 = time.perf_counter()
    csr = synth.generate(users, items, nnz)
    vocab = R.build_vocab(np.bincount(csr.keys, minlength=items), 5, 0.001)
    lines = ["input: synth.generate(%d, %d, %d): %d sentences, %d words, vocabulary %d of %d (min_count 5, sample 0.001), made in %.1f s on the host"
             % (users, items, nnz, csr.num_users, csr.keys.shape[0], vocab["size"], items, time.perf_counter() - t0),
             "device: %s" % torch.cuda.get_device_name(0)]
    print("\n".join(lines), flush=True)
    for d in (20, 128):
        for atomic in (1, 0, 1, 0)[:2 if epochs < 2 else 4]:
            measure(lines, csr, vocab, d, atomic, epochs)
    quality(lines)
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
