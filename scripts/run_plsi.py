"""pLSI epochs at the ML-20M shape without torch: the timing behind the pLSI row of the README and the target of a rocprofv3 pass.
    python scripts/run_plsi.py [d=20] [epochs=24] [warmup=3] [mode=resident|batched] [batches=8] [out=FILE]
138,493 x 27,278, 20 M entries (bench.py's synthetic matrix).  Prints one line per epoch -- wall ms and the split from bfh_plsi_get_stats
(P half-step / transpose / Q half-step / normalise / copy-back) -- and a summary line: the medians after the warm-up epochs and the
algorithmic bytes per epoch, entries x (8 + 2 x 4 vdim) + the factor writes, over the median kernel time."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from buffalo_amd.backend import CyPLSI  # noqa: E402

modes = dict(kv.split("=") for kv in sys.argv[1:])
d = int(modes.pop("d", 20))
epochs = int(modes.pop("epochs", 24))
warmup = int(modes.pop("warmup", 3))
mode = modes.pop("mode", "resident")
n_batches = int(modes.pop("batches", 8))
out_path = modes.pop("out", "")
csr = bench.load_matrix("ml20m", 7)
U, I, nnz = csr.num_users, csr.num_items, csr.nnz
P, Q = np.zeros((U, d), dtype=np.float32), np.zeros((I, d), dtype=np.float32)
g = CyPLSI()
path = bench._opt_file({"d": d, "random_seed": 7, "num_workers": 1})
assert g.init(path)
os.unlink(path)
g.initialize_model(P, Q)
vdim = g.get_vdim()
if mode == "resident":
    g.set_resident_csr(csr.indptr, csr.keys, csr.vals)
edges = np.linspace(0, U, n_batches + 1).astype(int)
rows = []
for e in range(warmup + epochs):
    g.reset_stats()
    t0 = time.perf_counter()
    g.reset()
    if mode == "resident":
        loss = g.update_resident()
    else:
        loss = 0.0
        for a, b in zip(edges[:-1], edges[1:]):
            beg, end = (0 if a == 0 else int(csr.indptr[a - 1])), int(csr.indptr[b - 1])
            loss += g.partial_update(int(a), int(b), csr.indptr, csr.keys[beg:end], csr.vals[beg:end])
    g.normalize(1.0, 1.0)
    g.swap()
    wall = (time.perf_counter() - t0) * 1e3
    st = g.get_stats()
    rows.append({"wall_ms": wall, "p_ms": st["kernel_ms"], "transpose_ms": st["aux_ms"], "q_ms": st["optimizer_ms"],
                 "normalise_ms": st["exchange_kernel_ms"], "copy_back_ms": st["allreduce_ms"], "split_owners": st["merges"], "loss": loss / nnz})
    print("run_plsi", mode, "d", d, "epoch", e, json.dumps(rows[-1]), flush=True)
kept = rows[warmup:]
med = {k: float(np.median([r[k] for r in kept])) for k in kept[0] if k.endswith("_ms")}
kernel_ms = med["p_ms"] + med["q_ms"] + med["normalise_ms"] + med["transpose_ms"]
alg_bytes = nnz * (8 + 2 * 4 * vdim) + 2 * 4.0 * (U + I) * vdim        # both half-steps gather one row per entry; every new row is written once (+ normalised)
summary = {"mode": mode, "d": d, "vdim": vdim, "U": U, "I": I, "nnz": nnz, "epochs": len(kept), "median": med,
           "algorithmic_bytes": alg_bytes, "algorithmic_gbs_over_kernel_time": alg_bytes / (kernel_ms * 1e-3) / 1e9,
           "p_pass_rows_per_s": nnz / (med["p_ms"] * 1e-3), "q_pass_rows_per_s": nnz / (med["q_ms"] * 1e-3)}
print("run_plsi summary", json.dumps(summary), flush=True)
if out_path:
    json.dump({"summary": summary, "epochs": rows}, open(out_path, "w"), indent=1)
