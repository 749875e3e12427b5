"""First timing of the Stream database builder (`bfh_stream_*`, csrc/stream.hip) on an ML-20M-shaped stream.

    python scripts/stream_first_contact.py [--repeats 5] > profiles/stream_first_contact.txt

Input: buffalo_amd.synth's ML-20M-shaped matrix written as a stream file -- one line per user, its items as names "i%05d" separated by one space.
Device figures: host-to-host time of set_vocabulary + build + fetch_events + fetch_counts and the HIP-event times of `bfh_stats`.
Python yardstick: the restatement of tests/stream_cases.py (str.split + dict + Counter, as stream.py:197-271 works) on the first 1/16 of the users
-- a SLICE, the whole file is not run -- and np.bincount over the fetched items as the floor for the counts.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

README_TRIAD_TBPS = (5.76, 6.15)      # STREAM triad the README quotes (two-valued per process, another process, another box)


def stream_text(m):
    """CSR -> bytes: fixed-width names, ' ' between the items of a user, '\\n' after the last (synth makes no empty rows)."""
    nnz = m.nnz
    out = np.empty((nnz, 7), np.uint8)
    out[:, 0] = ord("i")
    k = m.keys.astype(np.int64)
    for d in range(5):
        out[:, 5 - d] = 48 + (k % 10)
        k //= 10
    out[:, 6] = ord(" ")
    out[m.indptr - 1, 6] = ord("\n")
    return out.tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shape", default="ml20m")
    args = ap.parse_args()
    from buffalo_amd import synth
    from buffalo_amd.ingest import StreamBuilder
    import stream_cases as sc

    U, I, nnz = synth.SHAPES[args.shape]
    m = synth.generate(U, I, nnz)
    text = stream_text(m)
    names = "".join("i%05d\n" % i for i in range(I)).encode()
    print("# Stream database builder (csrc/stream.hip) -- first device run, one MI355X.  Box-to-box caveat as everywhere in this directory:")
    print("# times of one box, one process.")
    print("input: %s shape, %d users, %d items, %d tokens, text %.1f MB, names %.2f MB" % (args.shape, U, I, m.nnz, len(text) / 1e6, len(names) / 1e6))

    walls, stats = [], []
    b = StreamBuilder()
    for rep in range(args.repeats + 1):          # one handle: the first run pays the allocations and is reported apart
        b.reset_stats()
        t0 = time.perf_counter()
        b.set_vocabulary(names)
        res = b.build(text)
        indptr, items = res.events()
        counts = res.item_counts()
        walls.append((time.perf_counter() - t0) * 1e3)
        stats.append(b.stats())
        if rep == 0:
            assert res.counts == {"num_users": U, "num_events": m.nnz, "num_train": m.nnz, "num_records": m.nnz, "num_vali": 0}, res.counts
            assert np.array_equal(indptr, m.indptr) and np.array_equal(items, m.keys), "events differ from the matrix the text was written from"
    b.close()
    t0 = time.perf_counter()
    floor = np.bincount(items, minlength=I)
    bincount_ms = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(floor, counts)
    print("checked: events() equals the matrix the text was written from; item_counts() equals np.bincount")
    print("host-to-host, one handle (set_vocabulary + build + fetch_events + fetch_counts): first %.1f ms, then median %.1f ms (min %.1f, max %.1f, %d runs)"
          % (walls[0], np.median(walls[1:]), min(walls[1:]), max(walls[1:]), args.repeats))
    k = np.array([s["kernel_ms"] for s in stats[1:]])
    a = np.array([s["aux_ms"] for s in stats[1:]])
    print("HIP events: kernel_ms (token boundaries + lookup) median %.2f ms (min %.2f); aux_ms (uploads, table build, splits, two sorts per list, counts) median %.2f ms"
          % (np.median(k), k.min(), np.median(a)))
    tbps = len(text) / (np.median(k) * 1e-3) / 1e12
    print("text bytes / kernel_ms = %.3f TB/s -- %.2f-%.2f of the STREAM triad the README quotes (%.2f / %.2f TB/s)"
          % (tbps, tbps / README_TRIAD_TBPS[1], tbps / README_TRIAD_TBPS[0], README_TRIAD_TBPS[0], README_TRIAD_TBPS[1]))
    print("passes over the text: 2 full (count marks, write marks: 16-byte loads) + 1 over the token bytes (hash + compare, byte loads by the token's thread);")
    print("  the upload of the text from pageable host memory is in aux_ms, not in kernel_ms")
    s = stats[-1]
    print("stats of one run: samples %d, accepted %d, merges %d, loaded_rows (extra probes) %d = %.3f per token, h2d %.1f MB, d2h %.1f MB"
          % (s["samples"], s["accepted"], s["merges"], s["loaded_rows"], s["loaded_rows"] / max(1, s["samples"]), s["h2d_bytes"] / 1e6, s["d2h_bytes"] / 1e6))

    cut_users = U // 16
    cut = int(m.indptr[cut_users - 1]) * 7
    t0 = time.perf_counter()
    want = sc.restate(names, text[:cut])
    py_ms = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(want["items"], items[:len(want["items"])])
    print("Python restatement (str.split + dict + Counter) on a SLICE, the first 1/16 of the users (%d users, %d tokens): %.0f ms -> %.1f s for the file by tokens (extrapolated, not run)"
          % (cut_users, len(want["items"]), py_ms, py_ms * m.nnz / max(1, len(want["items"])) / 1e3))
    print("np.bincount over the %d fetched items (the floor for the counts on the host): %.1f ms" % (len(items), bincount_ms))


if __name__ == "__main__":
    main()
