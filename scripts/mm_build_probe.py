"""First timing of the MatrixMarket database builder (`bfh_mm_*`, csrc/mm.hip) on an ML-20M-shaped file.

    python scripts/mm_build_probe.py [--repeats 3] > profiles/mm_first_contact.txt

Input: buffalo_amd.synth's ML-20M-shaped matrix written as a coordinate file in row order, one "row col value" line per entry with the ids
zero-padded to a fixed width (sscanf's %d reads them as decimal) and ratings 0.5 .. 5.0, so the text is made by numpy and not by 20 M string
formats.  1 % of the lines held out, capped at 500 (the default option of the reference), drawn as base.py:220-226 draws them.
Device figures: host-to-host time of a warm build + both fetch_group + fetch_vali, and the HIP-event times of `bfh_stats` read after every call
(kernel_ms = line ends + parse; aux_ms of the build = upload, split, prepro, held-out sort; aux_ms of a fetch_group = its sort).
Yardstick: the path before this builder, same process: the split of the text on the host as mm.py:167-234 does it (restated with numpy line
indices), then one text_to_csr call per orientation.
Accuracy lines: ImplicitALS values of the device against the numpy restatement of tests/mm_cases.py (the correctly rounded value) on the small cases
of tests/test_mm_gpu.py, in float32 ulps.
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
HEAD = "%%%%MatrixMarket matrix coordinate real general\n%%\n%d %d %d\n"


def mm_text(m):
    """CSR -> bytes: "RRRRRR CCCCC V.V\\n" per entry, 17 bytes, ids 1-based."""
    nnz = m.nnz
    rows = np.repeat(np.arange(1, m.num_users + 1, dtype=np.int64), np.diff(np.concatenate([[0], m.indptr])))
    cols = m.keys.astype(np.int64) + 1
    half = (rows * 7 + cols * 3) % 10 + 1                 # rating = half / 2: 0.5 .. 5.0
    out = np.full((nnz, 17), ord(" "), np.uint8)
    for d in range(6):
        out[:, 5 - d] = 48 + rows % 10
        rows //= 10
    for d in range(5):
        out[:, 11 - d] = 48 + cols % 10
        cols //= 10
    out[:, 13] = 48 + half // 2
    out[:, 14] = ord(".")
    out[:, 15] = 48 + 5 * (half % 2)
    out[:, 16] = ord("\n")
    return (HEAD % (m.num_users, m.num_items, nnz)).encode() + out.tobytes(), (half / 2).astype(np.float32)


def host_split(text, skip_lines, num_nnz, positions):
    """mm.py:167-234 with numpy: the body without the held-out lines (the working text), and the held-out lines."""
    buf = np.frombuffer(text, np.uint8)
    ends = np.flatnonzero(buf == 10)
    body0 = int(ends[skip_lines - 1]) + 1
    starts = np.concatenate([[body0], ends[skip_lines:skip_lines + num_nnz - 1] + 1])
    stops = ends[skip_lines:skip_lines + num_nnz] + 1
    pieces, at = [], body0
    held = []
    for p in positions:
        pieces.append(text[at:int(starts[p])])
        held.append(text[int(starts[p]):int(stops[p])])
        at = int(stops[p])
    pieces.append(text[at:int(stops[num_nnz - 1])])
    return b"".join(pieces), held


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shape", default="ml20m")
    args = ap.parse_args()
    from buffalo_amd import synth
    from buffalo_amd.ingest import MatrixMarketBuilder, text_to_csr
    import mm_cases as mc

    U, I, nnz = synth.SHAPES[args.shape]
    m = synth.generate(U, I, nnz)
    text, vals = mm_text(m)
    nnz = m.nnz
    np.random.seed(3)
    sz = min(500, int(nnz * 0.01))
    positions = np.sort(np.random.choice(nnz - 1, sz, replace=False)).astype(np.int64)
    print("# MatrixMarket database builder (csrc/mm.hip) -- first device run, one MI355X.  Box-to-box caveat as everywhere in this directory:")
    print("# times of one box, one process.")
    print("input: %s shape, %d x %d, %d body lines of 17 bytes, text %.1f MB, %d lines held out" % (args.shape, U, I, nnz, len(text) / 1e6, sz))

    b = MatrixMarketBuilder()
    first_groups = None
    for label, (pname, kw) in (("none", (None, {})), ("OneBased", ("OneBased", {})), ("MinMaxScalar(1, 5)", ("MinMaxScalar", {"min": 1, "max": 5})),
                               ("ImplicitALS(0.5)", ("ImplicitALS", {"epsilon": 0.5}))):
        b.set_value_prepro(pname, **kw)
        walls, steps = [], []
        for rep in range(args.repeats + 1):          # one handle: the first run pays the allocations and is reported apart
            b.reset_stats()
            t0 = time.perf_counter()
            res = b.build(text, positions)
            s_build = b.stats()
            g1 = res.group(1)
            s_g1 = b.stats()
            g2 = res.group(2)
            s_g2 = b.stats()
            vali = res.vali()
            walls.append((time.perf_counter() - t0) * 1e3)
            steps.append((s_build["kernel_ms"], s_build["aux_ms"], s_g1["aux_ms"] - s_build["aux_ms"], s_g2["aux_ms"] - s_g1["aux_ms"]))
            last = b.stats()
        if pname is None:
            first_groups = (g1, g2, vali)
            keep = np.ones(nnz, bool)
            keep[positions] = False
            assert np.array_equal(g1["indptr"], np.cumsum(np.bincount(np.repeat(np.arange(U), np.diff(np.concatenate([[0], m.indptr])))[keep], minlength=U)))
            assert np.array_equal(g1["key"], m.keys[keep]) and np.array_equal(g1["val"], vals[keep]), "rowwise group differs from the matrix the text was written from"
            print("checked: the rowwise group equals the matrix the text was written from, without the held-out lines")
        st = np.array(steps[1:])
        print("%-18s host-to-host (build + group(1) + group(2) + vali): first %.1f ms, then median %.1f ms (min %.1f, max %.1f, %d runs)"
              % (label, walls[0], np.median(walls[1:]), min(walls[1:]), max(walls[1:]), args.repeats))
        print("%-18s HIP events, medians: line ends + parse %.2f ms | upload + split + prepro + held-out sort %.2f ms | rowwise sort %.2f ms | colwise sort %.2f ms"
              % ("", *np.median(st, axis=0)))
        if pname is None:
            k = float(np.median(st[:, 0]))
            tbps = len(text) / (k * 1e-3) / 1e12
            print("%-18s text bytes / kernel_ms = %.3f TB/s -- %.2f-%.2f of the STREAM triad the README quotes (%.2f / %.2f TB/s); lines parsed on the host: %d"
                  % ("", tbps, tbps / README_TRIAD_TBPS[1], tbps / README_TRIAD_TBPS[0], README_TRIAD_TBPS[0], README_TRIAD_TBPS[1], last["merges"]))
            print("%-18s bytes of one run: h2d %.1f MB, d2h %.1f MB" % ("", last["h2d_bytes"] / 1e6, last["d2h_bytes"] / 1e6))
    b.close()

    # the path before the builder: host split, then the text goes up and is parsed once per orientation
    walls, parts = [], []
    for rep in range(2):
        t0 = time.perf_counter()
        working, held = host_split(text, 3, nnz, positions)
        t1 = time.perf_counter()
        o1, s1 = text_to_csr(working, nnz - sz, U, I, 1, with_stats=True)
        o2, s2 = text_to_csr(working, nnz - sz, I, U, 2, with_stats=True)
        t2 = time.perf_counter()
        walls.append((t2 - t0) * 1e3)
        parts.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, s1["kernel_ms"] + s2["kernel_ms"], s1["h2d_bytes"] + s2["h2d_bytes"], s1["d2h_bytes"] + s2["d2h_bytes"]))
    for got, exp in ((first_groups[0], o1), (first_groups[1], o2)):
        assert all(got[k].tobytes() == exp[k].tobytes() for k in ("indptr", "key", "val")), "the builder's group differs from text_to_csr on the working text"
    assert len(held) == sz
    print("checked: both groups of the builder (no prepro) equal text_to_csr on the working text, bit for bit")
    p = parts[-1]
    print("path before (second of 2 runs): host split with numpy line indices %.1f ms + two text_to_csr calls %.1f ms = %.1f ms host-to-host; their HIP-event time %.2f ms;"
          " h2d %.1f MB, d2h %.1f MB" % (p[0], p[1], walls[-1], p[2], p[3] / 1e6, p[4] / 1e6))

    # accuracy of the ImplicitALS kernel against the correctly rounded restatement
    tile = mc.align_to_tile(mc.tile_text()).encode()
    pos, _ = mc.tile_positions(tile)
    b = MatrixMarketBuilder()
    b.set_value_prepro("ImplicitALS", epsilon=0.5)
    res = b.build(tile, pos)
    want = mc.restate(tile, pos, "ImplicitALS", epsilon=0.5)
    worst = max(int(mc.ulps(res.group(1)["val"], want["rowwise"]["val"]).max()), int(mc.ulps(res.group(2)["val"], want["colwise"]["val"]).max()),
                int(mc.ulps(res.vali()[2], want["vali"][2]).max()))
    print("ImplicitALS(0.5), tile case of tests/test_mm_gpu.py (3,000 lines): largest distance to the correctly rounded restatement %d ulp" % worst)
    b.close()


if __name__ == "__main__":
    main()
