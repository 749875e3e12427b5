"""Golden row normalisations, made by the REFERENCE's own `Algo._normalize` (TEST INFRASTRUCTURE).

    python tests/golden/make_similar_vectors.py [--out FILE]        # needs /root/reference; default: tests/golden/similar_vectors.npz

`buffalo/algo/base.py` is imported unchanged from where the reference lies (make_front_traces.install_reference supplies the compiled
modules this image lacks); `Algo._normalize` (base.py:26-28) uses nothing of its instance, so it is called on the class.  The inputs are
rebuilt by tests/similar_cases.golden_input(d) -- 40 rows per d, seed 9000 + d -- so only the seeds and the reference's OUTPUT are stored."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import make_front_traces as G  # noqa: E402
import similar_cases as sc  # noqa: E402

OUT = os.path.join(HERE, "similar_vectors.npz")


def reference_outputs():
    G.install_reference()
    from buffalo.algo.base import Algo
    out = {"ds": np.array(sc.NORMALIZE_DS, np.int32), "seeds": np.array([9000 + d for d in sc.NORMALIZE_DS], np.int32),
           "numpy": np.array(np.__version__)}
    for d in sc.NORMALIZE_DS:
        Fn = Algo._normalize(None, sc.golden_input(d))
        assert Fn.dtype == np.float32 and Fn.shape == (40, d)
        out["Fn_%d" % d] = Fn
    return out


if __name__ == "__main__":
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else OUT
    vec = reference_outputs()
    np.savez_compressed(path, **vec)
    print("wrote", path, os.path.getsize(path), "bytes,", len(vec), "arrays")
