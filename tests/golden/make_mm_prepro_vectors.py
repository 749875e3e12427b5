"""Golden MatrixMarket databases with `data.value_prepro`, made by the REFERENCE's own data package (TEST INFRASTRUCTURE).

    python tests/golden/make_mm_prepro_vectors.py [--out FILE]        # needs /root/reference; default: tests/golden/mm_prepro_vectors.npz

make_data_vectors.py is imported unchanged for the setup that runs `MatrixMarket(opt).create()` here (install, _merge, _mm_text, _write).
Only what the reference wrote is stored: both groups cut to attrs["num_nnz"] (the tail of key / val is padding, base.py:185-194), vali/*
with the drawn `indexes`, the attrs.  One meta field is added, `ials_ref_ulp`: the largest float32-ulp distance between the reference's
ImplicitALS values (numpy's float32 log on this CPU) and the correctly rounded restatement of tests/mm_cases.py, measured here.
The inputs are rebuilt by `inputs()` below, so the tests regenerate them and only the reference's OUTPUT is stored."""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import make_data_vectors as mk  # noqa: E402
import mm_cases as mc  # noqa: E402

OUT = os.path.join(HERE, "mm_prepro_vectors.npz")
SAMPLE = {"name": "sample", "p": 0.1, "max_samples": 30}


def inputs():
    """name -> (text, value_prepro option or None, validation option, numpy seed or None)"""
    base = mk._mm_text(60, 40, 0.2, 1, real=True)
    minmax = {"name": "MinMaxScalar", "min": 1, "max": 5}
    return {
        "none_seed3": (base, None, SAMPLE, 3),
        "onebased_seed3": (base, {"name": "OneBased"}, SAMPLE, 3),
        "minmax_seed3": (base, minmax, SAMPLE, 3),
        "minmax_seed5": (base, minmax, SAMPLE, 5),
        "minmax_seed4": (base, minmax, SAMPLE, 4),
        "ials_seed3": (base, {"name": "ImplicitALS", "epsilon": 0.5}, SAMPLE, 3),
        "minmax_constant": (mc.CONSTANT_TEXT, minmax, {}, None),
        "none_seed3_crlf": (mc.as_crlf(base), None, SAMPLE, 3),
        "none_seed3_open_end": (mc.without_final_newline(base), None, SAMPLE, 3),
        "none_seed3_comments": (mc.with_extra_comments(base), None, SAMPLE, 3),
    }


def prepro_args(opt):
    """value_prepro option -> (name, keyword arguments) of mm_cases.restate / MatrixMarketBuilder.set_value_prepro"""
    return (None, {}) if not opt else (opt["name"], {k: v for k, v in opt.items() if k != "name"})


def reference_databases():
    h5 = mk.install()
    from buffalo.data.mm import MatrixMarket, MatrixMarketOptions
    from buffalo.misc import aux
    out, meta = {}, {}
    with tempfile.TemporaryDirectory() as d:
        work = os.path.join(d, "work")
        os.makedirs(work)
        for name, (text, prepro, vali, seed) in inputs().items():
            main = os.path.join(d, name + ".mtx")
            with open(main, "w", newline="") as f:                            # the bytes as given: no newline translation
                f.write(text)
            opt = MatrixMarketOptions().get_default_option()
            mk._merge(opt, {"input": {"main": main, "uid": None, "iid": None}, "data": {"validation": vali, "value_prepro": prepro or {}}})
            opt.data.tmp_dir = work
            opt.data.path = os.path.join(d, name + ".h5py")
            opt = aux.Option(opt)
            if seed is not None:
                np.random.seed(seed)
            data = MatrixMarket(opt)
            data.create()
            t = h5.tree(data.handle)
            meta[name] = {k: int(v) for k, v in t["@attrs"].items()}
            meta[name]["header"] = {k: int(v) for k, v in data.get_header().items()}
            n = meta[name]["num_nnz"]
            for g in ("rowwise", "colwise"):
                out["%s/%s/indptr" % (name, g)] = t[g]["indptr"]
                out["%s/%s/key" % (name, g)] = t[g]["key"][:n]
                out["%s/%s/val" % (name, g)] = t[g]["val"][:n]
            if "vali" in t:
                meta[name]["vali"] = {k: (v if isinstance(v, str) else int(v)) for k, v in t["vali"]["@attrs"].items()}
                for k, v in t["vali"].items():
                    if k != "@attrs":
                        out["%s/vali/%s" % (name, k)] = v
            assert not os.listdir(work), "the reference left temporary files behind"
    worst = 0
    for name, (text, prepro, vali, seed) in inputs().items():
        if prepro and prepro["name"] == "ImplicitALS":
            pname, kw = prepro_args(prepro)
            r = mc.restate(text.encode(), np.sort(out[name + "/vali/indexes"]), pname, **kw)
            for ours, ref in ((r["rowwise"]["val"], out[name + "/rowwise/val"]), (r["colwise"]["val"], out[name + "/colwise/val"]),
                              (r["vali"][2], out[name + "/vali/val"])):
                worst = max(worst, int(mc.ulps(ours, ref).max()))
    meta["ials_ref_ulp"] = worst
    out["meta"] = np.array(json.dumps(meta, sort_keys=True))
    return out


if __name__ == "__main__":
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else OUT
    vec = reference_databases()
    np.savez_compressed(path, **vec)
    print("wrote", path, os.path.getsize(path), "bytes,", len(vec), "arrays; ials_ref_ulp =", json.loads(str(vec["meta"]))["ials_ref_ulp"])
