"""The numpy restatement of MatrixMarket databases (tests/mm_cases.py) against the databases the REFERENCE's own MatrixMarket.create() built:
the three MatrixMarket cases of tests/golden/data_vectors.npz and every case of tests/golden/mm_prepro_vectors.npz (value_prepro, line-end
forms; see tests/golden/make_mm_prepro_vectors.py).  No GPU: this pins the yardstick tests/test_mm_gpu.py holds the device builder to.

Everything is compared exactly, with one exception: ImplicitALS values must lie within `ials_ref_ulp` (the distance measured when the fixture
was made) of the fixture's -- the reference's numpy float32 log depends on the CPU, the restatement is the correctly rounded value."""
import json
import os
import sys

import numpy as np
import pytest

import mm_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_data_vectors as mk  # noqa: E402
import make_mm_prepro_vectors as mp  # noqa: E402

OLD, NEW = np.load(mk.OUT), np.load(mp.OUT)
OLD_META, NEW_META = json.loads(str(OLD["meta"])), json.loads(str(NEW["meta"]))
OLD_CASES = ["mm_reference_test", "mm_sampled_validation", "mm_real_values_no_validation"]
NEW_CASES = sorted(mp.inputs())
ALL_CASES = OLD_CASES + NEW_CASES


def golden_inputs(tmp_dir, name):
    """(text bytes, sorted sample positions or None, prepro name, prepro arguments, the golden arrays of the case, its meta)"""
    if name in OLD_CASES:
        kind, over, seed = mk.cases(str(tmp_dir))[name]
        assert kind == "mm"
        with open(over["input"]["main"], "rb") as f:
            text = f.read()
        vali, prepro, gold, meta = over.get("data", {}).get("validation", {"name": "sample", "p": 0.01, "max_samples": 500}), None, OLD, OLD_META[name]
    else:
        text, prepro, vali, seed = mp.inputs()[name]
        text, gold, meta = text.encode(), NEW, NEW_META[name]
    want = {k[len(name) + 1:]: gold[k] for k in gold.files if k.startswith(name + "/")}
    positions = None
    if vali.get("name") == "sample":                                     # base.py:220-226
        num_nnz = mc.header(mc.lines_of(text))[2]
        np.random.seed(seed)
        sz = min(vali["max_samples"], int(num_nnz * vali["p"]))
        drawn = np.random.choice(num_nnz - 1, sz, replace=False)
        assert np.array_equal(drawn, want["vali/indexes"])
        positions = np.sort(drawn)
    pname, kw = mp.prepro_args(prepro)
    return text, positions, pname, kw, want, meta


def same_values(got, want, pname, ulp, what):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, what
    if pname == "ImplicitALS":
        assert mc.ulps(got, want).max() <= ulp, (what, int(mc.ulps(got, want).max()))
    else:
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), what


def check_against_golden(want, meta, pname, ulp, header, groups, vali):
    """header / {1: group, 2: group} / vali() of ANY builder against one golden database; `ulp` = the allowance for ImplicitALS values."""
    n = meta["num_nnz"]                                                  # attrs["num_nnz"]: the train entries
    assert (header["num_users"], header["num_items"], header["num_train"]) == (meta["num_users"], meta["num_items"], n)
    assert header["num_nnz"] == n + header["num_vali"]
    for sort_key, g in ((1, "rowwise"), (2, "colwise")):
        got = groups[sort_key]
        assert got["indptr"].dtype == np.int64 and np.array_equal(got["indptr"], want[g + "/indptr"]), g
        assert got["key"].dtype == np.int32 and np.array_equal(got["key"], want[g + "/key"][:n]), g
        same_values(got["val"], want[g + "/val"][:n], pname, ulp, g)
    rows, cols, vals = vali
    if "vali/row" in want:
        assert len(rows) == meta["vali"]["num_samples"] == header["num_vali"]
        assert np.array_equal(rows, want["vali/row"]) and np.array_equal(cols, want["vali/col"])
        same_values(vals, want["vali/val"], pname, ulp, "vali")
    else:
        assert len(rows) == len(cols) == len(vals) == header["num_vali"] == 0


@pytest.mark.parametrize("name", ALL_CASES)
def test_restatement_builds_the_reference_database(tmp_path, name):
    text, positions, pname, kw, want, meta = golden_inputs(tmp_path, name)
    r = mc.restate(text, positions, pname, **kw)
    check_against_golden(want, meta, pname, NEW_META["ials_ref_ulp"], r["header"], {1: r["rowwise"], 2: r["colwise"]}, r["vali"])


def test_the_fixture_holds_what_the_issue_lists():
    assert NEW_META["ials_ref_ulp"] <= 1
    r = {s: mc.restate(*golden_inputs(None, "minmax_seed%d" % s)[:2], "MinMaxScalar", min=1, max=5) for s in (3, 4, 5)}
    widened = {s: not np.array_equal(v["value_range"][:2], v["value_range"][2:]) for s, v in r.items()}
    assert widened == {3: True, 4: False, 5: True}                       # the held-out values widen the range on seeds 3 and 5 only
    const = mc.restate(mc.CONSTANT_TEXT.encode(), None, "MinMaxScalar", min=1, max=5)
    assert np.array_equal(const["rowwise"]["val"], np.full(5, 5.0, np.float32))


def test_restatement_refuses_what_the_reference_cannot_build():
    text = mk._mm_text(60, 40, 0.2, 1, real=True).encode()
    with pytest.raises(ValueError, match="listed twice"):
        mc.restate(text, [53, 64])                                       # the same (row, col) on both lines
    nnz = mc.header(mc.lines_of(text))[2]
    for bad in ([5, 5], [7, 3], [nnz - 1], [-1]):
        with pytest.raises(ValueError, match="sample positions"):
            mc.restate(text, bad)
    with pytest.raises(ValueError, match="body lines"):
        mc.restate(text[:text.rindex(b"\n", 0, len(text) - 1) + 1])
    with pytest.raises(ValueError, match="disagree"):
        mc.restate(b" % indented comment\n" + text)
