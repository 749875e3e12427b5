"""The plain-Python restatement of Stream databases (tests/stream_cases.py) against the databases the REFERENCE's own Stream.create() built
(tests/golden/data_vectors.npz, see tests/golden/make_data_vectors.py).  No GPU: this pins the yardstick tests/test_stream_gpu.py holds the
device builder to."""
import json
import os
import sys

import numpy as np
import pytest

import stream_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_data_vectors as mk  # noqa: E402

GOLDEN = np.load(mk.OUT)
META = json.loads(str(GOLDEN["meta"]))
STREAM_CASES = ["stream_reference_test_as_matrix", "stream_reference_test_keep_order", "stream_sppmi", "stream_sampled_validation"]


def golden_inputs(tmp_dir, name):
    """(names bytes, text bytes, internal_data_type, vali_n, sorted sample positions or None, the reference's header num_nnz) of a golden case:
    the input files are rebuilt by make_data_vectors.cases(), the split is derived as Stream._create / _create_validation derive it."""
    kind, over, seed = mk.cases(str(tmp_dir))[name]
    assert kind == "stream"
    with open(over["input"]["iid"], "rb") as f:
        names = f.read()
    with open(over["input"]["main"], "rb") as f:
        text = f.read()
    data = over.get("data", {})
    vali = data.get("validation", {"name": "newest", "n": 1})          # StreamOptions' default (stream.py:47-52)
    internal = data.get("internal_data_type", "stream")
    vali_n = vali.get("n", 0) if vali.get("name") == "newest" else 0    # stream.py:100-104
    positions = None
    if vali.get("name") == "sample":
        whole = sc.restate(names, text)                                  # the header count before the split: stream.py:113-119
        num_nnz = len(whole["records"][0]) if internal == "matrix" else len(whole["items"])
        np.random.seed(seed)
        sz = min(vali["max_samples"], int(num_nnz * vali["p"]))          # base.py:220-226
        drawn = np.random.choice(num_nnz - 1, sz, replace=False)
        assert np.array_equal(drawn, GOLDEN[name + "/vali/indexes"])
        positions = np.sort(drawn)
    return names, text, internal, vali_n, positions, META[name]["header"]["num_nnz"]


def check_against_golden(name, internal, num_nnz, counts, events, groups, vali):
    """counts / events() / {1: group, 2: group} cut at num_nnz / vali() of ANY builder against the golden database `name`."""
    want = {k[len(name) + 1:]: GOLDEN[k] for k in GOLDEN.files if k.startswith(name + "/")}
    head = META[name]["header"]
    assert (counts["num_users"], counts["num_items"]) == (head["num_users"], head["num_items"])
    if internal == "stream":                                             # order kept, rowwise only (stream.py:160-164)
        indptr, items = events
        assert len(items) == num_nnz
        assert np.array_equal(indptr, want["rowwise/indptr"]) and np.array_equal(items, want["rowwise/key"][:num_nnz])
        assert np.array_equal(want["rowwise/val"][:num_nnz], np.ones(num_nnz, np.float32))
    else:
        for sort_key, g in ((1, "rowwise"), (2, "colwise")):
            got = groups[sort_key]
            assert len(got["key"]) == num_nnz
            assert np.array_equal(got["indptr"], want[g + "/indptr"]), g
            # the reference allocates key / val before the validation samples are taken out (base.py:185-194): the tail stays zero
            assert np.array_equal(got["key"], want[g + "/key"][:num_nnz]) and not want[g + "/key"][num_nnz:].any(), g
            assert np.array_equal(got["val"].view(np.int32), want[g + "/val"][:num_nnz].view(np.int32)), g
    rows, cols, vals = vali
    assert len(rows) == META[name]["vali"]["num_samples"]                # base.py:244
    assert np.array_equal(rows, want["vali/row"]) and np.array_equal(cols, want["vali/col"])
    assert np.array_equal(sc.vali_values_reordered(rows, cols, vals), want["vali/val"])


@pytest.mark.parametrize("name", STREAM_CASES)
def test_restatement_builds_the_reference_database(tmp_path, name):
    names, text, internal, vali_n, positions, num_nnz = golden_inputs(tmp_path, name)
    r = sc.restate(names, text, vali_n, positions)
    if positions is None:                                                # the header count IS the number of working-file lines
        assert num_nnz == (len(r["records"][0]) if internal == "matrix" else len(r["items"]))
    groups = {k: sc.group(r["records"], nm, k, num_nnz) for k, nm in ((1, r["num_users"]), (2, r["num_items"]))}
    check_against_golden(name, internal, num_nnz, r, (r["indptr"], r["items"]), groups, r["vali"])
    assert np.array_equal(r["item_counts"], np.bincount(r["items"], minlength=r["num_items"]))
