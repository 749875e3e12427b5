"""Stream databases built on the device (`bfh_stream_*`, buffalo_amd.ingest.StreamBuilder) against the reference's own databases
(tests/golden/data_vectors.npz) and the plain-Python restatement tests/test_stream_ref_cpu.py pins to them (tests/stream_cases.py).
Every output is an integer array (or a count as a float): every check is exact equality."""
import ctypes as C

import numpy as np
import pytest

import stream_cases as sc
from test_stream_ref_cpu import STREAM_CASES, check_against_golden, golden_inputs

pytestmark = pytest.mark.gpu


def builder(names):
    from buffalo_amd.ingest import StreamBuilder
    return StreamBuilder(names)


# ---- 1. the four golden cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", STREAM_CASES)
def test_device_builds_the_reference_database(tmp_path, name):
    names, text, internal, vali_n, positions, num_nnz = golden_inputs(tmp_path, name)
    b = builder(names)
    res = b.build(text, vali_n=vali_n, sample_positions=positions)
    counts = dict(res.counts, num_items=b.num_items)
    events = res.events()
    groups = {k: res.group(k, num_nnz) for k in (1, 2)} if internal == "matrix" else None
    check_against_golden(name, internal, num_nnz, counts, events, groups, res.vali())
    assert np.array_equal(res.item_counts(), np.bincount(events[1], minlength=b.num_items))
    assert res.stats["samples"] == res.counts["num_events"] and res.stats["accepted"] == res.counts["num_train"]
    assert res.stats["merges"] == res.counts["num_records"] and res.stats["kernel_ms"] > 0


# ---- 2. boundaries -----------------------------------------------------------------------------------------------------------------------
BOUNDARY = sc.boundary_cases()


@pytest.mark.parametrize("name", sorted(BOUNDARY))
def test_boundaries_equal_the_restatement(name):
    names, text = BOUNDARY[name]
    b = builder(names)
    for vali_n in (0, 1, 50):   # no split; `newest` (a user with one event is never held out); n larger than every sequence
        sc.assert_same(b.build(text, vali_n=vali_n), sc.restate(names, text, vali_n), b.num_items)


# ---- 3. the table ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_items", [1, 2, 1000])
def test_table_with_near_equal_prefix_and_utf8_names(num_items):
    names = sc.mixed_names(num_items)
    text = sc.random_stream(names, 200, 30, num_items)
    b = builder(names)
    assert b.num_items == num_items
    res = b.build(text, vali_n=2)
    sc.assert_same(res, sc.restate(sc.names_file(names), text, 2), num_items)


def test_large_catalogue_takes_the_global_count_path():
    names = ["i%05d" % i for i in range(70001)]
    text = sc.random_stream(names, 5000, 0, 7, total=200000)
    b = builder(sc.names_file(names))
    assert b.num_items == 70001
    res = b.build(text)
    assert res.counts["num_events"] == 200000
    sc.assert_same(res, sc.restate(sc.names_file(names), text), 70001)
    assert res.stats["loaded_rows"] >= 0


def test_mid_catalogue_takes_the_one_block_per_cu_histogram():
    """20,001 items: above the size at which several LDS histograms share a CU, below the global-atomic path (an 80 KB histogram)."""
    names = ["i%05d" % i for i in range(20001)]
    text = sc.random_stream(names, 3000, 0, 9, total=60000)
    b = builder(sc.names_file(names))
    sc.assert_same(b.build(text, vali_n=1), sc.restate(sc.names_file(names), text, 1), 20001)


def test_vocabulary_from_the_text_when_no_names_are_given():
    text = b"pie apple\npie\n\x1cjuice\x1dapple\n"
    b = builder(None)
    res = b.build(text)
    assert b.names == b"apple\njuice\npie\n"
    sc.assert_same(res, sc.restate(b.names, text), 3)


# ---- 4. splits ---------------------------------------------------------------------------------------------------------------------------
SPLIT_NAMES = ["i%03d" % i for i in range(40)]


def split_text():
    lines = sc.random_stream(SPLIT_NAMES, 300, 24, 11).split(b"\n")[:-1]
    lines[5] = b"i003 i007 i003 i009"          # two positions of one user holding the same item
    return b"\n".join(lines) + b"\n"


def split_positions(text, how_many):
    whole = sc.restate(sc.names_file(SPLIT_NAMES), text)
    n = whole["num_events"]
    if how_many == 0:
        return np.zeros(0, np.int64)
    if how_many == 1:
        return np.array([n - 1], np.int64)
    first5 = int(whole["indptr"][4])
    fixed = {0, n - 1, first5, first5 + 2}
    rest = np.random.default_rng(5).permutation(np.setdiff1d(np.arange(n), list(fixed)))[:how_many - len(fixed)]
    return np.sort(np.concatenate([np.array(sorted(fixed)), rest])).astype(np.int64)


@pytest.mark.parametrize("vali_n", [1, 3])
def test_newest_split(vali_n):
    text, names = split_text(), sc.names_file(SPLIT_NAMES)
    b = builder(names)
    res = b.build(text, vali_n=vali_n)
    want = sc.restate(names, text, vali_n)
    sc.assert_same(res, want, 40)
    sc.assert_same(res, want, 40, cut=res.counts["num_records"] - 3)


@pytest.mark.parametrize("how_many", [0, 1, 37])
def test_sample_split(how_many):
    text, names = split_text(), sc.names_file(SPLIT_NAMES)
    pos = split_positions(text, how_many)
    assert len(pos) == how_many
    b = builder(names)
    res = b.build(text, sample_positions=pos)
    want = sc.restate(names, text, 0, pos)
    assert res.counts["num_events"] - res.counts["num_train"] == how_many
    sc.assert_same(res, want, 40)
    sc.assert_same(res, want, 40, cut=res.counts["num_records"] - 3)
    if how_many == 37:
        rows, cols, vals = res.vali()
        assert vals[(rows == 5) & (cols == 3)].tolist() == [2.0]      # the two sampled events of user 5 are one triple with count 2


# ---- 5. errors: BFH_ERR_INVALID with a message, never a fault ------------------------------------------------------------------------------
class Raw:
    """The C ABI without the wrapper: status codes and messages as they are."""

    def __init__(self, names=None):
        from buffalo_amd._lib import lib
        self.L = lib()
        self.h = self.L.bfh_stream_create()
        assert self.h
        self.num_items = None
        if names is not None:
            n = C.c_int(0)
            self.rc_vocab = self.L.bfh_stream_set_vocabulary(self.h, names, len(names), C.byref(n))
            self.num_items = n.value

    def build(self, text, vali_n=0, pos=None):
        out = (C.c_int64 * 5)()
        arr = None if pos is None else np.ascontiguousarray(pos, dtype=np.int64)
        ptr = None if arr is None else arr.ctypes.data_as(C.POINTER(C.c_int64))
        return self.L.bfh_stream_build(self.h, text, len(text), vali_n, ptr, 0 if arr is None else len(arr), out), list(out)

    def message(self):
        return (self.L.bfh_last_error(self.h) or b"").decode("utf-8", "replace")

    def fetch_counts(self):
        counts = np.zeros(max(1, self.num_items or 1), np.int64)
        return self.L.bfh_stream_fetch_counts(self.h, counts.ctypes.data_as(C.POINTER(C.c_int64)))

    def __del__(self):
        self.L.bfh_stream_destroy(self.h)


INVALID = -1
NAMES = b"apple\nmango\npie\n"


def test_unknown_token_names_the_first_one_in_file_order():
    r = Raw(NAMES)
    rc, _ = r.build(b"apple pie\nmango\napple kiwi pie\nplum\nmango fig\n")
    assert rc == INVALID and "line 3" in r.message() and "'kiwi'" in r.message(), r.message()
    assert r.fetch_counts() == INVALID                    # a failed build leaves nothing to fetch
    long_token = b"z" * 100
    rc, _ = r.build(b"apple\n" + long_token + b"\n")
    assert rc == INVALID and "line 2" in r.message() and "'" + "z" * 64 + "'" in r.message()


def test_a_proper_prefix_of_a_name_is_unknown():
    r = Raw(NAMES)
    rc, _ = r.build(b"apple\nmango app\n")
    assert rc == INVALID and "line 2" in r.message() and "'app'" in r.message()


def test_duplicate_names_are_refused():
    r = Raw(b"apple\nmango\n apple \npie\n")
    assert r.rc_vocab == INVALID and "twice" in r.message()
    rc, _ = r.build(b"apple\n")
    assert rc == INVALID and "set_vocabulary" in r.message()


def test_split_arguments_are_checked():
    r = Raw(NAMES)
    text = b"apple pie mango\npie pie\n"
    assert r.build(text, vali_n=1, pos=[0])[0] == INVALID and "exclude" in r.message()
    assert r.build(text, pos=[3, 1])[0] == INVALID and "ascending" in r.message()
    assert r.build(text, pos=[1, 1])[0] == INVALID and "ascending" in r.message()
    assert r.build(text, pos=[1, 5])[0] == INVALID and "outside" in r.message()
    assert r.build(text, pos=[-1])[0] == INVALID and "outside" in r.message()
    rc, counts = r.build(text, pos=[1, 4])
    assert rc == 0 and counts == [2, 5, 3, 3, 2]


def test_call_order_is_checked():
    r = Raw(NAMES)
    assert r.fetch_counts() == INVALID and "before" in r.message()
    fresh = Raw()
    rc, _ = fresh.build(b"apple\n")
    assert rc == INVALID and "set_vocabulary" in fresh.message()


# ---- 6. rebuild --------------------------------------------------------------------------------------------------------------------------
def test_a_second_build_is_that_of_a_fresh_handle_and_runs_repeat():
    names = sc.names_file(SPLIT_NAMES)
    first, second = split_text(), sc.random_stream(SPLIT_NAMES, 77, 9, 3)
    b = builder(names)
    b.build(first, vali_n=1)
    again = b.build(second, vali_n=2)
    want = sc.restate(names, second, 2)
    sc.assert_same(again, want, 40)
    fresh = builder(names).build(second, vali_n=2)
    once_more = b.build(second, vali_n=2)
    for f in ("events", "records", "vali"):
        for x, y in zip(getattr(fresh, f)(), getattr(once_more, f)()):
            assert x.tobytes() == y.tobytes()
    assert np.array_equal(fresh.item_counts(), once_more.item_counts())
    with pytest.raises(Exception):
        again.events()                                   # replaced by the later build
