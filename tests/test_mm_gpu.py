"""MatrixMarket databases built on the device (`bfh_mm_*`, buffalo_amd.ingest.MatrixMarketBuilder) against the reference's own databases
(tests/golden/data_vectors.npz, tests/golden/mm_prepro_vectors.npz) and the numpy restatement tests/test_mm_ref_cpu.py pins to them
(tests/mm_cases.py).  Every check is exact equality of bits, except ImplicitALS values: within 1 ulp of the restatement (the device's
binary64 log is within one binary64 ulp of the true value, so the rounding to binary32 can move by at most one step; equality is expected)
and within `ials_ref_ulp` + 1 of the reference's, whose float32 log is CPU-dependent."""
import ctypes as C

import numpy as np
import pytest

import mm_cases as mc
from test_mm_ref_cpu import ALL_CASES, NEW_META, check_against_golden, golden_inputs

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = -1, -3


def builder(pname=None, **kw):
    from buffalo_amd.ingest import MatrixMarketBuilder
    b = MatrixMarketBuilder()
    b.set_value_prepro(pname, **kw)
    return b


def assert_same(res, want, pname, what=""):
    """Every output of a MatrixMarketResult against the restatement: exactly, ImplicitALS values within 1 ulp.  Returns the largest ulp distance."""
    assert res.header == want["header"], (what, res.header)
    worst = 0
    pairs = [(res.group(1), want["rowwise"], "rowwise"), (res.group(2), want["colwise"], "colwise")]
    for got, exp, g in pairs:
        assert got["indptr"].dtype == np.int64 and np.array_equal(got["indptr"], exp["indptr"]), (what, g)
        assert got["key"].dtype == np.int32 and np.array_equal(got["key"], exp["key"]), (what, g)
    rows, cols, vals = res.vali()
    assert rows.dtype == cols.dtype == np.int32 and np.array_equal(rows, want["vali"][0]) and np.array_equal(cols, want["vali"][1]), what
    for got, exp, g in [(p[0]["val"], p[1]["val"], p[2]) for p in pairs] + [(vals, want["vali"][2], "vali")]:
        assert got.dtype == exp.dtype == np.float32 and got.shape == exp.shape, (what, g)
        if pname == "ImplicitALS":
            d = int(mc.ulps(got, exp).max()) if len(got) else 0
            worst = max(worst, d)
            assert d <= 1, (what, g, d)
        else:
            assert np.array_equal(got.view(np.int32), exp.view(np.int32)), (what, g)
    if pname == "MinMaxScalar":
        assert np.array_equal(res.value_range().view(np.int32), want["value_range"].view(np.int32)), (what, res.value_range(), want["value_range"])
    return worst


# ---- 1. every fixture case -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_CASES)
def test_device_builds_the_reference_database(tmp_path, name):
    text, positions, pname, kw, want, meta = golden_inputs(tmp_path, name)
    res = builder(pname, **kw).build(text, positions)
    check_against_golden(want, meta, pname, NEW_META["ials_ref_ulp"] + 1, res.header, {1: res.group(1), 2: res.group(2)}, res.vali())
    worst = assert_same(res, mc.restate(text, positions, pname, **kw), pname, name)
    print("%s: largest ulp distance to the restatement %d" % (name, worst))
    assert res.stats["samples"] == res.header["num_nnz"] and res.stats["accepted"] == res.header["num_train"]
    assert res.stats["merges"] == 0 and res.stats["kernel_ms"] > 0


def test_a_path_is_read_like_its_bytes(tmp_path):
    text, positions, _, _, _, _ = golden_inputs(tmp_path, "none_seed3_crlf")
    path = tmp_path / "main.mtx"
    path.write_bytes(text)
    assert_same(builder().build(str(path), positions), mc.restate(text, positions), None)


# ---- 2. lines across tile ends -------------------------------------------------------------------------------------------------------------
TILE_TEXT = mc.align_to_tile(mc.tile_text())
TILE_FORMS = {"lf": TILE_TEXT, "crlf": mc.as_crlf(TILE_TEXT), "lone_cr": mc.as_lone_cr(TILE_TEXT)}


@pytest.mark.parametrize("form,prepro", [("lf", p) for p in sorted(mc.PREPROS)] + [("crlf", "none"), ("lone_cr", "none")])
def test_lines_across_tile_ends_equal_the_restatement(form, prepro):
    text = TILE_FORMS[form].encode()
    assert len(text) > 9 * 4096
    positions, exact = mc.tile_positions(text)
    nnz = mc.header(mc.lines_of(text))[2]
    assert {0, 1, nnz - 2} <= set(positions.tolist()) and set(range(100, 105)) <= set(positions.tolist())
    if form == "lf":
        assert exact >= 1                                    # a line ends exactly at a 4,096-byte boundary, the next one starts there
    pname, kw = mc.PREPROS[prepro]
    res = builder(pname, **kw).build(text, positions)
    worst = assert_same(res, mc.restate(text, positions, pname, **kw), pname, (form, prepro))
    print("tile case %s %s: largest ulp distance to the restatement %d" % (form, prepro, worst))
    assert res.stats["merges"] == 0


# ---- 3. one parse and two sorts against the shipped path --------------------------------------------------------------------------------------
def test_groups_equal_text_to_csr_on_the_working_text():
    from buffalo_amd.ingest import text_to_csr
    text = TILE_TEXT.encode()
    positions, _ = mc.tile_positions(text)
    want = mc.restate(text, positions)
    res = builder().build(text, positions)
    h = res.header
    for sort_key, num_major, num_minor in ((1, h["num_users"], h["num_items"]), (2, h["num_items"], h["num_users"])):
        got, exp = res.group(sort_key), text_to_csr(want["working_text"], h["num_train"], num_major, num_minor, sort_key)
        for k in ("indptr", "key", "val"):
            assert got[k].dtype == exp[k].dtype and got[k].tobytes() == exp[k].tobytes(), (sort_key, k)


# ---- 4. values of the held-out triples in file order -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("prepro", sorted(mc.PREPROS))
def test_vali_file_order_mode(prepro):
    text = TILE_TEXT.encode()
    positions, _ = mc.tile_positions(text)
    pname, kw = mc.PREPROS[prepro]
    b = builder(pname, **kw)
    b.set_mode("vali_file_order", 1)
    assert_same(b.build(text, positions), mc.restate(text, positions, pname, vali_file_order=True, **kw), pname)
    plain = mc.restate(text, positions)
    assert not np.array_equal(plain["vali"][2], mc.restate(text, positions, vali_file_order=True)["vali"][2])    # the two orders differ here
    b.set_mode("vali_file_order", 0)
    assert_same(b.build(text, positions), mc.restate(text, positions, pname, **kw), pname)


# ---- 5. refusals: a status and a message, never a fault ----------------------------------------------------------------------------------------
class Raw:
    """The C ABI without the wrapper: status codes and messages as they are."""

    def __init__(self):
        from buffalo_amd._lib import lib
        self.L = lib()
        self.h = self.L.bfh_mm_create()
        assert self.h

    def build(self, text, pos=None):
        out = (C.c_int64 * 6)()
        arr = None if pos is None else np.ascontiguousarray(pos, dtype=np.int64)
        ptr = None if arr is None else arr.ctypes.data_as(C.POINTER(C.c_int64))
        return self.L.bfh_mm_build(self.h, text, len(text), ptr, 0 if arr is None else len(arr), out), list(out)

    def prepro(self, name, a=0.0, b=0.0):
        return self.L.bfh_mm_set_value_prepro(self.h, name, a, b)

    def message(self):
        return (self.L.bfh_last_error(self.h) or b"").decode("utf-8", "replace")

    def fetch_vali(self, n=64):
        r, c, v = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float32)
        return self.L.bfh_mm_fetch_vali(self.h, r.ctypes.data_as(C.POINTER(C.c_int32)), c.ctypes.data_as(C.POINTER(C.c_int32)),
                                        v.ctypes.data_as(C.POINTER(C.c_float)))

    def fetch_range(self):
        out = np.zeros(4, np.float32)
        return self.L.bfh_mm_fetch_value_range(self.h, out.ctypes.data_as(C.POINTER(C.c_float)))

    def __del__(self):
        self.L.bfh_mm_destroy(self.h)


def base_text():
    import make_data_vectors as mk
    return mk._mm_text(60, 40, 0.2, 1, real=True)


def test_positions_are_checked():
    r, text = Raw(), base_text().encode()
    nnz = mc.header(mc.lines_of(text))[2]
    assert r.build(text, [7, 3])[0] == INVALID and "ascending" in r.message()
    assert r.build(text, [5, 5])[0] == INVALID and "ascending" in r.message()
    assert r.build(text, [-1])[0] == INVALID and "outside" in r.message()
    assert r.build(text, [3, nnz])[0] == INVALID and "outside" in r.message()
    assert r.build(text, [nnz - 1])[0] == INVALID and "outside" in r.message()          # the last line is never held out
    assert r.fetch_vali() == INVALID                                                   # a failed build leaves nothing to fetch
    rc, counts = r.build(text, [0, nnz - 2])
    assert rc == 0 and counts == [60, 40, nnz, 3, nnz - 2, 2]


def test_a_held_out_pair_listed_twice_is_refused_with_its_lines():
    r, text = Raw(), base_text().encode()
    lines = mc.lines_of(text)
    assert lines[3 + 53].split()[:2] == lines[3 + 64].split()[:2]
    assert r.build(text, [53, 64])[0] == INVALID
    assert "57" in r.message() and "68" in r.message() and "same (row, col)" in r.message(), r.message()     # 1-based file lines: 3 header lines
    assert r.build(text, [10, 53, 70])[0] == 0                                          # one of the two alone is fine


def test_file_shape_is_checked():
    r, text = Raw(), base_text()
    body_end = text.rindex("\n", 0, len(text) - 1) + 1
    nnz = mc.header(mc.lines_of(text.encode()))[2]
    assert r.build(text[:body_end].encode())[0] == INVALID
    assert "line %d" % (nnz + 2) in r.message() and "%d body lines" % (nnz - 1) in r.message(), r.message()
    lines = text.split("\n")
    for bad in ("7 x 1.5", "7 8", "", "7 8 abc"):
        broken = "\n".join(lines[:10] + [bad] + lines[11:]).encode()
        assert r.build(broken, [2])[0] == INVALID and "line 11 " in r.message(), (bad, r.message())
    assert r.build((" % indented\n" + text).encode())[0] == INVALID and "line 1 " in r.message()
    assert r.build(b"%%MatrixMarket\n% only comments\n")[0] == INVALID and "size line" in r.message()
    assert r.build(b"%%MatrixMarket\n3 4\n1 1 1\n")[0] == INVALID and "line 2 " in r.message()
    outside = "\n".join(lines[:10] + ["61 1 1.0"] + lines[11:]).encode()
    assert r.build(outside)[0] == INVALID and "outside the matrix" in r.message()


def test_prepro_names_and_arguments_are_checked():
    r, text = Raw(), base_text().encode()
    assert r.prepro(b"SPPMI") == UNSUPPORTED and "SPPMI" in r.message()
    assert r.prepro(b"Standardize") == UNSUPPORTED and "Standardize" in r.message()
    assert r.prepro(b"ImplicitALS", 0.0) == INVALID and r.prepro(b"ImplicitALS", -0.5) == INVALID and "epsilon" in r.message()
    assert r.prepro(None) == 0 and r.prepro(b"") == 0 and r.prepro(b"OneBased") == 0 and r.prepro(b"ImplicitALS", 0.5) == 0
    assert r.build(text)[0] == 0
    assert r.fetch_range() == INVALID and "MinMaxScalar" in r.message()
    assert r.prepro(b"MinMaxScalar", 1.0, 5.0) == 0
    assert r.fetch_range() == INVALID                                                   # the build before it had no range
    assert r.build(text)[0] == 0 and r.fetch_range() == 0
    bad = base_text().split("\n")
    bad[10] = "7 8 inf"
    assert r.build("\n".join(bad).encode())[0] == INVALID and "finite" in r.message()


def test_a_fetch_before_a_build_is_refused():
    r = Raw()
    assert r.fetch_vali() == INVALID and "before" in r.message()
    assert r.fetch_range() == INVALID
    assert r.L.bfh_mm_set_mode(r.h, b"no_such_mode", 1) == INVALID


# ---- 6. rebuild ----------------------------------------------------------------------------------------------------------------------------
def test_a_second_build_is_that_of_a_fresh_handle_and_runs_repeat():
    first, second = TILE_TEXT.encode(), base_text().encode()
    p1, _ = mc.tile_positions(first)
    p2 = np.array([4, 9, 200], np.int64)
    b = builder("MinMaxScalar", min=1, max=5)
    stale = b.build(first, p1)
    again = b.build(second, p2)
    want = mc.restate(second, p2, "MinMaxScalar", min=1, max=5)
    assert_same(again, want, "MinMaxScalar")
    fresh = builder("MinMaxScalar", min=1, max=5).build(second, p2)
    more = b.build(second + b"1 1 9.5\n2 2 0.001\n", p2)                                 # more body lines than the size line says: nothing changes
    for x, y in zip((fresh.group(1), fresh.group(2)), (more.group(1), more.group(2))):
        assert all(x[k].tobytes() == y[k].tobytes() for k in ("indptr", "key", "val"))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(fresh.vali(), more.vali()))
    assert fresh.value_range().tobytes() == more.value_range().tobytes() and more.header == fresh.header
    with pytest.raises(Exception):
        stale.group(1)                                                                  # replaced by the later builds
    with pytest.raises(Exception):
        again.vali()


# ---- 7. on to the evaluator ------------------------------------------------------------------------------------------------------------------
def test_the_result_feeds_the_evaluator():
    from buffalo_amd.evaluate import Evaluator
    text = TILE_TEXT.encode()
    positions, _ = mc.tile_positions(text)
    b = builder()
    b.set_mode("vali_file_order", 1)
    res = b.build(text, positions)
    g, (rows, cols, vals) = res.group(1), res.vali()
    ev = Evaluator()
    ev.set_data(res.header["num_users"], res.header["num_items"], g["indptr"], g["key"], rows, cols, vals)
    assert ev.num_rows() == len(np.unique(rows))
