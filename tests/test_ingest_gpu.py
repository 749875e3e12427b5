"""Device-side COO -> CSR (bfh_coo_to_csr) vs the oracle's restatement of fileio.hpp:263-420: integer work,
so everything is compared bit for bit -- incl. duplicates (stable order), empty rows and both orientations."""
import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in ("indptr", "key", "val"))


@pytest.mark.parametrize("n,R,C", [(1, 1, 1), (7, 3, 1000), (5000, 70, 40), (200000, 138493, 27278), (99999, 5, 3)])
def test_matches_oracle_bit_for_bit(oracle, n, R, C):
    from buffalo_amd.ingest import coo_to_csr
    rng = np.random.default_rng(n)
    r = rng.integers(0, R, n).astype(np.int32)
    c = rng.integers(0, C, n).astype(np.int32)
    v = rng.permutation(n).astype(np.float32)      # distinct: any reordering of duplicates shows
    for major, minor, nm, nn in ((r, c, R, C), (c, r, C, R)):
        assert _same(coo_to_csr(major, minor, v, nm, nn), oracle.coo_to_csr(major, minor, v, nm, nn))


def test_empty_and_invalid_inputs(oracle):
    from buffalo_amd._lib import BuffaloHipError
    from buffalo_amd.ingest import coo_to_csr
    e = np.array([], np.int32)
    g = coo_to_csr(e, e, np.array([], np.float32), 4, 9)
    assert np.array_equal(g["indptr"], np.zeros(4, np.int64)) and g["key"].shape == (0,)
    with pytest.raises(BuffaloHipError):
        coo_to_csr(np.array([0, 4], np.int32), np.array([0, 0], np.int32), np.ones(2, np.float32), 4, 9)
    with pytest.raises(BuffaloHipError):
        coo_to_csr(np.array([0, 1], np.int32), np.array([0, -1], np.int32), np.ones(2, np.float32), 4, 9)


def test_empty_major_ids_in_front_between_and_behind():
    """Rows 0-1, 3-4 and 6-7 of an 8 x 4 matrix are empty: the END offsets of the ids in front of the first record's (the branch
    of the END-offset rule that only the first record takes), between the two rows and behind the last.  Through bfh_coo_to_csr
    and, as the columns of the transposed text, through bfh_text_to_csr's orient step in front of the same kernels."""
    from buffalo_amd.ingest import coo_to_csr, text_to_csr
    major, minor = np.array([2, 5, 2, 5], np.int32), np.array([1, 0, 0, 3], np.int32)
    vals = np.array([10.0, 20.0, 30.0, 40.0], np.float32)
    text = "".join("%d %d %g\n" % (b + 1, a + 1, v) for a, b, v in zip(major, minor, vals)).encode()
    for g in (coo_to_csr(major, minor, vals, 8, 4), text_to_csr(text, 4, 8, 4, 2)):
        assert g["indptr"].tolist() == [0, 0, 2, 2, 2, 4, 4, 4]
        assert g["key"].tolist() == [0, 1, 0, 3]
        assert g["val"].tolist() == [30.0, 10.0, 20.0, 40.0]


def test_loaders_build_their_groups_on_the_device(tmp_path, oracle):
    """The MatrixMarket loader checks of tests/test_front_cpu.py, with the real device path underneath."""
    import scipy.io
    from buffalo_front.data import MatrixMarketOptions, load
    M = sp.random(40, 30, density=0.2, format="coo", random_state=3)
    M.data[:] = np.random.default_rng(0).integers(1, 5, size=M.nnz)
    scipy.io.mmwrite(str(tmp_path / "main.mtx"), M)
    opt = MatrixMarketOptions().get_default_option()
    opt.input.main = str(tmp_path / "main.mtx")
    opt.data.validation = {}
    d = load(opt)
    d.create()
    rw, cw = d.get_group("rowwise"), d.get_group("colwise")
    csr, csc = M.tocsr(), M.tocsc()
    csr.sort_indices(), csc.sort_indices()
    assert np.array_equal(rw["indptr"], csr.indptr[1:]) and np.array_equal(rw["key"], csr.indices) and np.allclose(rw["val"], csr.data)
    assert np.array_equal(cw["indptr"], csc.indptr[1:]) and np.array_equal(cw["key"], csc.indices)


def test_full_size_properties():
    """ML-20M-sized: 20,000,263 records in random order -> both orientations; sortedness, END offsets,
    and an order-independent checksum tying every (row, col, val) of the output to the input."""
    from buffalo_amd import synth
    from buffalo_amd.ingest import coo_to_csr
    csr = synth.generate(*synth.SHAPES["ml20m"], seed=7)
    U, I, nnz = csr.num_users, csr.num_items, csr.nnz
    rows = np.repeat(np.arange(U, dtype=np.int32), np.diff(np.concatenate([[0], csr.indptr])))
    perm = np.random.default_rng(1).permutation(nnz)
    r, c = rows[perm], csr.keys[perm]
    v = (perm % 1000).astype(np.float32)
    g, st = coo_to_csr(r, c, v, U, I, with_stats=True)
    assert np.array_equal(g["indptr"], csr.indptr) and np.array_equal(g["key"], csr.keys)     # the generator's CSR is (row, col)-sorted and duplicate-free
    inv = np.empty(nnz, np.int64)
    inv[perm] = np.arange(nnz)
    assert np.array_equal(g["val"], v[inv])                    # every value travelled with its record
    gt = coo_to_csr(c, r, v, I, U)
    assert gt["indptr"][-1] == nnz and np.all(np.diff(gt["indptr"]) >= 0)
    t = csr.transpose()
    assert np.array_equal(gt["indptr"], t.indptr) and np.array_equal(gt["key"], t.keys)
    assert st["samples"] == nnz and st["kernel_ms"] > 0
    print("ingest 20M records: device %.2f ms (pack + radix sort + unpack)" % st["kernel_ms"])


@pytest.mark.parametrize("seed,n", [(1, 1), (2, 401), (3, 1000), (4, 50000)])
def test_text_parse_is_sscanf_bit_for_bit(oracle, seed, n):
    """bfh_parse_triples vs the oracle's restatement of fileio.hpp:280-310 (pinned by the reference's compiled fileio.hpp on the same files,
    tests/test_oracle_ref_fileio.py): ids equal, values equal as BITS -- every decimal shape a rating file holds, and the ones the device
    hands back to sscanf (near-ties of the float rounding, > 19 digits, out-of-range exponents, inf / nan / hex floats); the count of
    handed-back lines is reported and stays a small share."""
    import text_cases
    from buffalo_amd.ingest import parse_triples
    rng = np.random.default_rng(seed)
    text, lines = text_cases.make_text(rng, n, num_rows=5000, num_cols=7000)
    (r, c, v), st = parse_triples(text, lines, with_stats=True)
    ro, co, vo = oracle.parse_triples(text, lines)
    np.testing.assert_array_equal(r, ro)
    np.testing.assert_array_equal(c, co)
    np.testing.assert_array_equal(v.view(np.uint32), vo.view(np.uint32))
    assert st["samples"] == lines
    if n >= 1000:
        assert 0 < st["merges"] < 0.5 * lines       # the specials, near-ties and 17-digit reprs of text_cases went the host way (a third of ITS lines), the ordinary values did not
    # fewer lines asked for than the file holds: the first ones (fileio.hpp:312-320); more: an error (its assert)
    if n > 10:
        r2, c2, v2 = parse_triples(text, lines - 7)
        np.testing.assert_array_equal(r2, ro[:-7])
        np.testing.assert_array_equal(v2.view(np.uint32), vo[:-7].view(np.uint32))
    from buffalo_amd._lib import BuffaloHipError
    with pytest.raises(BuffaloHipError, match="lines"):
        parse_triples(text, lines + 1)


def test_plain_rating_file_needs_no_host_help(oracle):
    """An ordinary MatrixMarket body (integer and half-star ratings, six-digit decimals): every line is parsed on the device."""
    from buffalo_amd.ingest import parse_triples
    rng = np.random.default_rng(9)
    n = 200000
    rows, cols = rng.integers(1, 138494, n), rng.integers(1, 27279, n)
    kinds = rng.integers(0, 3, n)
    toks = np.where(kinds == 0, (rng.integers(1, 11, n) * 0.5).astype(str), np.where(kinds == 1, rng.integers(1, 6, n).astype(str), np.char.mod("%.6f", rng.random(n) * 5)))
    text = ("\n".join("%d %d %s" % t for t in zip(rows, cols, toks)) + "\n").encode()
    (r, c, v), st = parse_triples(text, n, with_stats=True)
    ro, co, vo = oracle.parse_triples(text, n)
    assert st["merges"] == 0
    np.testing.assert_array_equal(r, ro)
    np.testing.assert_array_equal(c, co)
    np.testing.assert_array_equal(v.view(np.uint32), vo.view(np.uint32))


def test_a_file_of_nothing_but_handed_back_lines_keeps_its_order(oracle):
    """Every value carries more than 19 significant digits, so EVERY line is handed back to sscanf while the list of flagged lines still holds them
    all: the list is in the order of the flagging atomics, not of the file, and the re-parsed values have to land on their own lines (round 5
    copied them back in list order: ADVICE r05).  Ids distinct per line so that a permutation cannot hide."""
    from buffalo_amd.ingest import parse_triples
    rng = np.random.default_rng(21)
    n = 30000                                   # > one block of the parse kernel, < the list's capacity
    rows, cols = np.arange(1, n + 1), rng.integers(1, 7000, n)
    text = ("\n".join("%d %d %.25f" % (r_, c_, x) for r_, c_, x in zip(rows, cols, rng.random(n) * 5)) + "\n").encode()
    (r, c, v), st = parse_triples(text, n, with_stats=True)
    ro, co, vo = oracle.parse_triples(text, n)
    assert st["merges"] == n
    np.testing.assert_array_equal(r, ro)
    np.testing.assert_array_equal(c, co)
    np.testing.assert_array_equal(v.view(np.uint32), vo.view(np.uint32))


@pytest.mark.parametrize("sort_key", [1, 2])
def test_text_to_csr_matches_the_reference_builder(oracle, sort_key, tmp_path):
    """bfh_text_to_csr = fileio.hpp:263-420 end to end (parse -> stable sort -> END offsets -> 0-based minors): against the reference's own
    compiled builder on the same file where oracle/_ref travelled with the snapshot, and against the oracle (parse + coo_to_csr) always."""
    import text_cases
    from buffalo_amd.ingest import text_to_csr
    from oracle import ref_fileio as rf
    rng = np.random.default_rng(17 + sort_key)
    R, C_ = 300, 170
    text, lines = text_cases.make_text(rng, 20000, num_rows=R, num_cols=C_)
    nm, nn = (R, C_) if sort_key == 1 else (C_, R)
    g, st = text_to_csr(text, lines, nm, nn, sort_key, with_stats=True)
    ro, co, vo = oracle.parse_triples(text, lines)
    major, minor = (ro - 1, co - 1) if sort_key == 1 else (co - 1, ro - 1)
    want = oracle.coo_to_csr(major, minor, vo, nm, nn)
    assert np.array_equal(g["indptr"], want["indptr"]) and np.array_equal(g["key"], want["key"])
    np.testing.assert_array_equal(g["val"].view(np.uint32), want["val"].view(np.uint32))
    if rf.available():
        src = tmp_path / "w.txt"
        src.write_bytes(text)
        d = tmp_path / "out"
        d.mkdir()
        workers = 4
        assert rf.lib().ref_sort_and_compressed_binarization(str(src).encode(), str(d).encode(), lines, nm, sort_key, workers) == workers + 1
        rec = np.dtype([("i", "<i4"), ("v", "<f4")])
        data = np.concatenate([np.fromfile(str(d / ("chunk%d.bin" % i)), dtype=rec) for i in range(workers)])
        np.testing.assert_array_equal(np.fromfile(str(d / "indptr.bin"), dtype=np.int64), g["indptr"])
        np.testing.assert_array_equal(data["i"], g["key"])
        np.testing.assert_array_equal(data["v"].view(np.uint32), g["val"].view(np.uint32))
    from buffalo_amd._lib import BuffaloHipError
    with pytest.raises(BuffaloHipError, match="outside the matrix"):
        text_to_csr(text, lines, nm - 1 if sort_key == 1 else nm, nn - 1 if sort_key == 2 else nn, sort_key)
