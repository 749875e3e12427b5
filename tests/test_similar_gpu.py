"""`most_similar` / `normalize` (bfh_topk_normalize[_device], bfh_topk_most_similar[_device|_vectors], buffalo_amd.parallel): cosine top-k
that leaves the factors unnormalised.  The call is defined by the old ones, so every comparison is exact (key values and score bits):

* `normalize` against the numpy restatement of the reference's `Algo._normalize` (tests/similar_cases.py, itself held to the reference's
  output and to numpy by tests/test_similar_cpu.py), host and device form, out of place and in place;
* `most_similar(F)` against `dot_topn(indexes, Fn, Fn)` on the dense and on the fused path, `most_similar_device` against `most_similar`,
  `most_similar_vectors(V, F)` against `dot_topn(arange, V, Fn)`;
* the caller's matrix keeps its bytes, the model stays usable, and the refusals carry a message and launch nothing."""
import functools

import numpy as np
import pytest

import similar_cases as sc
import topk_cases as tc

pytestmark = pytest.mark.gpu

FMIN = np.finfo(np.float32).tiny
PATHS = (("dense", 0, 0), ("fused", 1, 0), ("fused32", 1, 32))     # name, "fused", "fused_c0"


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _engine(fused=0, c0=0, flt=1):
    from buffalo_amd import parallel as par
    eng = par.TopK()
    eng.set_mode("fused", fused)
    eng.set_mode("fused_c0", c0)
    eng.set_mode("flt_min_rule", flt)
    return eng


@functools.lru_cache(maxsize=None)
def restated(d):
    """Fn of the case builder's matrix, computed once per d and shared (read-only)."""
    Fn = np.ascontiguousarray(sc.normalize(sc.factors(d)))
    Fn.setflags(write=False)
    return Fn


@functools.lru_cache(maxsize=None)
def queries():
    """A shuffled subset of the rows with repeats that holds every planted row, and a pool of 150 shuffled ids."""
    rng = np.random.default_rng(42)
    idx = np.concatenate([sc.PLANTED, rng.choice(sc.ROWS, size=120, replace=False), sc.PLANTED[:5], rng.integers(0, sc.ROWS, size=30)])
    idx = np.ascontiguousarray(rng.permutation(idx), dtype=np.int32)
    pool = np.ascontiguousarray(rng.permutation(sc.ROWS)[:150], dtype=np.int32)
    return idx, pool


def _out(n, k):
    return np.full((n, k), 12345, dtype=np.int32), np.full((n, k), 9.75, dtype=np.float32)


def _similar(eng, indexes, F, pool, k):
    keys, scores = _out(len(indexes), k)
    eng.most_similar(indexes, F, keys, scores, pool, k)
    return keys, scores


def _dot(eng, indexes, P, Q, pool, k):
    keys, scores = _out(len(indexes), k)
    eng.dot_topn(indexes, P, Q, tc.NO_BIAS, keys, scores, pool, k)
    return keys, scores


def _same(got, want, what):
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(_bits(got[1]), _bits(want[1])), what


def _device(a, ld, fill=0.0):
    """The host matrix a [rows, d] as a torch tensor [rows, ld] in HBM, its pad columns = `fill`."""
    import torch
    padded = np.full((a.shape[0], ld), fill, dtype=np.float32)
    padded[:, :a.shape[1]] = a
    return torch.from_numpy(padded).cuda()


@pytest.mark.parametrize("d", sc.NORMALIZE_DS)
def test_normalize_has_the_bits_of_the_restatement(d):
    """d < 8, the remainder loop, one and two halvings, every d % 8 / d % 32 situation; device form: out of place and in place, pad
    columns (garbage on the way in: they are not part of the sum) zero on the way out."""
    import torch
    from buffalo_amd import parallel as par
    F, want = sc.factors(d), restated(d)
    before = F.tobytes()
    got = _engine().normalize(F)
    assert got.dtype == np.float32 and got.shape == F.shape
    bad = np.flatnonzero((_bits(got) != _bits(want)).any(axis=1))
    print("d = %d: %d of %d rows differ from the restatement" % (d, len(bad), sc.ROWS))
    assert len(bad) == 0, bad[:10]
    assert F.tobytes() == before
    if d == 20:
        assert np.array_equal(_bits(par.normalize(F)), _bits(want))            # the module-level function
    ld = (d + 7) // 8 * 8 + (8 if d % 16 == 4 else 0)                          # d = 20, 100: a pitch beyond the next multiple of 8 too
    dF = _device(F, ld, fill=7.5)
    dOut = torch.full((sc.ROWS, ld), -3.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    _engine().normalize_device(dF.data_ptr(), sc.ROWS, d, ld, dOut.data_ptr())
    out = dOut.cpu().numpy()
    assert np.array_equal(_bits(out[:, :d]), _bits(want)) and not _bits(out[:, d:]).any()
    assert np.array_equal(dF.cpu().numpy()[:, :d], F) and (dF.cpu().numpy()[:, d:] == 7.5).all()      # the source is not written
    _engine().normalize_device(dF.data_ptr(), sc.ROWS, d, ld)                  # in place
    out = dF.cpu().numpy()
    assert np.array_equal(_bits(out[:, :d]), _bits(want)) and not _bits(out[:, d:]).any()


@pytest.mark.parametrize("pooled", [False, True])
@pytest.mark.parametrize("k", [1, 10, 700])
@pytest.mark.parametrize("d", [20, 100, 128, 200])
def test_most_similar_equals_dot_topn_over_the_normalised_rows(d, k, pooled):
    """Row b = the dot_topn row of indexes[b] with P = Q = Fn (self-excluded), under the same modes: the dense path everywhere, the fused
    path (the rule's sample, a one-tile sample) at d <= 128.  k = 700 > rows: padding.  F keeps its bytes."""
    F, Fn = sc.factors(d), restated(d)
    idx, pool = queries()
    pl = pool if pooled else tc.EMPTY_POOL
    before = F.tobytes()
    dense = None
    for name, fused, c0 in PATHS:
        if fused and d > 128:
            continue
        eng = _engine(fused, c0)
        got = _similar(eng, idx, F, pl, k)
        _same(got, _dot(eng, idx, Fn, Fn, pl, k), name)
        dense = dense or got
        _same(got, dense, name + " against dense")
    assert F.tobytes() == before
    keys, scores = dense
    kk = min(k, len(pl) if pooled else sc.ROWS)
    for b, q in enumerate(idx):
        assert q not in keys[b] and sc.ZERO not in keys[b]                     # never itself; the zero row scores 0 <= FLT_MIN
        if q == sc.ZERO:                                                       # as a query it gets only padding
            assert (keys[b] == -1).all() and (scores[b, :kk] == FMIN).all() and not _bits(scores[b, kk:]).any()
        if q == sc.NEG:
            assert sc.NEG_OF not in keys[b]                                    # cosine -1
        if not pooled and sc.DUP_A <= q < sc.DUP_A + 40:
            assert keys[b, 0] == q + sc.DUP_B - sc.DUP_A                       # its exact duplicate comes first
        if not pooled and k == 10 and sc.MULT <= q < sc.MULT + 20:
            assert ((keys[b] >= sc.MULT) & (keys[b] < sc.MULT + 20)).all()     # its positive multiples: cosine 1 up to rounding


def test_most_similar_without_the_flt_min_rule():
    """flt_min_rule = 0: every score is admissible, so k = 700 lists all 599 other rows, the zero row and the negative cosines included."""
    d, k = 20, 700
    F, Fn = sc.factors(d), restated(d)
    idx, _ = queries()
    eng = _engine(0, 0, 0)
    got = _similar(eng, idx, F, tc.EMPTY_POOL, k)
    _same(got, _dot(eng, idx, Fn, Fn, tc.EMPTY_POOL, k), "flt_min_rule = 0")
    assert (got[0][:, :sc.ROWS - 1] >= 0).all() and (got[0][:, sc.ROWS - 1:] == -1).all()
    b = int(np.flatnonzero(idx == sc.NEG)[0])
    assert got[0][b, sc.ROWS - 2] == sc.NEG_OF                                 # the last listed row: minus the query


@pytest.mark.parametrize("d,ld,fused", [(20, 32, 0), (20, 32, 1), (100, 104, 1), (128, 128, 1), (200, 200, 0)])
def test_device_form_equals_the_host_form(d, ld, fused):
    """most_similar_device from a matrix in HBM == most_similar of the same rows; the device matrix reads back unchanged."""
    F = sc.factors(d)
    idx, pool = queries()
    eng = _engine(fused)
    dF = _device(F, ld)
    import torch
    torch.cuda.synchronize()
    for pl, k in ((tc.EMPTY_POOL, 10), (pool, 40)):
        keys, scores = _out(len(idx), k)
        eng.most_similar_device(idx, dF.data_ptr(), sc.ROWS, d, ld, keys, scores, pl, k)
        _same((keys, scores), _similar(eng, idx, F, pl, k), (d, ld, fused, k))
    back = dF.cpu().numpy()
    assert np.array_equal(_bits(back[:, :d]), _bits(F)) and not _bits(back[:, d:]).any()


@pytest.mark.parametrize("d", [20, 100, 200])
def test_query_vectors_equal_dot_topn_of_the_vectors(d):
    """V = rows of Fn, raw rows of F and a zero vector, scored as given against Fn: row b = the dot_topn row of query b with P = V, Q = Fn.
    No self-exclusion: a query equal to a row lists that row (first: nothing else has cosine 1 with the rows chosen here)."""
    F, Fn = sc.factors(d), restated(d)
    own = [3, 77, 410, 599]
    V = np.ascontiguousarray(np.concatenate([Fn[own], F[[8, 250, sc.MULT + 1]], np.zeros((1, d), np.float32)]))
    _, pool = queries()
    arange = np.arange(len(V), dtype=np.int32)
    before = F.tobytes()
    for fused in (0, 1) if d <= 128 else (0,):
        eng = _engine(fused)
        for pl, k in ((tc.EMPTY_POOL, 10), (pool, 200)):
            keys, scores = _out(len(V), k)
            eng.most_similar_vectors(V, F, keys, scores, pl, k)
            _same((keys, scores), _dot(eng, arange, V, Fn, pl, k), (d, fused, k))
            if not len(pl):
                assert list(keys[:len(own), 0]) == own
                assert (keys[-1] == -1).all()                                  # the zero vector scores 0 everywhere
    assert F.tobytes() == before


def test_the_model_is_still_usable():
    """After most_similar on Q and on P, dot_topn(users, P, Q) on the same arrays gives what it gave before."""
    from buffalo_amd import parallel as par
    rng = np.random.default_rng(12)
    P = rng.normal(scale=0.3, size=(200, 24)).astype(np.float32)
    Q = sc.raw_factors(sc.ROWS, 24, 77)
    users = np.ascontiguousarray(rng.permutation(200)[:90], dtype=np.int32)
    p0, q0 = P.tobytes(), Q.tobytes()
    want = tc.run(par.dot_topn, users, P, Q, tc.NO_BIAS, tc.EMPTY_POOL, 10)
    items = np.arange(sc.ROWS, dtype=np.int32)
    keys, scores = _out(sc.ROWS, 10)
    par.most_similar(items, Q, keys, scores, tc.EMPTY_POOL, 10)
    _same((keys, scores), _dot(_engine(), items, *(2 * [np.ascontiguousarray(sc.normalize(Q))]), tc.EMPTY_POOL, 10), "module-level most_similar")
    keys, scores = _out(90, 10)
    par.most_similar(users, P, keys, scores, tc.EMPTY_POOL, 10)
    assert P.tobytes() == p0 and Q.tobytes() == q0
    _same(tc.run(par.dot_topn, users, P, Q, tc.NO_BIAS, tc.EMPTY_POOL, 10), want, "dot_topn after most_similar")


def test_refusals_carry_their_own_message_and_launch_nothing():
    from buffalo_amd import parallel as par
    from buffalo_amd._lib import BuffaloHipError
    F = sc.factors(20)
    idx = np.arange(5, dtype=np.int32)
    eng = par.TopK()
    for outside in (-1, sc.ROWS):
        with pytest.raises(BuffaloHipError, match="index outside"):
            _similar(eng, np.array([0, outside], np.int32), F, tc.EMPTY_POOL, 10)
        with pytest.raises(BuffaloHipError, match="pool id outside"):
            _similar(eng, idx, F, np.array([3, outside], np.int32), 10)
        with pytest.raises(BuffaloHipError, match="pool id outside"):
            k, s = _out(2, 10)
            eng.most_similar_vectors(np.ascontiguousarray(F[:2]), F, k, s, np.array([3, outside], np.int32), 10)
    for k in (0, 16385):
        with pytest.raises(BuffaloHipError, match="k must be in"):
            _similar(eng, idx, F, tc.EMPTY_POOL, k)
    with pytest.raises(BuffaloHipError, match="at least one row and one column"):
        _similar(eng, idx[:0], np.empty((0, 20), np.float32), tc.EMPTY_POOL, 10)
    with pytest.raises(BuffaloHipError, match="at least one row and one column"):
        eng.normalize(np.empty((4, 0), np.float32))
    with pytest.raises(BuffaloHipError, match="leading dimension"):
        eng.most_similar_device(idx, 4096, sc.ROWS, 20, 20, *_out(5, 10), tc.EMPTY_POOL, 10)      # refused before the address is used
    with pytest.raises(ValueError, match="out_keys / out_scores"):
        eng.most_similar(idx, F, *_out(5, 9), tc.EMPTY_POOL, 10)
    with pytest.raises(ValueError, match="out_keys / out_scores"):
        eng.most_similar(idx, F, *_out(4, 10), tc.EMPTY_POOL, 10)
    with pytest.raises(ValueError, match="same number of columns"):
        eng.most_similar_vectors(np.zeros((2, 19), np.float32), F, *_out(2, 10), tc.EMPTY_POOL, 10)
    st = eng.stats()
    assert st["samples"] == 0 and st["h2d_bytes"] == 0 and st["aux_ms"] == 0 and st["kernel_ms"] == 0      # nothing was uploaded or launched
    keys, _ = _similar(eng, idx, F, tc.EMPTY_POOL, 10)                         # the handle survives
    assert (keys >= 0).all() and eng.stats()["aux_ms"] > 0                     # the normalise kernel counts into aux_ms
