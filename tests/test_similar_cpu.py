"""The restatement of the reference's row normalisation (tests/similar_cases.py) that the GPU tests of most_similar compare against:
it equals what the reference's own `Algo._normalize` produced (tests/golden/similar_vectors.npz, made by make_similar_vectors.py) and the
row sums of the installed numpy, bit for bit, for every d the GPU test uses."""
import os

import numpy as np
import pytest

import similar_cases as sc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "similar_vectors.npz")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_the_golden_file_covers_every_d():
    with np.load(GOLDEN) as g:
        assert tuple(g["ds"]) == sc.NORMALIZE_DS
        assert list(g["seeds"]) == [9000 + d for d in sc.NORMALIZE_DS]


@pytest.mark.parametrize("d", sc.NORMALIZE_DS)
def test_restatement_equals_the_reference_output(d):
    with np.load(GOLDEN) as g:
        want = g["Fn_%d" % d]
    got = sc.normalize(sc.golden_input(d))
    assert got.dtype == np.float32 and got.shape == want.shape == (40, d)
    assert np.array_equal(_bits(got), _bits(want))
    assert not got[3].any()                                        # the zero row stays zero: sqrt(1e-8) divides it


@pytest.mark.parametrize("d", sc.NORMALIZE_DS + (3, 32, 33, 64, 160, 192, 520, 1100))
def test_restated_sum_equals_numpy_row_sums(d):
    """(F ** 2).sum(-1) of the installed numpy on the contiguous matrix; 520 and 1100 columns: two and three halvings deep."""
    F = sc.factors(d) if d in sc.NORMALIZE_DS else sc.raw_factors(200, d, 7000 + d)
    assert np.array_equal(_bits(sc.sum_of_squares(F)), _bits((F ** 2).sum(-1)))
    assert np.array_equal(_bits(sc.normalize(F)), _bits(F / np.sqrt((F ** 2).sum(-1) + 1e-8)[..., np.newaxis]))


def test_the_traps_are_real():
    """What the restatement must not be replaced by: a sum over zero-padded columns and a float64 sum rounded at the end give other bits."""
    F = sc.factors(100)
    padded = np.zeros((sc.ROWS, 104), np.float32)
    padded[:, :100] = F
    s = sc.sum_of_squares(F)
    assert (_bits(sc.sum_of_squares(padded)) != _bits(s)).any()
    assert (_bits((F.astype(np.float64) ** 2).sum(-1).astype(np.float32)) != _bits(s)).any()


def test_planted_rows():
    F = sc.factors(20)
    Fn = sc.normalize(F)
    assert not Fn[sc.ZERO].any()
    assert np.array_equal(_bits(Fn[sc.DUP_A:sc.DUP_A + 40]), _bits(Fn[sc.DUP_B:sc.DUP_B + 40]))
    assert np.array_equal(_bits(Fn[sc.NEG]), _bits(-Fn[sc.NEG_OF]))
    assert np.allclose(Fn[sc.MULT:sc.MULT + 20], Fn[sc.MULT], rtol=1e-5, atol=1e-7)
    assert set([sc.ZERO, sc.NEG, sc.NEG_OF, sc.DUP_A, sc.DUP_B, sc.MULT]) <= set(sc.PLANTED)
