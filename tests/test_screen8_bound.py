"""The 8-bit screening tier's quantiser and per-row bound (csrc/screen8.hip), restated in NumPy (tools/screen8_model.py) and
held to exactly computed scores: for every row, |exact score of the stored row - exact score of the dequantised row| must not
exceed bound * |q|, with both scores and |q| computed without rounding that matters (rational arithmetic over the doubles).
The rows are chosen to stress the quantiser: elements spanning 16 decades, constant rows, one-hot rows, denormals, rows whose
length is not a multiple of 16."""
import math
from fractions import Fraction

import numpy as np
import pytest

from tools.screen8_model import dequantise, kacc, plan, quantise


def _exact_dot(a, q):
    """sum a_j q_j for fp64 inputs, rounded once: every double is a dyadic rational."""
    return float(sum(Fraction(float(x)) * Fraction(float(y)) for x, y in zip(a, q)))


def _exact_norm(q):
    return math.sqrt(float(sum(Fraction(float(x)) ** 2 for x in q)))


def _stress_rows(d, rs):
    rows = []
    rows.append(rs.randn(d))                                               # ordinary
    rows.append(10.0 ** rs.uniform(-16, 0, size=d) * rs.choice([-1, 1], d))  # 16 decades
    rows.append(np.full(d, 0.37))                                          # constant
    rows.append(-np.full(d, 1.0))
    e = np.zeros(d); e[d // 2] = 1.0
    rows.append(e)                                                          # one-hot
    e = np.zeros(d); e[0] = -1.0
    rows.append(e)
    rows.append(rs.randn(d) * 1e-42)                                       # fp32 denormals only
    mix = rs.randn(d); mix[::3] = 1e-44                                    # denormals next to ordinary values
    rows.append(mix)
    half = rs.randn(d); half[: d // 2] *= 1e-6
    rows.append(half)
    rows.append((np.arange(d, dtype=np.float64) % 5 - 2.0) * 0.5)          # many elements on the quantiser's rounding ties
    out = []
    for r in rows:
        n = np.linalg.norm(r)
        # the engine stores normalised rows; the row of denormals stays as it is
        out.append((r / n if n > 1e-30 else r).astype(np.float32))
    return np.array(out, dtype=np.float32)


@pytest.mark.parametrize("d", (1, 5, 16, 17, 100, 300, 512))
def test_bound_encloses_the_exact_score_difference(d):
    rs = np.random.RandomState(100 + d)
    An = _stress_rows(d, rs)
    codes, sc, bound = quantise(An)
    assert codes.shape == (len(An), (d + 15) // 16 * 16)
    assert (codes[:, d:] == 128).all() and codes[:, :d].min() >= 1
    deq = dequantise(codes, sc, d)
    queries = [rs.randn(d), np.ones(d), 10.0 ** rs.uniform(-12, 3, size=d), -An[0].astype(np.float64)]
    for i in range(len(An)):
        a = An[i].astype(np.float64)
        # the residual norm itself, exactly
        res = math.sqrt(float(sum((Fraction(float(x)) - Fraction(float(y))) ** 2 for x, y in zip(a, deq[i]))))
        assert float(bound[i]) >= res, (d, i, float(bound[i]), res)
        assert float(bound[i]) <= res * (1 + 3e-6) + 2e-45, (d, i)            # ... and not loose: the bound IS the residual
        for q in queries:
            diff = abs(_exact_dot(a, q) - _exact_dot(deq[i], q))
            assert diff <= float(bound[i]) * _exact_norm(q), (d, i, diff, float(bound[i]))


def test_codes_are_the_nearest_levels_and_the_extreme_element_is_full_scale():
    rs = np.random.RandomState(7)
    An = rs.randn(64, 96).astype(np.float32)
    An /= np.linalg.norm(An, axis=1)[:, None].astype(np.float32)
    codes, sc, bound = quantise(An)
    c = codes[:, :96].astype(np.int64) - 128
    assert np.abs(c).max(axis=1).tolist() == [127] * 64
    # nearest level: the residual of every element is at most half a step
    r = np.abs(An.astype(np.float64) - c * sc.astype(np.float64)[:, None])
    assert (r <= 0.5 * sc.astype(np.float64)[:, None] * (1 + 1e-12)).all()
    # uniformly spread residuals: bound ~ step * sqrt(d / 12)
    assert np.all(bound < sc * math.sqrt(96 / 12.0) * 1.5)


def test_zero_and_tiny_rows_keep_a_usable_scale():
    An = np.zeros((3, 20), dtype=np.float32)
    An[1, 3] = 1e-45                      # smallest fp32 denormal
    An[2, :] = 1.2e-38
    codes, sc, bound = quantise(An)
    assert (sc >= np.float32(1.17549435e-38)).all()
    assert (codes[0] == 128).all() and bound[0] == 0
    deq = dequantise(codes, sc, 20)
    for i in range(3):
        res = math.sqrt(float(((An[i].astype(np.float64) - deq[i]) ** 2).sum()))
        assert float(bound[i]) >= res


def test_accumulation_term_is_small_against_the_quantisation_bound():
    """kacc (the fp32 summation term of the screen kernel) at the flagship's row length is far below the residual norm."""
    d = 512
    G, CH = plan(d)
    assert (G, CH) == (32, 1)
    rs = np.random.RandomState(3)
    An = rs.randn(200, d)
    An = (An / np.linalg.norm(An, axis=1)[:, None]).astype(np.float32)
    codes, sc, bound = quantise(An)
    assert float((sc * kacc(d, G, CH)).max()) < 0.01 * float(bound.min())
