"""CPU-only: the 4-bit front pass (csrc/screen4.hip) restated in NumPy (tools/screen4_model.py).  Every row's exact fp64
score lies within e4 of its 4-bit score; the sentinel threshold never exceeds the exact maximum and never excludes the
arg-max row or a row tied with it; the model tool runs at a reduced size."""
import numpy as np
import pytest

from tools import screen4_model as m4
from tools.screen8_model import dequantise, kacc, plan, quantise


def _rows(kind, d, rs):
    if kind == "randn":
        return rs.randn(300, d)
    if kind == "dominant":                        # one element far above the rest: clipping at 0.8 max|a| is active
        X = rs.randn(50, d)
        X[np.arange(50), rs.randint(0, d, size=50)] = 40.0 * (1 + rs.rand(50))
        return X
    if kind == "constant":
        return np.outer(rs.uniform(0.5, 2.0, size=20) * rs.choice([-1.0, 1.0], size=20), np.ones(d))
    raise AssertionError(kind)


def _scaled_query(qstar):
    """The q * 2^-E convention of apply_common.h store_query: the fp32 query holds q* 2^-E, E = exponent of max|q*|."""
    _, E = np.frexp(np.abs(qstar).max())
    return np.ldexp(qstar, -int(E)), int(E)


@pytest.mark.parametrize("power", (0, 100, -100))
@pytest.mark.parametrize("kind,d", (("randn", 16), ("randn", 40), ("randn", 512), ("dominant", 40), ("dominant", 512),
                                    ("constant", 16), ("constant", 40), ("constant", 512)))
def test_every_exact_score_is_within_e4(kind, d, power):
    rs = np.random.RandomState(1000 + d + abs(power))
    X = np.ldexp(_rows(kind, d, rs), power)                  # rows scaled by 2^power; the normalised rows do not change
    Astar = X / np.sqrt((X * X).sum(axis=1))[:, None]        # exact normalised rows (fp64)
    An = Astar.astype(np.float32)                            # as stored
    for qstar in (X.sum(axis=0), np.ldexp(rs.randn(d), power), X[0] - 0.3 * X[1]):
        qsc, _ = _scaled_query(qstar)
        q32 = qsc.astype(np.float32)
        exact = Astar @ qsc                                  # the exact score in the query's scaled units
        qscale = np.float32(np.sqrt((q32.astype(np.float64) ** 2).sum()))
        codes, sc, b4 = m4.quantise4(An)
        assert codes.min() >= -7 and codes.max() <= 7
        if kind == "dominant":
            assert (np.abs(An).max(axis=1) > 7.0 * sc).all()     # the dominant element is clipped
        x, step, qerr, (l, h1, h2) = m4.quantise_query(q32)
        assert np.array_equal(256 * h2 + 16 * h1 + l, x)
        for dig in (l, h1, h2):
            assert dig.min() >= -8 and dig.max() <= 7
        eA, eB = m4.e4_coefficients(qscale, qerr, m4.err_coef_f32(d))
        s4 = m4.score4(codes, sc, x, step)
        e4 = m4.e4_of(s4, b4, eA, eB)
        gap = np.abs(s4.astype(np.float64) - exact)
        print(kind, d, power, "max |score4 - exact| / e4 = %.3f" % float((gap / e4).max()), "bound4 mean %.3f" % float(b4.mean()))
        assert (gap <= e4.astype(np.float64)).all()
        # the stored nibbles: 8 per dword, code + 8, padding 8
        pk = m4.pack4(codes)
        assert pk.shape[1] == (d + 31) // 32 * 16
        assert np.array_equal((pk[:, : d // 2] & 15).astype(np.int16) - 8, codes[:, 0:d - d % 2:2])


def _lower8(An, q32, qscale, d):
    c8, s8, b8 = quantise(An)
    G, CH = plan(d)
    s = dequantise(c8, s8, d) @ q32.astype(np.float64)
    e = ((b8.astype(np.float64) + s8.astype(np.float64) * kacc(d, G, CH)) * 1.000002 + m4.err_coef_f32(d)) * float(qscale)
    return s - e - np.abs(s) * 2e-7


@pytest.mark.parametrize("d", (16, 40, 512))
def test_sentinel_rule_never_excludes_the_winner(d):
    rs = np.random.RandomState(77 + d)
    X = rs.randn(4000, d)
    X[1234] = X[17]
    X[3999] = 2.0 * X[17]                                   # same normalised row: exact ties
    Astar = X / np.sqrt((X * X).sum(axis=1))[:, None]
    An = Astar.astype(np.float32)
    codes, sc, b4 = m4.quantise4(An)
    bins, nbins = m4.wave_of_row4(len(X), d)
    for trial in range(6):
        qstar = Astar[17] * 3.0 + 0.01 * rs.randn(d) if trial % 2 == 0 else rs.randn(d)
        qsc, _ = _scaled_query(qstar)
        q32 = qsc.astype(np.float32)
        qscale = np.float32(np.sqrt((q32.astype(np.float64) ** 2).sum()))
        exact = Astar @ qsc
        L8 = _lower8(An, q32, qscale, d)
        # sentinels as the kernel picks them from some earlier query's upper bounds, and 64 arbitrary rows
        prev = (An.astype(np.float64) @ rs.randn(d))
        for sent in (m4.pick_sentinels(prev, np.arange(len(X)), bins, nbins), rs.choice(len(X), 64, replace=False)):
            assert len(sent) <= 64
            Lg = np.float32(L8[sent].max())
            assert float(Lg) <= exact.max()
            x, step, qerr, _ = m4.quantise_query(q32)
            eA, eB = m4.e4_coefficients(qscale, qerr, m4.err_coef_f32(d))
            U4 = m4.upper4(m4.score4(codes, sc, x, step), b4, eA, eB)
            listed = ~(U4 < Lg)
            winners = np.flatnonzero(exact >= exact.max() - 1e-15 * abs(exact.max()))
            if trial % 2 == 0:
                assert {17, 1234, 3999} <= set(winners.tolist())
            assert listed[winners].all()


def test_model_tool_at_reduced_size():
    out, lines = m4.run(20000, 64, 14, 3, "randn", verbose=False)
    assert out["iterations_4bit"] == 12 and out["redos"] == 0 and not out["dropped"]
    assert 0.0 < out["listed_fraction_mean"] < 1.0
    assert all("listed_c0.7" in ln and "fullest_c1.0" in ln and "top_minus_Lg_over_q" in ln for ln in lines[1:])
    # rows of rank 100 with a segment capacity this size cannot hold: the tier drops after 4 redos, it does not thrash
    out, lines = m4.run(20000, 64, 40, 3, "lowrank", verbose=False, seg_cap=4)
    assert out["dropped"] and out["redos"] == 4
    first = next(i for i, ln in enumerate(lines) if ln["dropped"])
    assert first < 20 and all(ln["tier"] == "8-bit" for ln in lines[first + 1:])
