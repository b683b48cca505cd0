"""CPU-only: the definitions behind bc.energy_distance / bc.stein_discrepancy as tests/discrepancy_restatement.py
writes them out -- the closed form of the Stein kernel against automatic differentiation of the base kernel, the signs of both
V-statistics, that both tell a shifted sample from an exact one -- and the argument errors of the public functions that are raised
before any device call."""
import numpy as np
import pytest

import discrepancy_restatement as restate


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("D", (1, 3))
def test_closed_form_against_autograd_of_the_base_kernel(D):
    """k_p(x, y) = tr(d_x d_y k) + g_x . d_y k + g_y . d_x k + (g_x . g_y) k with k the IMQ kernel differentiated by torch in float64.
    Both sides are a few dozen float64 operations on numbers of order one: 64 u of the absolute elementary terms."""
    import torch
    rs = np.random.RandomState(10 + D)
    c = 1.3
    for _ in range(20):
        x, y, gx, gy = (rs.randn(D) for _ in range(4))
        tx = torch.tensor(x, dtype=torch.float64, requires_grad=True)
        ty = torch.tensor(y, dtype=torch.float64, requires_grad=True)
        k = (c * c + ((tx - ty) ** 2).sum()) ** -0.5
        dkx, dky = torch.autograd.grad(k, (tx, ty), create_graph=True)
        trace = sum(torch.autograd.grad(dkx[i], ty, retain_graph=True)[0][i] for i in range(D))
        want = float(trace.detach()) + gx.dot(dky.detach().numpy()) + gy.dot(dkx.detach().numpy()) + gx.dot(gy) * float(k.detach())
        for dtype in (np.float64, np.longdouble):
            kp, mag = restate.stein_terms(x, gx, y, gy, c, dtype)
            assert kp.shape == (1, 1) and abs(float(kp[0, 0]) - want) <= 64 * 2.0 ** -53 * float(mag[0, 0])
    assert float(restate.imq(np.zeros(D), np.zeros(D), c)) == pytest.approx(1 / c, rel=1e-15)
    # the diagonal: k_p(x, x) = D / c^3 + |g|^2 / c
    kp, _ = restate.stein_terms(x, gx, x, gx, c, np.longdouble)
    assert float(kp[0, 0]) == pytest.approx(D / c ** 3 + gx.dot(gx) / c, rel=1e-15)


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("dtype", (np.float64, np.longdouble))
@pytest.mark.parametrize("seed", range(4))
def test_both_v_statistics_are_non_negative(dtype, seed):
    rs = np.random.RandomState(seed)
    S, T, D = 40 + 17 * seed, 30 + 11 * seed, 1 + 2 * seed
    X, Y, G = rs.randn(S, D) * (1 + seed), rs.randn(T, D) + 0.3, 3.0 * rs.randn(S, D)
    value, m_xy, m_xx, m_yy = restate.energy_distance(X, Y, dtype)
    assert value >= 0 and m_xy > 0 and m_xx > 0 and m_yy > 0
    same = restate.energy_distance(X, X, dtype)[0]
    assert abs(same) <= 8 * np.finfo(dtype).eps * m_xx                          # (energy(X, X) = 0: the three means are one number)
    ksd2, u, mag = restate.stein_discrepancy(X, G, 1.0, dtype)
    assert ksd2 >= 0 and mag >= ksd2
    total, _, diag = restate.stein_sum(X, G, X, G, 1.0, dtype)
    assert u == (total - diag) / (dtype(S) * dtype(S - 1))
    assert np.isnan(restate.stein_discrepancy(X[:1], G[:1], 1.0, dtype)[1])


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("seed", range(1, 7))
def test_both_tell_a_shifted_sample_from_an_exact_one(seed):
    """Target N(0, I) in D = 3 (score -x), 1024 exact draws against the same draws shifted by 0.5 / sqrt(D) per coordinate; the
    energy distance is taken to a second exact sample.  Measured with this restatement over seeds 1 - 6: the shifted sample's
    ksd^2 is 16 - 28 times the exact sample's, its energy^2 23 - 38 times.  Asserted: 5 times."""
    rs = np.random.RandomState(seed)
    D, S = 3, 1024
    X, Y = rs.randn(S, D), rs.randn(S, D)
    Xs = X + 0.5 / np.sqrt(D)
    k_exact = restate.stein_discrepancy(X, -X, 1.0, np.float64)[0]
    k_shift = restate.stein_discrepancy(Xs, -Xs, 1.0, np.float64)[0]
    e_exact = restate.energy_distance(X, Y, np.float64)[0]
    e_shift = restate.energy_distance(Xs, Y, np.float64)[0]
    print("seed %d: ksd^2 %.4g -> %.4g (x %.1f), energy^2 %.4g -> %.4g (x %.1f)"
          % (seed, k_exact, k_shift, k_shift / k_exact, e_exact, e_shift, e_shift / e_exact))
    assert k_exact > 0 and e_exact > 0
    assert k_shift >= 5 * k_exact and e_shift >= 5 * e_exact


# ---------------------------------------------------------------------------------------------------------------- 4
def test_argument_errors_before_any_device_call():
    import torch
    import bayesiancoresets_amd as bc
    from bayesiancoresets_amd import discrepancy
    rs = np.random.RandomState(0)
    x, y, g = rs.randn(10, 3), rs.randn(7, 3), rs.randn(10, 3)
    for bad in (dict(x=rs.randn(5, 33), y=rs.randn(5, 33)), dict(x=x, y=rs.randn(7, 4)), dict(x=np.zeros((0, 3)), y=y),
                dict(x=x, y=np.zeros((4, 0, 3))), dict(x=rs.randn(5), y=y), dict(x=x, y=y, max_draws=0),
                dict(x=x, y=y, center=np.zeros(3))):
        with pytest.raises(ValueError):
            bc.energy_distance(**bad)
    pts = rs.randn(20, 3)
    for bad in (dict(samples=x), dict(samples=x, scores=g, family="logistic", pts=pts), dict(samples=x, scores=g, pts=pts),
                dict(samples=x, family="logistic"), dict(samples=x, family="probit", pts=pts), dict(samples=x, scores=rs.randn(10, 4)),
                dict(samples=x, scores=rs.randn(9, 3)), dict(samples=rs.randn(2, 5, 3), scores=g), dict(samples=rs.randn(4, 33), scores=rs.randn(4, 33)),
                dict(samples=np.zeros((0, 3)), scores=np.zeros((0, 3))), dict(samples=x, scores=g, c=0.0), dict(samples=x, scores=g, c=-1.0),
                dict(samples=x, scores=g, c=np.inf), dict(samples=x, scores=g, c=np.nan), dict(samples=x, scores=g, max_draws=-3)):
        with pytest.raises(ValueError):
            bc.stein_discrepancy(**bad)
    # past 2^20 draws a side: refused on the shape alone -- the input is a broadcast view of one row, nothing that size exists
    huge = np.broadcast_to(np.zeros((1, 3)), (discrepancy.MAX_DRAWS + 1, 3))
    with pytest.raises(ValueError, match="at most"):
        bc.energy_distance(huge, y)
    with pytest.raises(ValueError, match="at most"):
        bc.stein_discrepancy(huge, huge)
    if not torch.cuda.is_available():
        # ... and thinned below the limit they get as far as the device: there is no CPU fallback
        with pytest.raises(RuntimeError, match="needs a GPU"):
            bc.energy_distance(huge, y, max_draws=100)
        with pytest.raises(RuntimeError, match="needs a GPU"):
            bc.stein_discrepancy(x, g)
        with pytest.raises(RuntimeError, match="need a GPU"):
            discrepancy._pair_stat(0, x)
