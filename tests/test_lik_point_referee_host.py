"""CPU only: the long-double referee of csrc/lik_point.h (tests/lik_point_referee.py) before the device is held to it.

(1) against 60-digit mpmath on the whole grid: every term within 4 ulp of long double of its own size -- the value itself for
    the logistic terms and the Poisson h, which add terms of one sign; y rate'/rate + rate' for the Poisson g, whose two addends
    cancel at y = rate whatever the arithmetic; the referee's scale_ll = y (1 + |log rate|) + rate for the Poisson ll (the
    1 + : log rate is the logarithm of a rounded rate, and next to rate = 1 that rounding is all there is of it);
(2) against the reference's recorded outputs (tests/golden/mcmc_golden.npz; F15, tests/golden/poiss_golden.npz) at the tolerances
    tests/test_hmc_host.py and tests/test_poisson_model.py hold the example models to;
(3) what the inputs of tests/test_gpu_lik_point.py presume (tests/lik_point_cases.py): every "one Newton step" probe starts
    where the referee's Newton step is at most 2^-30 at a positive Newton matrix, and the referee's fit of the end-to-end case
    converges in at most half of the iterations the device is given."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lik_point_cases as cases  # noqa: E402
import lik_point_referee as ref  # noqa: E402

LD = np.longdouble
ULP = 2.0 ** -63                  # spacing of long double at 1 (64-bit significand)
DEVICE_MAX_ITER = 100             # LaplacePosteriorSampler's default, which the end-to-end GPU test leaves in place


def test_long_double_is_wider_than_double():
    assert np.finfo(LD).eps <= 2.0 ** -63, "np.longdouble is no wider than float64 here: the referee cannot referee"


def _to_mp(mp, v):
    """A long double as an mpf, exactly (also below the range of float64)."""
    m, e = np.frexp(v)
    hi = np.float64(m)
    lo = np.float64(m - LD(hi))
    return mp.ldexp(mp.mpf(float(hi)) + mp.mpf(float(lo)), int(e))


def _truth(mp, family, s, y):
    """((ll, its magnitude), (g, ..), (h, ..)) from the definitions at 60 digits."""
    s, y = mp.mpf(float(s)), mp.mpf(float(y))
    if family == "logistic":
        e = mp.exp(-s)
        ll, g, h = -mp.log1p(e), e / (1 + e), -e / (1 + e) ** 2
        return (ll, abs(ll)), (g, abs(g)), (h, abs(h))
    # (rate'' rate - rate'^2 loses 2 |s| log10(e) digits at negative s: the working precision leaves 60 behind that)
    with mp.workdps(mp.mp.dps + (int(-0.87 * float(s)) + 1 if s < 0 else 0)):
        u = mp.exp(s)
        L = mp.log1p(u)
        sig, dsig = u / (1 + u), u / (1 + u) ** 2
        ll = y * mp.log(L) - L
        g = y * sig / L - sig
        h = y * (dsig * L - sig * sig) / (L * L) - dsig
        return (ll, y * (1 + abs(mp.log(L))) + L), (g, y * sig / L + sig), (h, abs(h))


@pytest.mark.parametrize("family", ref.FAMILIES)
def test_point_terms_against_mpmath(family):
    mp = pytest.importorskip("mpmath")
    grid = cases.host_grid(family)
    assert grid.size == 8001 + len(cases.BRANCH_POINTS) + (2 if family == "logistic" else 0)
    with mp.workdps(60):
        for y in ((0.0,) if family == "logistic" else cases.Y_VALUES):
            ll, g, h = ref.point_terms(family, grid, np.full(grid.shape, y))
            worst = [0.0, 0.0, 0.0]
            for i, s in enumerate(grid):
                for k, (got, (want, mag)) in enumerate(zip((ll[i], g[i], h[i]), _truth(mp, family, s, y))):
                    assert mag > 0
                    worst[k] = max(worst[k], float(abs(_to_mp(mp, got) - want) / (mag * ULP)))
            print("%s y=%g: referee against 60 digits, ulp of long double: ll %.2f, g %.2f, h %.2f" % ((family, y) + tuple(worst)))
            assert max(worst) <= 4.0, (family, y, worst)


def test_log_factorial_against_mpmath():
    mp = pytest.importorskip("mpmath")
    ys = np.array([0, 1, 2, 3, 7, 50, 64, 65, 66, 100, 1e3, 12345, 1e6])
    got = ref.log_factorial(ys)
    assert got[0] == 0 and got[1] == 0
    with mp.workdps(60):
        for y, v in zip(ys[2:], got[2:]):
            want = mp.loggamma(mp.mpf(float(y)) + 1)
            assert abs(_to_mp(mp, v) - want) <= 4 * ULP * want, y


def test_nan_in_nan_out():
    for family in ref.FAMILIES:
        for t in ref.point_terms(family, np.array([np.nan, 1.0]), np.array([2.0, 2.0])):
            assert np.isnan(t[0]) and np.isfinite(t[1])


def test_derivatives_are_derivatives():
    """g = d ll / ds and h = d g / ds by central differences in long double (step 1e-6: truncation 1e-12, rounding 1e-13 of the
    scale) -- the formulas of the referee are those of one function."""
    s = np.concatenate((np.linspace(-40.0, 40.0, 161), [-300.0, -120.0, 90.0]))
    d = LD(1e-6)
    for family in ref.FAMILIES:
        for y in ((0.0,) if family == "logistic" else (0.0, 3.0, 50.0)):
            yv = np.full(s.shape, y)
            _, g, h = ref.point_terms(family, s, yv)
            up, dn = ref.point_terms(family, s.astype(LD) + d, yv), ref.point_terms(family, s.astype(LD) - d, yv)
            assert np.all(np.abs((up[0] - dn[0]) / (2 * d) - g) <= 1e-9 * (1 + y))
            assert np.all(np.abs((up[1] - dn[1]) / (2 * d) - h) <= 1e-9 * (1 + y))


# ------------------------------------------------------------------------------------------------ the reference's outputs
@pytest.mark.parametrize("tag,family", (("lr", "logistic"), ("poiss", "poisson")))
@pytest.mark.parametrize("wtag", ("full", "wtd"))
def test_composed_sums_equal_the_mcmc_golden(tag, family, wtag):
    gold = np.load(os.path.join(ROOT, "tests", "golden", "mcmc_golden.npz"))
    Z, th = gold[tag + "_Z"], gold[tag + "_th"]
    w = None if wtag == "full" else gold["w"]
    val, grad = ref.log_joint_grad(family, Z, w, th)
    ref_v, ref_g = gold["%s_%s_lj" % (tag, wtag)], gold["%s_%s_grad" % (tag, wtag)]
    np.testing.assert_allclose(val.astype(np.float64), ref_v, rtol=1e-12, atol=0)
    scale = np.abs(ref_g).max(axis=1, keepdims=True)
    assert np.all(np.abs(grad.astype(np.float64) - ref_g) <= 1e-12 * scale)


def test_F15_poisson_log_likelihood():
    g = np.load(os.path.join(ROOT, "tests", "golden", "poiss_golden.npz"))
    z, th = g["ll_z"], g["ll_th"]
    s = z[:, :-1].dot(th.T)
    y = z[:, -1:]
    ll, lf = ref.point_terms("poisson", s, y, with_h=False)[0], ref.log_factorial(y)
    # the fixture is a float64 evaluation of y log rate - log y! - rate: next to test_poisson_model's rtol it is allowed 4 roundings
    # of its own addends (5013 - 4219 - 800 = -5.8 at s = 800, y = 750), which a copy of its arithmetic repeats and the referee does not
    addends = (np.abs(y * np.log(np.log1p(np.exp(s.astype(LD))))) + np.log1p(np.exp(s.astype(LD))) + lf).astype(np.float64)
    assert np.all(np.abs((ll - lf).astype(np.float64) - g["ll"]) <= 1e-13 * np.abs(g["ll"]) + 4 * ref.U * addends)


@pytest.mark.parametrize("tag,family,D", (("poiss_full", "poisson", 4), ("poiss_wtd", "poisson", 4), ("lr_full", "logistic", 3), ("lr_wtd", "logistic", 3)))
def test_F15_laplace_fit(tag, family, D):
    g = np.load(os.path.join(ROOT, "tests", "golden", "poiss_golden.npz"))
    Z = g["poiss_Z"] if family == "poisson" else g["lr_Z"]
    w = g["poiss_w"] if tag.endswith("wtd") else np.ones(Z.shape[0])
    sel = w > 0
    mu, H, steps, ok = ref.laplace_fit(family, Z[sel], w[sel], np.zeros(D))
    assert ok and steps <= 50
    np.testing.assert_allclose(mu.astype(np.float64), g[tag + "_mu"], rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(ref.inverse(H).astype(np.float64), g[tag + "_cov"], rtol=2e-4, atol=1e-7)


# --------------------------------------------------------------------------------- what the GPU cases presume, on the CPU
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_h_probes_start_at_a_stationary_point(family):
    probes = cases.h_probe_cases(family)
    if family == "poisson":
        band = [s for s, _ in probes if -745 < s < -355]
        assert len(set(band)) >= 40 and len(set(s for s in band if -372.5 < s < -355)) >= 15
    worst = 0.0
    for s0, y in probes:
        c = cases.h_probe(family, s0, y)
        assert np.all(c["w"] > 0) and np.all(np.isfinite(c["Z"])) and c["Z"][0, 0] * c["t0"] == s0
        if family == "poisson" and -745 < s0 < -355 and y <= 1e3:
            assert c["w"][0] == 1.0
        H, step = cases.h_probe_start(c)
        assert H >= 1 and abs(step) <= cases.STEP_MARGIN, (s0, y, float(H), float(step))
        # the second point's curvature stays small next to the identity's 1; what it adds to the bound is below the first point's
        x2 = c["Z"][1, 0] ** 2
        h2 = ref.point_terms(family, c["Z"][1:, 0] * c["t0"], c["Z"][1:, -1])[2][0]
        assert float(c["w"][1] * abs(h2) * x2) <= 2.0 ** -9
        W, lo, hi = cases.h_probe_expected(c, c["t0"])
        assert lo <= W <= hi and np.isfinite(float(W)) and 0 < W <= 1
        worst = max(worst, abs(float(step)))
    print("%s: %d probes, the referee's largest Newton step at a start %.3g (margin %.3g)" % (family, len(probes), worst, cases.STEP_MARGIN))


def test_end_to_end_case_converges_on_the_referee():
    Z, w, th0 = cases.end_to_end_case()
    mu, H, steps, ok = ref.laplace_fit("poisson", Z, w, th0)
    print("end to end: the referee converges in %d Newton steps to %s" % (steps, mu.astype(np.float64)))
    assert ok and steps <= DEVICE_MAX_ITER // 2
    grad = ref.newton_step("poisson", Z, w, mu)[0]
    assert np.abs(grad).max() <= 1e-15
