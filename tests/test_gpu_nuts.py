"""GPU: the NUTS transition of bc.DeviceHMC(kernel="nuts") (csrc/nuts.hip) against (1) the recursive NumPy
statement (tests/nuts_restatement.py), teacher-forced over every transition, (2) the depth cap and the smallest shapes, (3) ground
truths no sampler produced (the prior; a tensor-grid quadrature), (4) failures that stick, (5) reproducibility, limits and the
untouched default.

The depth counts completed doublings, so a transition of depth d took at least 2^d - 1 leapfrog steps; one that a turn of a
proper sub-span cut short inside doubling d shows 2^d - 1 < n_leapfrog < 2^(d+1) - 1 without a divergence -- that is what (1)
looks for to know the span tests were exercised."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bayesian-coresets_amd", "examples", "common"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import nuts_restatement as nr  # noqa: E402
from test_gpu_hmc import _case, _moment_z, _quadrature, _tolerances  # noqa: E402

pytestmark = pytest.mark.gpu
CLOSE = 1e-9
QUANTITIES = ("xi", "alpha", "eps", "dsel")


@pytest.fixture(scope="module")
def bc():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import bayesiancoresets_amd as bc
    return bc


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "mcmc_golden.npz"))


def _teacher_forced(family, pts, wts, D, J, res, fixed=None):
    """Every transition of the device run restarted from the device's previous state and base step in the recursive statement,
    in long double (the referee) and in float64.  Returns per quantity the device's and the float64 statement's largest deviation
    from the referee in units of the quantity's scale, the transitions whose depth / leapfrog count / divergence disagree with the
    referee, and those too close to call (left out of both)."""
    tr = res.trace
    tl = nr.Target(family, pts, wts, D, res.center, res.transform, np.longdouble)
    td = nr.Target(family, pts, wts, D, res.center, res.transform, np.float64)
    dg = tr["diag"]
    C, T = dg.shape[:2]
    nw, eps0 = res.n_warmup, tr["step0"]
    dev, f64 = dict.fromkeys(QUANTITIES, 0.0), dict.fromkeys(QUANTITIES, 0.0)
    wrong = close = 0
    for c in range(C):
        for t in range(T):
            xi = tr["xi"][c, t - 1] if t else np.zeros(D)
            base, hbar, lebar = dg[c, t - 1, 3:6] if t else (eps0 if fixed is None else fixed, 0.0, 0.0)
            z = tr["noise"][c, t]
            rl, rd = nr.transition_recursive(tl, xi, z, base, J), nr.transition_recursive(td, xi, z, base, J)
            assert np.array_equal(tr["proposal"][c, t], tr["xi"][c, t])              # (the proposal is the selected state)
            if fixed is not None or t >= nw:
                assert dg[c, t, 3] == base
            if rl["margin"] < CLOSE:
                close += 1
                continue
            got = (int(dg[c, t, 1]), int(dg[c, t, 2]), bool(dg[c, t, 6] > 0.5))
            if got != (rl["depth"], rl["n_leapfrog"], rl["divergent"]):
                wrong += 1
                continue
            assert (rd["depth"], rd["n_leapfrog"], rd["divergent"]) == got
            sx = max(1.0, float(np.abs(rl["state"]).max()))
            sh = max(1.0, float(abs(rl["H0"])))
            pairs = {"xi": (np.abs(tr["xi"][c, t] - rl["state"]).max() / sx, np.abs(rd["state"] - rl["state"]).max() / sx),
                     "alpha": (abs(dg[c, t, 0] - rl["alpha"]), abs(rd["alpha"] - rl["alpha"])),
                     "dsel": (abs(dg[c, t, 7] - rl["dsel"]) / sh, abs(rd["dsel"] - rl["dsel"]) / sh)}
            if fixed is None and t < nw:
                nl = nr.dual_average_alpha(t + 1, rl["alpha"], hbar, lebar, eps0, t + 1 == nw, np.longdouble)[0]
                nd = nr.dual_average_alpha(t + 1, rd["alpha"], hbar, lebar, eps0, t + 1 == nw, np.float64)[0]
                pairs["eps"] = (abs(dg[c, t, 3] - nl) / nl, abs(nd - nl) / nl)
            for q, (a, b) in pairs.items():
                dev[q], f64[q] = max(dev[q], float(a)), max(f64[q], float(b))
    return dev, f64, wrong, close, C * T


def _hold(what, dev, f64, wrong, close, total):
    tol = _tolerances(f64)
    for q in QUANTITIES:
        print("%s %s: device %.3g, float64 statement %.3g (ratio %.2f), tolerance %.3g" % (what, q, dev[q], f64[q], dev[q] / max(f64[q], 1e-300), tol[q]))
    print("%s: %d transitions, %d disagree, %d too close to call" % (what, total, wrong, close))
    assert wrong == 0
    assert close <= 0.01 * total
    for q in QUANTITIES:
        assert dev[q] <= tol[q], (q, dev[q], tol[q])


# ---------------------------------------------------------------------------------------------------------------- 1
# Observed on an MI355X: see DESIGN.md 4.14.
@pytest.mark.parametrize("family", ("logistic", "poisson"))
def test_transitions_equal_restatement(bc, gold, family):
    pts, wts, D = _case(gold, family)
    J = 6
    res = bc.DeviceHMC(family, D, chains=32, seed=2024, kernel="nuts", max_depth=J).sample(pts, wts, 50, 50, keep_trace=True)
    assert not res.streamed and res.kernel == "nuts"
    dg = res.trace["diag"]
    assert dg.shape == (32, 100, 8) and res.trace["noise"].shape == (32, 100, nr.noise_columns(D, J))
    _hold(family, *_teacher_forced(family, pts, wts, D, J, res))
    depth, leaps, div = dg[:, :, 1].astype(int), dg[:, :, 2].astype(int), dg[:, :, 6] > 0.5
    print("%s: depth histogram %s, mean leapfrogs %.2f, divergent %d, step %.3f" % (family, np.bincount(depth.ravel(), minlength=J + 1).tolist(), leaps.mean(), div.sum(), res.step_size.mean()))
    assert (depth == 1).any() and (depth == 2).any() and (depth >= 3).any()
    cut_short = ~div & (leaps > (1 << depth) - 1) & (leaps < (1 << (depth + 1)) - 1)
    assert cut_short.any()                                      # (a turn of a proper sub-span stopped a tree: the span tests ran)
    assert (leaps >= (1 << depth) - 1).all()
    # the result's fields are the sampling transitions of the diagnostics
    assert np.array_equal(res.tree_depth, depth[:, 50:]) and np.array_equal(res.n_leapfrog, leaps[:, 50:]) and np.array_equal(res.divergent, div[:, 50:])
    assert np.array_equal(res.accept_stat, dg[:, 50:, 0]) and np.array_equal(res.delta_h, dg[:, 50:, 7])
    np.testing.assert_allclose(res.accept_rate, dg[:, 50:, 0].mean(axis=1), rtol=1e-12)
    moved = (res.trace["xi"][:, 50:] != res.trace["xi"][:, 49:-1]).any(axis=2)
    assert np.array_equal(res.accepted, moved)


# ---------------------------------------------------------------------------------------------------------------- 2
def _small(name):
    rs = np.random.RandomState(41)
    family, D, k = {"case": ("logistic", 5, 40), "wide": ("logistic", 32, 3), "one": ("poisson", 1, 1), "prior": ("logistic", 3, 0)}[name]
    if k == 0:
        pts = wts = None
    elif family == "poisson":
        pts, wts = np.hstack((rs.randn(k, D), rs.poisson(2.0, (k, 1)).astype(np.float64))), rs.uniform(0.5, 4.0, k)
    else:
        pts, wts = rs.randn(k, D) / np.sqrt(D), rs.uniform(0.5, 4.0, k)
    return family, pts, wts, D, 0.1 * rs.randn(D), np.eye(D) + 0.1 * rs.randn(D, D) / np.sqrt(D)


@pytest.mark.parametrize("name,J", (("case", 2), ("wide", 2), ("wide", 3), ("one", 2), ("prior", 2)))
def test_depth_cap_and_smallest_shapes(bc, name, J):
    family, pts, wts, D, mu, Wm = _small(name)
    hmc = bc.DeviceHMC(family, D, chains=8, seed=3, kernel="nuts", max_depth=J)
    assert hmc.ld == D + D % 2
    res = hmc.sample(pts, wts, 6, 6, center=mu, transform=Wm, keep_trace=True, _dev_step_size=1e-3)
    dg = res.trace["diag"]
    assert (dg[:, :, 1] == J).all() and (dg[:, :, 2] == (1 << J) - 1).all() and not (dg[:, :, 6] > 0.5).any()
    assert np.all(res.step_size == 1e-3)
    _hold("%s J=%d" % (name, J), *_teacher_forced(family, pts, wts, D, J, res, fixed=1e-3))


# ---------------------------------------------------------------------------------------------------------------- 3
# Largest |z| observed on an MI355X with these seeds: see DESIGN.md 4.14.
def test_stationary_law_prior(bc):
    D = 4
    res = bc.DeviceHMC("logistic", D, chains=256, seed=31, kernel="nuts", max_depth=6).sample(None, None, 1000, 1000, center=np.zeros(D), transform=np.eye(D))
    assert res.samples.shape == (256, 1000, D)
    z = _moment_z(res.samples, np.zeros(D), np.eye(D))
    print("prior: largest |z| %.2f, rhat max %.4f, mean depth %.2f, mean leapfrogs %.2f, accept statistic %.3f, step %.3f, divergent %d"
          % (np.abs(z).max(), res.rhat.max(), res.tree_depth.mean(), res.n_leapfrog.mean(), res.accept_rate.mean(), res.step_size.mean(), res.divergent.sum()))
    assert z.size == 14 and np.abs(z).max() <= 5.0, z
    assert res.rhat.max() <= 1.01


def test_stationary_law_logistic_quadrature(bc):
    import model_lr
    rs = np.random.RandomState(29)
    k = 25
    X = np.hstack((rs.randn(k, 1), np.ones((k, 1))))
    yv = np.where(rs.rand(k) < 1 / (1 + np.exp(-X.dot(np.array([1.2, -0.4])))), 1.0, -1.0)
    pts, w = yv[:, None] * X, rs.uniform(5.0, 60.0, k)
    mean, cov = _quadrature(model_lr, pts, w)
    res = bc.DeviceHMC("logistic", 2, chains=256, seed=37, kernel="nuts", max_depth=6).sample(pts, w, 1000, 1000)
    z = _moment_z(res.samples, mean, cov)
    print("logistic D=2: largest |z| %.2f, rhat max %.4f, mean depth %.2f, mean leapfrogs %.2f, accept statistic %.3f, step %.3f, divergent %d"
          % (np.abs(z).max(), res.rhat.max(), res.tree_depth.mean(), res.n_leapfrog.mean(), res.accept_rate.mean(), res.step_size.mean(), res.divergent.sum()))
    assert z.size == 5 and np.abs(z).max() <= 5.0, z
    assert res.rhat.max() <= 1.01


# ---------------------------------------------------------------------------------------------------------------- 4
def test_failures_stick(bc, gold):
    from bayesiancoresets_amd import _native
    pts, wts, D = _case(gold, "logistic")
    bad = wts.copy()
    bad[3] = np.nan
    hmc = bc.DeviceHMC("logistic", D, chains=8, seed=1, kernel="nuts", max_depth=6)
    with pytest.raises(_native.EngineError):
        hmc.sample(pts, bad, 10)
    with pytest.raises(_native.EngineError):
        hmc.sample(pts, bad, 10, center=np.zeros(D), transform=np.eye(D))
    res = hmc.sample(pts, wts, 20, 0, center=np.zeros(D), transform=np.eye(D), _dev_step_size=1e6)
    assert res.divergent.all() and (res.tree_depth == 0).all() and (res.n_leapfrog == 1).all()
    assert np.all(res.accept_rate == 0.0) and not res.accepted.any()
    assert np.all(np.isfinite(res.samples)) and np.all(res.samples == 0.0)


# ---------------------------------------------------------------------------------------------------------------- 5
def test_reproducible_limits_and_default_untouched(bc, gold):
    from bayesiancoresets_amd import _native
    lib = _native.load()
    pts, wts, D = _case(gold, "poisson")
    kw = dict(chains=16, kernel="nuts", max_depth=6)
    a = bc.DeviceHMC("poisson", D, seed=9, **kw).sample(pts, wts, 50)
    b = bc.DeviceHMC("poisson", D, seed=9, **kw).sample(pts, wts, 50)
    c = bc.DeviceHMC("poisson", D, seed=10, **kw).sample(pts, wts, 50)
    assert np.array_equal(a.samples, b.samples) and np.array_equal(a.delta_h, b.delta_h) and np.array_equal(a.n_leapfrog, b.n_leapfrog)
    assert not np.array_equal(a.samples, c.samples)
    assert lib.bcx_nuts_coreset_ok(40, 5) and not lib.bcx_nuts_coreset_ok(10, 33)
    assert lib.bcx_nuts_coreset_lds_bytes(40, 5) == 40 * 9 * 8 and lib.bcx_nuts_coreset_lds_bytes(10, 33) == -1
    big = np.repeat(pts, 400, axis=0)                          # 24 000 points of 4 parameters: past any workgroup's LDS
    with pytest.raises(ValueError, match="hmc"):
        bc.DeviceHMC("poisson", D, seed=9, **kw).sample(big, np.repeat(wts, 400), 5, 5, center=np.zeros(D), transform=np.eye(D))
    with pytest.raises(ValueError, match="hmc"):
        bc.DeviceHMC("poisson", D, seed=9, **kw).sample(pts, wts, 5, 5, _dev_force_stream=True)
    with pytest.raises(ValueError, match="max_depth"):          # 64 x 20000 x (4 + 30 + 2046) doubles: past 2 GiB
        bc.DeviceHMC("poisson", D, chains=64, seed=9, kernel="nuts", max_depth=10).sample(pts, wts, 10000)
    d0 = bc.DeviceHMC("poisson", D, chains=16, seed=9).sample(pts, wts, 50)
    d1 = bc.DeviceHMC("poisson", D, chains=16, seed=9, kernel="hmc").sample(pts, wts, 50)
    assert d0.kernel == "hmc" and np.array_equal(d0.samples, d1.samples) and np.array_equal(d0.delta_h, d1.delta_h)
