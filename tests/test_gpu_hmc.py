"""GPU: the device HMC (csrc/hmc.hip, bc.DeviceHMC, bc.log_joint_grad) against (1) the reference's log joint (golden),
(2) the replicated data set -- the check the reference left as a TODO (examples/common/mcmc.py:71-119), (3) the NumPy
restatement of the transition, teacher-forced over every transition of 64 chains, on both paths, (4) ground truths no sampler
produced (the prior; a tensor-grid quadrature), (5) the Laplace mode at large weights, (6) failures that stick, (7) limits."""
import os
import sys

import numpy as np
import pytest
from scipy.special import gammaln

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bayesian-coresets_amd", "examples", "common"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import hmc_restatement as hr  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -53


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


def _model(family):
    import model_lr
    import model_poiss
    return model_lr if family == "logistic" else model_poiss


def _bounds(family, Z, w, th):
    """Per output of the log joint / its gradient: 4 n 2^-53 sum_j |w_j t_j| over the n terms actually added (the points' and
    the prior's); the caller adds 8 ulp of the value compared."""
    Z, th = np.atleast_2d(Z), np.atleast_2d(th)
    D = th.shape[1]
    X = Z[:, :D]
    y = Z[:, D] if family == "poisson" else np.zeros(Z.shape[0])
    s = X.dot(th.T)
    ll, g = hr.point_terms(family, s, y[:, None])
    if family == "poisson":
        ll = ll - gammaln(y + 1.0)[:, None]
    n = Z.shape[0] + D + 1
    bv = (np.abs(w[:, None] * ll).sum(axis=0) + 0.5 * (th ** 2).sum(axis=1) + 0.5 * D * np.log(2 * np.pi)) * 4 * n * EPS
    bg = (np.einsum("jc,jd->cd", np.abs(w[:, None] * g), np.abs(X)) + np.abs(th)) * 4 * n * EPS
    return bv, bg


def _check_ljg(family, Z, w, th, val, grad, ref_val, ref_grad, what):
    bv, bg = _bounds(family, Z, w, th)
    ev = np.abs(val - ref_val) - 8 * np.spacing(np.abs(ref_val))
    eg = np.abs(grad - ref_grad) - 8 * np.spacing(np.abs(ref_grad))
    print("%s: value error / bound %.3g, gradient error / bound %.3g" % (what, (ev / bv).max(), (eg / bg).max()))
    assert np.all(ev <= bv), (what, (ev / bv).max())
    assert np.all(eg <= bg), (what, (eg / bg).max())


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("tag,family", (("lr", "logistic"), ("poiss", "poisson")))
@pytest.mark.parametrize("wtag", ("full", "wtd"))
def test_log_joint_grad_equals_golden(bc, gold, tag, family, wtag):
    Z, th = gold[tag + "_Z"], gold[tag + "_th"]               # N = 900: no multiple of the kernel's 128-row tile
    w = None if wtag == "full" else gold["w"]                  # (None: the NULL weight pointer)
    wh = np.ones(Z.shape[0]) if w is None else w
    ref_v, ref_g = gold["%s_%s_lj" % (tag, wtag)], gold["%s_%s_grad" % (tag, wtag)]
    v7, g7 = bc.log_joint_grad(family, Z, w, th)
    _check_ljg(family, Z, wh, th, v7, g7, ref_v, ref_g, "%s %s C=7" % (tag, wtag))
    v1, g1 = bc.log_joint_grad(family, Z, w, th[2])
    _check_ljg(family, Z, wh, th[2:3], v1, g1, ref_v[2:3], ref_g[2:3], "%s %s C=1" % (tag, wtag))
    v7b, g7b = bc.log_joint_grad(family, Z, w, th)
    assert np.array_equal(v7, v7b) and np.array_equal(g7, g7b)


@pytest.mark.parametrize("tag,family", (("lr", "logistic"), ("poiss", "poisson")))
def test_log_joint_grad_many_columns_equals_host_model(bc, gold, tag, family):
    Z, w = gold[tag + "_Z"], gold["w"]
    D = gold[tag + "_th"].shape[1]
    th = 0.6 * np.random.RandomState(8).randn(10000, D)
    mod = _model(family)
    v, g = bc.log_joint_grad(family, Z, w, th)
    _check_ljg(family, Z, w, th, v, g, mod.log_joint(Z, th, w), mod.grad_th_log_joint(Z, th, w), "%s C=10000" % tag)
    v2, g2 = bc.log_joint_grad(family, Z, w, th)
    assert np.array_equal(v, v2) and np.array_equal(g, g2)
    # no rows at all: the prior
    v0, g0 = bc.log_joint_grad(family, None, None, th[:5])
    np.testing.assert_allclose(v0, -0.5 * D * np.log(2 * np.pi) - 0.5 * (th[:5] ** 2).sum(axis=1), rtol=1e-14)
    np.testing.assert_array_equal(g0, -th[:5])


# ------------------------------------------------------------------------------------------- the teacher-forced comparison
def _teacher_forced(family, pts, wts, D, L, res, chains=None, transitions=None):
    """Every transition of the device run restarted from the device's previous state and step in the restatement, in long
    double (the referee) and in float64.  Returns per quantity the device's and the float64 restatement's largest deviation
    from the referee in units of the quantity's scale, and the accept decisions that disagree / are too close to call."""
    tr = res.trace
    mu, Wm = res.center, res.transform
    tl = hr.Target(family, pts, wts, D, mu, Wm, np.longdouble)
    td = hr.Target(family, pts, wts, D, mu, Wm, np.float64)
    C, T = tr["diag"].shape[:2]
    nw, eps0 = res.n_warmup, tr["step0"]
    dev = dict(proposal=0.0, dH=0.0, eps=0.0)
    f64 = dict(proposal=0.0, dH=0.0, eps=0.0)
    wrong, close = 0, 0
    for c in (range(C) if chains is None else chains):
        for t in (range(T) if transitions is None else transitions):
            xi = tr["xi"][c, t - 1] if t else np.zeros(D)
            base, hbar, lebar = (tr["diag"][c, t - 1, 3:6] if t else (eps0, 0.0, 0.0))
            z = tr["noise"][c, t]
            rl, rd = hr.transition(tl, xi, z, base, L), hr.transition(td, xi, z, base, L)
            sp = max(1.0, float(np.abs(rl["proposal"]).max()))
            sh = max(1.0, float(abs(rl["H0"])), float(abs(rl["H1"])))
            dev["proposal"] = max(dev["proposal"], float(np.abs(tr["proposal"][c, t] - rl["proposal"]).max()) / sp)
            f64["proposal"] = max(f64["proposal"], float(np.abs(rd["proposal"] - rl["proposal"]).max()) / sp)
            dev["dH"] = max(dev["dH"], float(abs(tr["diag"][c, t, 0] - rl["dH"])) / sh)
            f64["dH"] = max(f64["dH"], float(abs(rd["dH"] - rl["dH"])) / sh)
            assert float(abs(tr["diag"][c, t, 2] - rl["eps_t"])) <= 32 * EPS * float(rl["eps_t"])      # (the jittered step: one exp)
            if t < nw:
                nl = hr.dual_average(t + 1, rl["dH"], hbar, lebar, eps0, t + 1 == nw, np.longdouble)[0]
                nd = hr.dual_average(t + 1, rd["dH"], hbar, lebar, eps0, t + 1 == nw, np.float64)[0]
                dev["eps"] = max(dev["eps"], float(abs(tr["diag"][c, t, 3] - nl) / nl))
                f64["eps"] = max(f64["eps"], float(abs(nd - nl) / nl))
            else:
                assert tr["diag"][c, t, 3] == base
            if abs(float(rl["dH"] - rl["e"])) > 1e-9 * max(1.0, float(rl["e"])):
                wrong += bool(tr["diag"][c, t, 1] > 0.5) != rl["accepted"]
            else:
                close += 1
            # the state the device went on from is the proposal or the previous state, as it decided
            want = tr["proposal"][c, t] if tr["diag"][c, t, 1] > 0.5 else xi
            assert np.array_equal(tr["xi"][c, t], want)
    return dev, f64, wrong, close


def _tolerances(f64):
    """16 x the float64 restatement's own deviation from the long-double one, per quantity, at least 32 ulp of the scale."""
    return {q: max(16.0 * f64[q], 32 * 2.0 ** -52) for q in f64}


def _case(gold, family):
    rs = np.random.RandomState(17)
    if family == "logistic":
        k, D = 40, 5
        X = np.hstack((rs.randn(k, D - 1), np.ones((k, 1))))
        yv = np.where(rs.rand(k) < 1 / (1 + np.exp(-X.dot(np.array([1.0, -0.5, 0.5, 0.2, 0.1])))), 1.0, -1.0)
        pts = yv[:, None] * X
    else:
        k, D = 60, 4
        pts = gold["poiss_Z"][rs.choice(900, k, replace=False)]
    return pts, rs.uniform(0.5, 8.0, k), D


_RUNS = {}


def _run(bc, gold, family, streamed):
    key = (family, streamed)
    if key not in _RUNS:
        pts, wts, D = _case(gold, family)
        hmc = bc.DeviceHMC(family, D, chains=64, leapfrog=8, seed=2024)
        _RUNS[key] = (pts, wts, D, hmc.sample(pts, wts, 100, 100, keep_trace=True, _dev_force_stream=streamed))
    return _RUNS[key]


# ---------------------------------------------------------------------------------------------------------------- 3
# Observed on an MI355X (device deviation / float64 restatement's deviation, largest over the four runs): see DESIGN.md 4.12.
@pytest.mark.parametrize("family", ("logistic", "poisson"))
@pytest.mark.parametrize("streamed", (False, True))
def test_transitions_equal_restatement(bc, gold, family, streamed):
    pts, wts, D, res = _run(bc, gold, family, streamed)
    assert res.streamed == streamed
    assert res.trace["diag"].shape[:2] == (64, 200)
    dev, f64, wrong, close = _teacher_forced(family, pts, wts, D, 8, res)
    tol = _tolerances(f64)
    for q in ("proposal", "dH", "eps"):
        print("%s %s %s: device %.3g, float64 restatement %.3g (ratio %.2f), tolerance %.3g"
              % (family, "streamed" if streamed else "coreset", q, dev[q], f64[q], dev[q] / max(f64[q], 1e-300), tol[q]))
    for q in ("proposal", "dH", "eps"):
        assert dev[q] <= tol[q], (q, dev[q], tol[q])
    assert wrong == 0
    assert close <= 1
    acc = res.trace["diag"][:, :, 1].mean()
    assert 0.5 < acc < 0.99, acc                               # (both outcomes occur: the decisions above were exercised)


@pytest.mark.parametrize("family", ("logistic", "poisson"))
def test_paths_agree_at_first_transition(bc, gold, family):
    pts, wts, D, a = _run(bc, gold, family, False)
    _, _, _, b = _run(bc, gold, family, True)
    assert np.array_equal(a.trace["noise"], b.trace["noise"])
    _, f64, _, _ = _teacher_forced(family, pts, wts, D, 8, a, transitions=(0,))
    tol = _tolerances(f64)["proposal"]
    for name in ("proposal", "theta"):
        x, y = a.trace[name][:, 0], b.trace[name][:, 0]
        err = np.abs(x - y).max() / max(1.0, np.abs(x).max())
        print("%s %s at transition 1: coreset vs streamed %.3g (tolerance %.3g)" % (family, name, err, tol))
        assert err <= tol


# ---------------------------------------------------------------------------------------------------------------- 2
def test_integer_weights_equal_replication(bc, gold):
    rs = np.random.RandomState(23)
    for family, tag in (("logistic", "lr"), ("poisson", "poiss")):
        Zall = gold[tag + "_Z"]
        D = gold[tag + "_th"].shape[1]
        k = 30
        pts = Zall[rs.choice(900, k, replace=False)]
        w = rs.randint(1, 10, k).astype(np.float64)
        rep = np.repeat(pts, w.astype(int), axis=0)
        th = 0.5 * rs.randn(6, D)
        v, g = bc.log_joint_grad(family, pts, w, th)
        vr, gr = bc.log_joint_grad(family, rep, None, th)
        _check_ljg(family, rep, np.ones(rep.shape[0]), th, v, g, vr, gr, "%s weighted vs replicated" % tag)
        mu, cov = _model(family).laplace_fit(pts, w)
        Wm = np.linalg.cholesky(cov).T
        out = []
        for p, ww in ((pts, w), (rep, None)):
            hmc = bc.DeviceHMC(family, D, chains=64, leapfrog=8, seed=77)
            out.append(hmc.sample(p, ww, 1, 1, center=mu, transform=Wm, keep_trace=True))
            assert not out[-1].streamed
        assert np.array_equal(out[0].trace["noise"], out[1].trace["noise"])
        dev_w, f64, _, _ = _teacher_forced(family, pts, w, D, 8, out[0], transitions=(0,))
        dev_r, _, _, _ = _teacher_forced(family, pts, w, D, 8, out[1], transitions=(0,))      # (the replicated run against the WEIGHTED referee)
        tol = _tolerances(f64)
        print("%s first proposal: weighted %.3g, replicated %.3g, tolerance %.3g" % (tag, dev_w["proposal"], dev_r["proposal"], tol["proposal"]))
        for d in (dev_w, dev_r):
            assert d["proposal"] <= tol["proposal"] and d["dH"] <= tol["dH"]


# ---------------------------------------------------------------------------------------------------------------- 4
def _moment_z(samples, mean, cov):
    """z-scores of the pooled mean and covariance entries against the truth; standard errors from the spread of the per-chain
    estimates (second moments about the TRUE mean: unbiased per chain)."""
    C, T, D = samples.shape
    d = samples - mean
    m_c = samples.mean(axis=1)
    s_c = np.einsum("cti,ctj->cij", d, d) / T
    iu = np.triu_indices(D)
    est = np.concatenate((m_c.mean(axis=0), s_c.mean(axis=0)[iu]))
    se = np.concatenate((m_c.std(axis=0, ddof=1), s_c.std(axis=0, ddof=1)[iu])) / np.sqrt(C)
    return (est - np.concatenate((mean, cov[iu]))) / se


def _quadrature(mod, pts, w):
    """Mean and covariance of the D = 2 posterior by the trapezoid rule on a tensor grid over +-10 Laplace standard deviations
    (in the whitened coordinates), refined until neither changes by 1e-8."""
    mu, cov = mod.laplace_fit(pts, w)
    Lc = np.linalg.cholesky(cov)
    prev = None
    for n in (65, 129, 257, 513, 1025):
        u = np.linspace(-10.0, 10.0, n)
        U = np.stack(np.meshgrid(u, u, indexing="ij"), axis=-1).reshape(-1, 2)
        th = mu + U.dot(Lc.T)
        lj = mod.log_joint(pts, th, w)
        p = np.exp(lj - lj.max())
        p /= p.sum()
        m = p.dot(th)
        S = (th - m).T.dot((th - m) * p[:, None])
        if prev is not None and max(np.abs(m - prev[0]).max(), np.abs(S - prev[1]).max()) < 1e-8:
            return m, S
        prev = (m, S)
    raise AssertionError("quadrature did not settle")


# Largest |z| observed on an MI355X with these seeds: see DESIGN.md 4.12.
def test_stationary_law_prior(bc):
    D = 4
    res = bc.DeviceHMC("logistic", D, chains=256, leapfrog=8, seed=31).sample(None, None, 1000, 1000, center=np.zeros(D), transform=np.eye(D))
    assert not res.streamed and res.samples.shape == (256, 1000, D)
    z = _moment_z(res.samples, np.zeros(D), np.eye(D))
    print("prior: largest |z| %.2f, rhat max %.4f, accept %.3f, step %.3f" % (np.abs(z).max(), res.rhat.max(), res.accept_rate.mean(), res.step_size.mean()))
    assert z.size == 14 and np.abs(z).max() <= 5.0, z
    assert res.rhat.max() <= 1.01
    assert abs(res.accept_rate.mean() - 0.8) <= 0.1


def test_stationary_law_logistic_quadrature(bc):
    import model_lr
    rs = np.random.RandomState(29)
    k = 25
    X = np.hstack((rs.randn(k, 1), np.ones((k, 1))))
    yv = np.where(rs.rand(k) < 1 / (1 + np.exp(-X.dot(np.array([1.2, -0.4])))), 1.0, -1.0)
    pts, w = yv[:, None] * X, rs.uniform(5.0, 60.0, k)
    mean, cov = _quadrature(model_lr, pts, w)
    res = bc.DeviceHMC("logistic", 2, chains=256, leapfrog=8, seed=37).sample(pts, w, 1000, 1000)
    assert not res.streamed
    z = _moment_z(res.samples, mean, cov)
    print("logistic D=2: largest |z| %.2f, rhat max %.4f, accept %.3f, step %.3f" % (np.abs(z).max(), res.rhat.max(), res.accept_rate.mean(), res.step_size.mean()))
    assert z.size == 5 and np.abs(z).max() <= 5.0, z
    assert res.rhat.max() <= 1.01
    assert abs(res.accept_rate.mean() - 0.8) <= 0.1


# ---------------------------------------------------------------------------------------------------------------- 5
def test_laplace_agreement_at_large_weight(bc):
    g = np.load(os.path.join(ROOT, "tests", "golden", "poiss_golden.npz"))
    w = g["poiss_w"]
    sel = np.flatnonzero(w > 0)
    res = bc.DeviceHMC("poisson", 4, chains=64, leapfrog=8, seed=5).sample(g["poiss_Z"][sel], w[sel], 1000)
    m = res.samples.reshape(-1, 4).mean(axis=0)
    rel = np.linalg.norm(m - g["poiss_wtd_mu"]) / np.linalg.norm(g["poiss_wtd_mu"])
    print("poiss_wtd: relative error of the HMC mean against the golden Laplace mode %.4g, rhat max %.4f" % (rel, res.rhat.max()))
    assert np.isfinite(rel) and np.all(np.isfinite(res.samples))
    assert res.rhat.max() <= 1.01


# ---------------------------------------------------------------------------------------------------------------- 6
def test_failures_stick(bc, gold):
    from bayesiancoresets_amd import _native
    pts, wts, D = _case(gold, "logistic")
    bad = wts.copy()
    bad[3] = np.nan
    hmc = bc.DeviceHMC("logistic", D, chains=8, seed=1)
    with pytest.raises(_native.EngineError):
        hmc.sample(pts, bad, 10)
    for streamed in (False, True):
        with pytest.raises(_native.EngineError):
            hmc.sample(pts, bad, 10, center=np.zeros(D), transform=np.eye(D), _dev_force_stream=streamed)
        res = hmc.sample(pts, wts, 20, 0, center=np.zeros(D), transform=np.eye(D), _dev_step_size=1e6, _dev_force_stream=streamed)
        assert np.all(res.accept_rate == 0.0) and not res.accepted.any()
        assert np.all(np.isfinite(res.samples)) and np.all(res.samples == 0.0)


# ---------------------------------------------------------------------------------------------------------------- 7
def test_reproducible_and_limits(bc, gold):
    from bayesiancoresets_amd import _native
    lib = _native.load()
    pts, wts, D = _case(gold, "poisson")
    a = bc.DeviceHMC("poisson", D, chains=16, seed=9).sample(pts, wts, 50)
    b = bc.DeviceHMC("poisson", D, chains=16, seed=9).sample(pts, wts, 50)
    c = bc.DeviceHMC("poisson", D, chains=16, seed=10).sample(pts, wts, 50)
    assert np.array_equal(a.samples, b.samples) and np.array_equal(a.delta_h, b.delta_h)
    assert not np.array_equal(a.samples, c.samples)
    assert lib.bcx_hmc_coreset_ok(40, 5) and not lib.bcx_hmc_coreset_ok(1 << 20, 10) and not lib.bcx_hmc_coreset_ok(10, 33)
    big = np.repeat(pts, 400, axis=0)                          # 24 000 points of 4 parameters: past any workgroup's LDS
    assert not lib.bcx_hmc_coreset_ok(big.shape[0], D)
    mu, cov = _model("poisson").laplace_fit(pts, wts * 400)
    r = bc.DeviceHMC("poisson", D, chains=16, seed=9).sample(big, np.repeat(wts, 400), 5, 5, center=mu, transform=np.linalg.cholesky(cov).T)
    assert r.streamed and np.all(np.isfinite(r.samples))
    with pytest.raises(ValueError):
        bc.DeviceHMC("logistic", 33)
    with pytest.raises(ValueError):
        bc.log_joint_grad("logistic", np.zeros((3, 33)), None, np.zeros((1, 33)))
