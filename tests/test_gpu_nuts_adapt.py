"""GPU: the metric bc.DeviceHMC(kernel="nuts", adapt_metric="diag" | "dense") learns in its windowed warm-up (csrc/nuts_adapt.h,
DESIGN.md 4.17).  (1) nothing differs from the run without a metric before the first window ends; (2) every transition and every
window end against the long-double statement (tests/nuts_adapt_restatement.py), teacher-forced; (3) the smallest shapes; (4) ground
truths no sampler produced; (5) the benefit on a badly scaled target with the identity frame; (6) limits and reproducibility."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bayesian-coresets_amd", "examples", "common"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import nuts_adapt_restatement as ar  # noqa: E402
import nuts_restatement as nr  # noqa: E402
from test_gpu_hmc import _case, _moment_z, _quadrature  # noqa: E402
from test_gpu_nuts import _small  # noqa: E402

pytestmark = pytest.mark.gpu
CLOSE = 1e-9
QUANTITIES = ("xi", "alpha", "eps", "dsel", "L", "eta")


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


def _steps_run_with(res):
    """The step every transition ran with: the start step, then the base step the transition before handed on."""
    dg = res.trace["diag"]
    return np.concatenate((np.full((dg.shape[0], 1), res.trace["step0"]), dg[:, :-1, 3]), axis=1)


# ---------------------------------------------------------------------------------------------------------------- 1
def test_nothing_differs_before_the_first_window_ends(bc, gold):
    pts, wts, D = _case(gold, "logistic")
    kw = dict(chains=8, seed=5, kernel="nuts", max_depth=6)
    plain = bc.DeviceHMC("logistic", D, **kw)
    dense = bc.DeviceHMC("logistic", D, adapt_metric="dense", **kw)
    a, b = plain.sample(pts, wts, 10, 19, keep_trace=True), dense.sample(pts, wts, 10, 19, keep_trace=True)
    assert b.adapt_metric == "dense" and a.adapt_metric is None and b.metric_windows.shape == (0, 2)
    for q in ("samples", "accept_rate", "step_size", "delta_h", "accept_stat", "tree_depth", "n_leapfrog", "divergent", "accepted"):
        assert np.array_equal(getattr(a, q), getattr(b, q)), q
    for q in ("noise", "theta", "xi", "proposal", "diag"):
        assert np.array_equal(a.trace[q], b.trace[q]), q
    assert np.array_equal(b.metric, np.broadcast_to(np.eye(D), (8, D, D))) and b.trace["frames"].shape == (8, 0, D, D)
    plain = bc.DeviceHMC("logistic", D, **kw)
    dense = bc.DeviceHMC("logistic", D, adapt_metric="dense", **kw)
    a, b = plain.sample(pts, wts, 5, 200, keep_trace=True), dense.sample(pts, wts, 5, 200, keep_trace=True)
    assert b.metric_windows.tolist() == [[75, 100], [100, 150]]
    assert np.array_equal(a.trace["theta"][:, :100], b.trace["theta"][:, :100])
    assert np.array_equal(a.trace["xi"][:, :100], b.trace["xi"][:, :100])
    assert np.array_equal(a.trace["diag"][:, :100, 1:3], b.trace["diag"][:, :100, 1:3])
    assert np.array_equal(_steps_run_with(a)[:, :100], _steps_run_with(b)[:, :100])
    assert not np.array_equal(a.trace["theta"][:, 100:], b.trace["theta"][:, 100:])          # (and it does differ behind it)


# ---------------------------------------------------------------------------------------------------------------- 2
def _tolerances(f64):
    """The rule of _hold in tests/test_gpu_nuts.py: 16 x the float64 statement's own deviation from the long-double one, per
    quantity, at least 32 ulp of the scale."""
    return {q: max(16.0 * f64[q], 32 * 2.0 ** -52) for q in f64}


def _teacher_forced(family, pts, wts, D, J, res, metric):
    """Every transition of the device run restarted in the recursive statement from the device's previous eta, frame, step and
    noise row, and every window end restated from the device's own draws of the window, in long double (the referee) and in
    float64.  Per quantity the device's and the float64 statement's largest deviation from the referee in units of the
    quantity's scale; the transitions that disagree on depth / leapfrog count / divergence; those too close to call."""
    tr = res.trace
    dg, frames, wins = tr["diag"], tr["frames"], [tuple(w) for w in res.metric_windows.tolist()]
    C, T = dg.shape[:2]
    nw, eps0 = res.n_warmup, tr["step0"]
    segs = ar.segments(nw)
    ends = {e: i for i, (_, e) in enumerate(wins)}
    dev, f64 = dict.fromkeys(QUANTITIES, 0.0), dict.fromkeys(QUANTITIES, 0.0)
    wrong = close = 0

    def note(q, a, b):
        dev[q], f64[q] = max(dev[q], float(a)), max(f64[q], float(b))

    for c in range(C):
        wi, si = 0, 0
        tl = td = None
        for t in range(T):
            if t in ends:                      # the window ends[t] ended behind transition t - 1: the statement of that end
                s, e = wins[ends[t]]
                Lp = np.eye(D) if wi == 0 else frames[c, wi - 1]
                Ll, el = ar.window_end(tr["xi"][c, s:e].astype(np.longdouble).dot(Lp.astype(np.longdouble).T), metric, np.longdouble)
                Ld, ed = ar.window_end(tr["xi"][c, s:e].dot(Lp.T), metric, np.float64)
                sL, se = max(1.0, float(np.abs(Ll).max())), max(1.0, float(np.abs(el).max()))
                note("L", np.abs(frames[c, wi] - Ll).max() / sL, np.abs(Ld - Ll).max() / sL)
                note("eta", np.abs(tr["proposal"][c, t - 1] - el).max() / se, np.abs(ed - el).max() / se)
                wi, tl = wi + 1, None
            else:
                assert t == 0 or np.array_equal(tr["proposal"][c, t - 1], tr["xi"][c, t - 1])    # (the proposal is the selected state)
            if tl is None:
                L = np.eye(D) if wi == 0 else frames[c, wi - 1]
                tl = ar.framed_target(family, pts, wts, D, res.center, res.transform, L, np.longdouble)
                td = ar.framed_target(family, pts, wts, D, res.center, res.transform, L, np.float64)
            while si + 1 < len(segs) and t >= segs[si][1]:
                si += 1
            s0, s1 = segs[si]
            start = np.zeros(D) if t == 0 else (tr["proposal"] if t in ends else tr["xi"])[c, t - 1]
            base = eps0 if t == 0 else dg[c, t - 1, 3]
            z = tr["noise"][c, t]
            rl, rd = nr.transition_recursive(tl, start, z, base, J), nr.transition_recursive(td, start, z, base, J)
            if t >= nw:
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
            note("xi", np.abs(tr["xi"][c, t] - rl["state"]).max() / sx, np.abs(rd["state"] - rl["state"]).max() / sx)
            note("alpha", abs(dg[c, t, 0] - rl["alpha"]), abs(rd["alpha"] - rl["alpha"]))
            note("dsel", abs(dg[c, t, 7] - rl["dsel"]) / sh, abs(rd["dsel"] - rl["dsel"]) / sh)
            if t < nw:
                hbar, lebar = (0.0, 0.0) if t == s0 else dg[c, t - 1, 4:6]
                seg_eps = eps0 if s0 == 0 else dg[c, s0 - 1, 3]
                nl = nr.dual_average_alpha(t - s0 + 1, rl["alpha"], hbar, lebar, seg_eps, t + 1 == s1, np.longdouble)[0]
                nd = nr.dual_average_alpha(t - s0 + 1, rd["alpha"], hbar, lebar, seg_eps, t + 1 == s1, np.float64)[0]
                note("eps", abs(dg[c, t, 3] - nl) / nl, abs(nd - nl) / nl)
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


# Observed on an MI355X: see DESIGN.md 4.17.
@pytest.mark.parametrize("metric", ("diag", "dense"))
@pytest.mark.parametrize("family", ("logistic", "poisson"))
def test_transitions_and_window_ends_equal_restatement(bc, gold, family, metric):
    pts, wts, D = _case(gold, family)
    J = 6
    res = bc.DeviceHMC(family, D, chains=32, seed=2024, kernel="nuts", max_depth=J, adapt_metric=metric).sample(pts, wts, 100, 200, keep_trace=True)
    assert not res.streamed and res.kernel == "nuts" and res.adapt_metric == metric
    frames = res.trace["frames"]
    assert frames.shape == (32, 2, D, D) and res.metric.shape == (32, D, D) and np.array_equal(res.metric, frames[:, -1])
    assert res.metric_windows.tolist() == [[75, 100], [100, 150]]
    _hold("%s %s" % (family, metric), *_teacher_forced(family, pts, wts, D, J, res, metric))
    il, iu = np.tril_indices(D, -1), np.triu_indices(D, 1)
    assert (frames[:, :, iu[0], iu[1]] == 0).all() and (frames[:, :, np.arange(D), np.arange(D)] > 0).all()
    off = frames[:, :, il[0], il[1]]
    assert (off != 0).all() if metric == "dense" else (off == 0).all()
    dg = res.trace["diag"]
    assert np.array_equal(res.step_size, dg[:, 199, 3]) and np.array_equal(res.tree_depth, dg[:, 200:, 1].astype(int))
    print("%s %s: mean leapfrogs %.2f, step %.3f, divergent %d" % (family, metric, res.n_leapfrog.mean(), res.step_size.mean(), res.divergent.sum()))


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("metric", ("diag", "dense"))
@pytest.mark.parametrize("name,n_warmup", (("wide", 40), ("wide", 100), ("one", 40), ("prior", 40)))
def test_smallest_shapes(bc, name, n_warmup, metric):
    """D = 32 with k = 3 and a window of 30 < D draws (a rank-deficient covariance: the regulariser alone makes it definite), the
    same with 75 draws, D = 1 / k = 1, and no point at all."""
    family, pts, wts, D, mu, Wm = _small(name)
    hmc = bc.DeviceHMC(family, D, chains=8, seed=3, kernel="nuts", max_depth=3, adapt_metric=metric)
    res = hmc.sample(pts, wts, 10, n_warmup, center=mu, transform=Wm, keep_trace=True)
    wins = res.metric_windows.tolist()
    assert wins == [list(w) for w in ar.schedule(n_warmup)] and len(wins) == 1
    if name == "wide" and n_warmup == 40:
        assert wins[0][1] - wins[0][0] == 30 < D
    frames = res.trace["frames"]
    assert frames.shape == (8, 1, D, D) and np.isfinite(frames).all() and np.isfinite(res.samples).all()
    assert (frames[:, :, np.arange(D), np.arange(D)] > 0).all()
    assert not np.array_equal(frames[:, 0], np.broadcast_to(np.eye(D), (8, D, D)))          # (a frame was learned)
    assert np.array_equal(res.metric, frames[:, -1])
    assert not res.nonfinite_rejected and int(hmc._status.cpu().numpy()[0]) == 0
    assert np.array_equal(res.transform, Wm) and np.isfinite(res.step_size).all() and (res.step_size > 0).all()
    # the state is the same theta in both frames at the window's end (to rounding)
    e = wins[0][1]
    th_new = mu + np.einsum("cj,cij,ik->ck",res.trace["proposal"][:, e - 1], frames[:, 0], Wm)
    np.testing.assert_allclose(th_new, res.trace["theta"][:, e - 1], rtol=1e-10, atol=1e-10)


# ---------------------------------------------------------------------------------------------------------------- 4
# The bars of tests/test_gpu_nuts.py.  Largest |z| observed on an MI355X with these seeds: see DESIGN.md 4.17.
def test_stationary_law_prior(bc):
    D = 4
    res = bc.DeviceHMC("logistic", D, chains=256, seed=31, kernel="nuts", max_depth=6, adapt_metric="dense").sample(
        None, None, 1000, 1000, center=np.zeros(D), transform=np.eye(D))
    assert res.samples.shape == (256, 1000, D) and len(res.metric_windows) == 5
    z = _moment_z(res.samples, np.zeros(D), np.eye(D))
    print("prior: largest |z| %.2f, rhat max %.4f, mean depth %.2f, mean leapfrogs %.2f, accept statistic %.3f, step %.3f, divergent %d"
          % (np.abs(z).max(), res.rhat.max(), res.tree_depth.mean(), res.n_leapfrog.mean(), res.accept_rate.mean(), res.step_size.mean(), res.divergent.sum()))
    assert z.size == 14 and np.abs(z).max() <= 5.0, z
    assert res.rhat.max() <= 1.01


@pytest.mark.parametrize("metric", ("diag", "dense"))
def test_stationary_law_logistic_quadrature(bc, metric):
    import model_lr
    rs = np.random.RandomState(29)
    k = 25
    X = np.hstack((rs.randn(k, 1), np.ones((k, 1))))
    yv = np.where(rs.rand(k) < 1 / (1 + np.exp(-X.dot(np.array([1.2, -0.4])))), 1.0, -1.0)
    pts, w = yv[:, None] * X, rs.uniform(5.0, 60.0, k)
    mean, cov = _quadrature(model_lr, pts, w)
    res = bc.DeviceHMC("logistic", 2, chains=256, seed=37, kernel="nuts", max_depth=6, adapt_metric=metric).sample(
        pts, w, 1000, 1000, center=np.zeros(2), transform=np.eye(2))
    z = _moment_z(res.samples, mean, cov)
    print("logistic D=2 %s: largest |z| %.2f, rhat max %.4f, mean depth %.2f, mean leapfrogs %.2f, accept statistic %.3f, step %.3f, divergent %d"
          % (metric, np.abs(z).max(), res.rhat.max(), res.tree_depth.mean(), res.n_leapfrog.mean(), res.accept_rate.mean(), res.step_size.mean(), res.divergent.sum()))
    assert z.size == 5 and np.abs(z).max() <= 5.0, z
    assert res.rhat.max() <= 1.01


# ---------------------------------------------------------------------------------------------------------------- 5
def test_learned_metric_halves_the_leapfrogs(bc):
    """The target of tests/test_nuts_adapt_host.py: logistic, k = 60, D = 3, feature columns scaled by (1, 6, 30), the identity
    frame, J = 8, 32 chains x (200 + 200)."""
    pts, wts, _ = ar.scaled_logistic_case()
    D, J = 3, 8
    run = {}
    for metric in (None, "diag", "dense"):
        r = bc.DeviceHMC("logistic", D, chains=32, seed=77, kernel="nuts", max_depth=J, adapt_metric=metric).sample(
            pts, wts, 200, 200, center=np.zeros(D), transform=np.eye(D))
        run[metric] = r
        print("metric %s: %.2f leapfrogs per sampling transition, mean depth %.2f, step %.3g, divergent %d, mean %s"
              % (metric, r.n_leapfrog.mean(), r.tree_depth.mean(), r.step_size.mean(), r.divergent.sum(), r.samples.mean(axis=(0, 1))))
    m0 = run[None].samples.mean(axis=1)
    for metric in ("diag", "dense"):
        r = run[metric]
        assert r.n_leapfrog.mean() <= 0.5 * run[None].n_leapfrog.mean()
        assert r.tree_depth.mean() < J and (r.tree_depth < J).mean() > 0.99
        assert not r.divergent.any()
        m1 = r.samples.mean(axis=1)
        se = np.sqrt(m0.var(axis=0, ddof=1) / 32 + m1.var(axis=0, ddof=1) / 32)
        assert (np.abs(m1.mean(axis=0) - m0.mean(axis=0)) <= 5 * se).all(), (metric, m1.mean(axis=0), m0.mean(axis=0), se)


# ---------------------------------------------------------------------------------------------------------------- 6
def test_limits_and_reproducibility(bc, gold):
    import torch
    from bayesiancoresets_amd import _native
    lib = _native.load()
    pts, wts, D = _case(gold, "poisson")
    kw = dict(chains=16, kernel="nuts", max_depth=6, adapt_metric="dense")
    with pytest.raises(ValueError, match="drop adapt_metric"):
        bc.DeviceHMC("poisson", D, chains=16, kernel="hmc", adapt_metric="dense")
    with pytest.raises(ValueError, match="drop"):
        bc.DeviceHMC("poisson", D, chains=16, kernel="nuts", stream=True, adapt_metric="dense")
    with pytest.raises(ValueError, match="adapt_metric"):
        bc.DeviceHMC("poisson", D, chains=16, kernel="nuts", adapt_metric="full")
    hmc = bc.DeviceHMC("poisson", D, seed=9, **kw)
    with pytest.raises(ValueError, match="_dev_step_size"):
        hmc.sample(pts, wts, 5, 40, _dev_step_size=0.1)
    big = np.repeat(pts, 400, axis=0)                          # 24 000 points of 4 parameters: past any workgroup's LDS
    with pytest.raises(ValueError, match="drop adapt_metric"):
        hmc.sample(big, np.repeat(wts, 400), 5, 40, center=np.zeros(D), transform=np.eye(D))
    assert hmc.adapt_path(60) and not hmc.adapt_path(24000) and lib.bcx_nuts_adapt_ok(40, 5) and not lib.bcx_nuts_adapt_ok(10, 33)
    # the adapting kernel carries more static LDS: there are k the plain kernel holds and it does not, never the other way round
    ks = [k for k in range(100, 3000, 50) if lib.bcx_nuts_coreset_ok(k, D) != lib.bcx_nuts_adapt_ok(k, D)]
    assert ks and all(lib.bcx_nuts_coreset_ok(k, D) and not lib.bcx_nuts_adapt_ok(k, D) for k in ks)
    # a fixed step with a metric: BCX_ERR_ARG from the entry point itself
    f64 = dict(dtype=torch.float64, device="cuda")
    C, T, R, ld = 2, 30, nr.noise_columns(D, 2), D
    noise, samples, diag = torch.zeros(C, T, R, **f64), torch.zeros(C, T, ld, **f64), torch.zeros(C, T, 8, **f64)
    acc, eps, status = torch.zeros(C, **f64), torch.zeros(C, **f64), torch.zeros(2, dtype=torch.int32, device="cuda")
    frames, metric = torch.zeros(C, 1, D, D, **f64), torch.zeros(C, D, D, **f64)

    def call(fixed, which):
        return lib.bcx_nuts_adapt(None, 1, 0, D, None, None, D + 1, None, None, D, C, 20, 10, 2, 0.5, fixed, noise.data_ptr(), R, ld,
                                  samples.data_ptr(), None, None, diag.data_ptr(), acc.data_ptr(), eps.data_ptr(), status.data_ptr(), which,
                                  frames.data_ptr(), metric.data_ptr())
    assert call(0.1, 2) == _native.ERR_ARG and call(0.1, 1) == _native.ERR_ARG and call(0.0, 0) == _native.ERR_ARG and call(0.0, 3) == _native.ERR_ARG
    assert call(0.0, 2) == _native.OK
    torch.cuda.synchronize()
    assert np.isfinite(frames.cpu().numpy()).all() and (metric.cpu().numpy()[:, np.arange(D), np.arange(D)] > 0).all()
    a = bc.DeviceHMC("poisson", D, seed=9, **kw).sample(pts, wts, 50, 100)
    b = bc.DeviceHMC("poisson", D, seed=9, **kw).sample(pts, wts, 50, 100)
    c = bc.DeviceHMC("poisson", D, seed=10, **kw).sample(pts, wts, 50, 100)
    assert np.array_equal(a.samples, b.samples) and np.array_equal(a.metric, b.metric) and np.array_equal(a.n_leapfrog, b.n_leapfrog)
    assert np.array_equal(a.step_size, b.step_size)
    assert not np.array_equal(a.samples, c.samples) and not np.array_equal(a.metric, c.metric)
