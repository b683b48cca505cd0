"""CPU-only: the host statements the metric adaptation of the device NUTS (csrc/nuts_adapt.h) is held to.
(1) bcx_nuts_adapt_schedule equals the restatement's schedule; (2) the ABI; (3) the windowed chain in float64 and in long double
agree on every decision that is not too close to call; (4) the adapted chain leaves N(0, I) invariant on the prior; (5) on a badly
scaled target with the identity frame the learned metric at least halves the leapfrog steps per sampling transition; (6) the
constructor's argument checks."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bayesian-coresets_amd", "examples", "common"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import nuts_adapt_restatement as ar  # noqa: E402
import nuts_restatement as nr  # noqa: E402

CLOSE = 1e-9
EPS0 = 0.5


# ---------------------------------------------------------------------------------------------------------------- 1, 2
def test_schedule_equals_restatement():
    from bayesiancoresets_amd import _native
    lib = _native.load()
    buf = (ctypes.c_int32 * 64)()
    for n in range(0, 3001):
        cnt = lib.bcx_nuts_adapt_schedule(n, buf, 32)
        got = [(buf[2 * i], buf[2 * i + 1]) for i in range(cnt)]
        assert got == ar.schedule(n), n
        assert cnt == lib.bcx_nuts_adapt_schedule(n, None, 0)
        if cnt:                                                   # contiguous, inside the warm-up, a fast phase behind them
            assert all(a < b for a, b in got) and all(got[i][1] == got[i + 1][0] for i in range(cnt - 1))
            assert 0 <= got[0][0] and got[-1][1] < n
        else:
            assert n < 20
    assert ar.schedule(100) == [(15, 90)]
    assert ar.schedule(150) == [(75, 100)]
    assert ar.schedule(200) == [(75, 100), (100, 150)]
    assert ar.schedule(1000) == [(75, 100), (100, 150), (150, 250), (250, 450), (450, 950)]
    assert ar.schedule(19) == [] and ar.schedule(20) == [(3, 18)]
    assert lib.bcx_nuts_adapt_schedule(2 ** 31 - 1, None, 0) <= 32
    assert ar.segments(200) == [(0, 100), (100, 150), (150, 200)] and ar.segments(19) == [(0, 19)]


def test_abi_lists_the_adapt_symbols():
    from bayesiancoresets_amd import _native
    text = open(os.path.join(ROOT, "include", "bcx.h")).read()
    for name in ("bcx_nuts_adapt", "bcx_nuts_adapt_ok", "bcx_nuts_adapt_schedule"):
        assert name in _native.SYMBOLS
        assert name + "(" in text
        assert hasattr(_native.load(), name)


# ---------------------------------------------------------------------------------------------------------------- 3
def _logistic_case():
    """The logistic k = 40, D = 5 inputs of tests/test_gpu_hmc.py (_case)."""
    rs = np.random.RandomState(17)
    k, D = 40, 5
    X = np.hstack((rs.randn(k, D - 1), np.ones((k, 1))))
    yv = np.where(rs.rand(k) < 1 / (1 + np.exp(-X.dot(np.array([1.0, -0.5, 0.5, 0.2, 0.1])))), 1.0, -1.0)
    return yv[:, None] * X, rs.uniform(0.5, 8.0, k), D


@pytest.mark.parametrize("metric", ("diag", "dense"))
def test_float64_and_long_double_agree(metric):
    """Every transition of float64 chains (identity frame, 100 + 20 transitions: one window) restarted in long double from the
    same state, frame, step and noise; the window's end restated in long double from the float64 chain's own draws."""
    pts, wts, D = _logistic_case()
    J, nw, ns = 6, 100, 20
    rs = np.random.RandomState(13)
    total = close = wrong = 0
    worst = worst_L = 0.0
    for c in range(4):
        z = rs.randn(nw + ns, nr.noise_columns(D, J))
        rec = ar.run_chain("logistic", pts, wts, D, None, None, z, nw, J, EPS0, metric)
        assert len(rec["frames"]) == 1 and rec["window"][89] == 0 and rec["window"][90] == 1
        for t in range(nw + ns):
            L = np.eye(D) if rec["window"][t] == 0 else rec["frames"][rec["window"][t] - 1]
            tl = ar.framed_target("logistic", pts, wts, D, None, None, L, np.longdouble)
            r = nr.transition_recursive(tl, rec["start"][t], z[t], rec["base"][t], J)
            total += 1
            if r["margin"] < CLOSE:
                close += 1
                continue
            wrong += (r["depth"], r["n_leapfrog"], r["divergent"]) != (rec["depth"][t], rec["n_leapfrog"][t], rec["divergent"][t])
            worst = max(worst, float(np.abs(rec["eta"][t] - r["state"]).max()))
        Ll, el = ar.window_end(rec["eta"][15:90], metric, np.longdouble)       # (L = I in the window: xi0 = eta)
        worst_L = max(worst_L, float(np.abs(rec["frames"][0] - Ll).max()), float(np.abs(rec["start"][90] - el).max()))
        off = rec["frames"][0][np.tril_indices(D, -1)]
        assert (off != 0).all() if metric == "dense" else (off == 0).all()
    print("%s: %d transitions, %d too close, %d differ, states within %.3g, window end within %.3g" % (metric, total, close, wrong, worst, worst_L))
    assert close <= 0.01 * total
    assert wrong == 0
    # 75 Welford updates of O(1) draws, a 5 x 5 factorisation of a matrix of condition < 100 and one forward substitution: a few
    # hundred roundings of 1.1e-16 at the outside, amplified by the condition -- 1e-12 is that bound, not a measured figure
    assert worst_L <= 1e-12


# ---------------------------------------------------------------------------------------------------------------- 4
def test_adapted_restatement_samples_the_prior():
    D, J, C, nw, ns = 4, 6, 32, 150, 300
    rs = np.random.RandomState(11)
    means, covs = [], []
    for c in range(C):
        z = rs.randn(nw + ns, nr.noise_columns(D, J))
        r = ar.run_chain("logistic", None, None, D, None, None, z, nw, J, EPS0, "dense")
        assert len(r["frames"]) == 1 and not r["divergent"][nw:].any()
        s = r["theta"][nw:]
        means.append(s.mean(axis=0))
        covs.append((s * s).mean(axis=0))                                  # (second moments about the known mean 0)
    means, covs = np.array(means), np.array(covs)
    est = np.concatenate((means.mean(axis=0), covs.mean(axis=0)))
    se = np.concatenate((means.std(axis=0, ddof=1), covs.std(axis=0, ddof=1))) / np.sqrt(C)
    z = (est - np.concatenate((np.zeros(D), np.ones(D)))) / se
    print("adapted prior moments: largest |z| %.2f" % np.abs(z).max())
    assert np.abs(z).max() <= 5.0, z


# ---------------------------------------------------------------------------------------------------------------- 5
def test_learned_metric_halves_the_leapfrogs():
    """DESIGN.md 4.17's figures: 6 chains x (200 + 200), J = 8, W = I on the badly scaled logistic target."""
    pts, wts, rng = ar.scaled_logistic_case()
    D, J, C, nw, ns = 3, 8, 6, 200, 200
    noise = rng.standard_normal((C, nw + ns, nr.noise_columns(D, J)))
    leaps, steps, moments, div = {}, {}, {}, {}
    for metric in (None, "diag", "dense"):
        runs = [ar.run_chain("logistic", pts, wts, D, None, None, noise[c], nw, J, EPS0, metric) for c in range(C)]
        leaps[metric] = float(np.mean([r["n_leapfrog"][nw:].mean() for r in runs]))
        steps[metric] = float(np.mean([r["step"] for r in runs]))
        div[metric] = int(sum(r["divergent"][nw:].sum() for r in runs))
        th = np.array([r["theta"][nw:] for r in runs])
        moments[metric] = (th.mean(axis=(0, 1)), th.mean(axis=1).std(axis=0, ddof=1) / np.sqrt(C))
        print("metric %s: %.1f leapfrogs per sampling transition, step %.3g, divergent %d, mean %s" % (metric, leaps[metric], steps[metric], div[metric], moments[metric][0]))
    for metric in ("diag", "dense"):
        assert leaps[metric] <= 0.5 * leaps[None], (metric, leaps)
        assert div[metric] == 0
        se = np.sqrt(moments[metric][1] ** 2 + moments[None][1] ** 2)
        assert (np.abs(moments[metric][0] - moments[None][0]) <= 5 * se).all()


# ---------------------------------------------------------------------------------------------------------------- 6
def test_argument_checks_need_no_gpu():
    import bayesiancoresets_amd as bc
    with pytest.raises(ValueError, match="adapt_metric"):
        bc.DeviceHMC("logistic", 4, kernel="nuts", adapt_metric="full")
    with pytest.raises(ValueError, match="drop adapt_metric"):
        bc.DeviceHMC("logistic", 4, kernel="hmc", adapt_metric="diag")
    with pytest.raises(ValueError, match="drop"):
        bc.DeviceHMC("logistic", 4, kernel="nuts", stream=True, adapt_metric="dense")


def test_harness_switch_is_absent_unless_given():
    """--mcmc_adapt_metric has a suppressed default: without it the argument set, hence every result file's name, is unchanged."""
    import importlib.util
    path = os.path.join(ROOT, "bayesian-coresets_amd", "examples", "logistic_poisson_regression", "main.py")
    spec = importlib.util.spec_from_file_location("_lpr_main_adapt", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ap = mod.parser()
    assert not hasattr(ap.parse_args(["run"]), "mcmc_adapt_metric")
    a = ap.parse_args(["--eval", "mcmc", "--mcmc_kernel", "nuts", "--mcmc_adapt_metric", "diag", "run"])
    assert a.mcmc_adapt_metric == "diag"
    with pytest.raises(SystemExit):
        ap.parse_args(["--mcmc_adapt_metric", "full", "run"])
    a = ap.parse_args(["--mcmc_adapt_metric", "dense", "run"])                   # (without --eval mcmc --mcmc_kernel nuts it is refused)
    with pytest.raises(ValueError, match="mcmc_adapt_metric"):
        mod.run(a)
