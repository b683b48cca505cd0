"""CPU-only: the host statements the device NUTS (csrc/nuts.hip) is held to.  (1) the recursive and the
iterative statement of the transition (tests/nuts_restatement.py) agree bit for bit at every transition; (2) the transition
leaves N(0, I) invariant on the prior: moments within 5 standard errors, the bar of test_hmc_host.py; (3) at most 1 % of the
transitions are too close to call (the long-double statement's smallest decision margin below 1e-9) and none of the others comes
out differently in float64 -- the condition tests/test_gpu_nuts.py relies on; (4) the constructor's argument checks; (5) the ABI."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bayesian-coresets_amd", "examples", "common"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import nuts_restatement as nr  # noqa: E402

J, EPS0 = 6, 0.5
CLOSE = 1e-9


def _logistic_case():
    """The logistic k = 40, D = 5 inputs of tests/test_gpu_hmc.py (_case)."""
    rs = np.random.RandomState(17)
    k, D = 40, 5
    X = np.hstack((rs.randn(k, D - 1), np.ones((k, 1))))
    yv = np.where(rs.rand(k) < 1 / (1 + np.exp(-X.dot(np.array([1.0, -0.5, 0.5, 0.2, 0.1])))), 1.0, -1.0)
    return yv[:, None] * X, rs.uniform(0.5, 8.0, k), D


def _frames():
    import model_lr
    pts, wts, D = _logistic_case()
    mu, cov = model_lr.laplace_fit(pts, wts)
    return {"prior": ("logistic", None, None, 4, None, None, 32, 150, 300),
            "whitened": ("logistic", pts, wts, D, mu, np.linalg.cholesky(cov).T, 8, 60, 60),
            "plain": ("logistic", pts, wts, D, None, None, 8, 60, 60)}


_RUNS = {}


def _runs(name):
    """Per chain: the float64 chain by the recursive statement, and the noise it read (seed 11)."""
    if name not in _RUNS:
        family, pts, wts, D, mu, Wm, C, nw, ns = _frames()[name]
        rs = np.random.RandomState(11)
        tgt = nr.Target(family, pts, wts, D, mu, Wm)
        chains = []
        for c in range(C):
            z = rs.randn(nw + ns, nr.noise_columns(D, J))
            chains.append((z, nr.run_chain(tgt, z, nw, J, EPS0)))
        _RUNS[name] = (tgt, nw, chains)
    return _RUNS[name]


@pytest.mark.parametrize("name", ("prior", "whitened", "plain"))
def test_two_statements_agree(name):
    tgt, nw, chains = _runs(name)
    n = 0
    for z, rec in chains:
        it = nr.run_chain(tgt, z, nw, J, EPS0, step=nr.transition_iterative)
        for q in ("depth", "n_leapfrog", "alpha", "divergent", "xi", "theta", "base"):
            assert np.array_equal(rec[q], it[q]), (name, q)
        assert rec["step"] == it["step"]
        n += z.shape[0]
    depth = np.concatenate([r["depth"] for _, r in chains])
    leaps = np.concatenate([r["n_leapfrog"] for _, r in chains])
    print("%s: %d transitions, depth histogram %s, mean leapfrogs %.2f, step %.3f, divergent %d"
          % (name, n, np.bincount(depth, minlength=J + 1).tolist(), leaps.mean(), np.mean([r["step"] for _, r in chains]),
             sum(int(r["divergent"].sum()) for _, r in chains)))
    assert (leaps >= (1 << depth) - 1).all() and (leaps <= (1 << np.minimum(depth + 1, J)) - 1).all()


def test_restatement_samples_the_prior():
    tgt, nw, chains = _runs("prior")
    D, C = tgt.D, len(chains)
    means, covs = [], []
    for _, r in chains:
        s = r["theta"][nw:]
        means.append(s.mean(axis=0))
        covs.append((s[:, :, None] * s[:, None, :]).mean(axis=0))          # (second moments about the known mean 0)
    means, covs = np.array(means), np.array(covs)
    iu = np.triu_indices(D)
    est = np.concatenate((means.mean(axis=0), covs.mean(axis=0)[iu]))
    se = np.concatenate((means.std(axis=0, ddof=1), covs.std(axis=0, ddof=1)[iu])) / np.sqrt(C)
    z = (est - np.concatenate((np.zeros(D), np.eye(D)[iu]))) / se
    print("prior moments: largest |z| %.2f" % np.abs(z).max())
    assert np.abs(z).max() <= 5.0, z


@pytest.mark.parametrize("name", ("prior", "whitened", "plain"))
def test_close_calls_are_rare_and_the_rest_agree(name):
    """Every transition of the float64 chains restarted in long double from the same state, step and noise."""
    tgt, nw, chains = _runs(name)
    family, pts, wts, D, mu, Wm = _frames()[name][:6]
    tl = nr.Target(family, pts, wts, D, mu, Wm, np.longdouble)
    total = close = wrong = 0
    worst, smallest = 0.0, np.inf
    for z, rec in chains:
        for t in range(z.shape[0]):
            xi = rec["xi"][t - 1] if t else np.zeros(D)
            r = nr.transition_recursive(tl, xi, z[t], rec["base"][t], J)
            total += 1
            smallest = min(smallest, r["margin"])
            if r["margin"] < CLOSE:
                close += 1
                continue
            wrong += (r["depth"], r["n_leapfrog"], r["divergent"]) != (rec["depth"][t], rec["n_leapfrog"][t], rec["divergent"][t])
            worst = max(worst, float(np.abs(rec["xi"][t] - r["state"]).max()))
    print("%s: %d transitions, %d too close (smallest margin %.3g), %d differ, states within %.3g" % (name, total, close, smallest, wrong, worst))
    assert close <= 0.01 * total
    assert wrong == 0


def test_argument_checks_need_no_gpu():
    import bayesiancoresets_amd as bc
    with pytest.raises(ValueError):
        bc.DeviceHMC("logistic", 4, kernel="x")
    with pytest.raises(ValueError):
        bc.DeviceHMC("logistic", 4, kernel="nuts", max_depth=0)
    with pytest.raises(ValueError):
        bc.DeviceHMC("logistic", 4, kernel="nuts", max_depth=11)


def test_abi_lists_the_nuts_symbols():
    from bayesiancoresets_amd import _native
    text = open(os.path.join(ROOT, "include", "bcx.h")).read()
    for name in ("bcx_nuts_coreset", "bcx_nuts_coreset_ok", "bcx_nuts_coreset_lds_bytes"):
        assert name in _native.SYMBOLS
        assert name + "(" in text
