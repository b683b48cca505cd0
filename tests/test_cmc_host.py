"""CPU-only: the yardsticks of Coreset MCMC.  The NumPy restatement (tests/cmc_restatement.py) learns weights on
the small logistic problem; one chain leaves them alone; its weight step is ``nn_opt``'s; the new symbols are declared and
exported."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bayesian-coresets_amd", "examples", "common"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cmc_restatement as cr  # noqa: E402
import model_lr  # noqa: E402


def gaussian_kl(mu0, Sig0, mu1, Sig1):
    """KL(N(mu0, Sig0) || N(mu1, Sig1))."""
    Sig1inv = np.linalg.inv(Sig1)
    diff = mu1 - mu0
    return 0.5 * (np.trace(Sig1inv.dot(Sig0)) + diff.dot(Sig1inv).dot(diff) - np.linalg.slogdet(Sig1inv)[1] - np.linalg.slogdet(Sig0)[1]
                  - mu0.shape[0])


def problem(seed, N=2000, D=3, M=20):
    """The small logistic problem: x ~ N(0, I_D), theta = 1, y ~ Bernoulli(sigmoid(x.theta)) in {-1, +1}, rows y x; M points drawn
    uniformly; the frame is the Laplace fit of the uniform coreset.  (The uniform coreset's Laplace KL is 110 .. 2400 over seeds
    1 .. 6: the range of the prototype runs)"""
    rs = np.random.RandomState(seed)
    X = rs.randn(N, D)
    Z = np.where(rs.rand(N) < 1.0 / (1.0 + np.exp(-X.sum(axis=1))), 1.0, -1.0)[:, None] * X
    idcs = rs.choice(N, M, replace=False)
    pts = Z[idcs]
    mu, cov = model_lr.laplace_fit(pts, np.full(M, N / M))
    return rs, Z, pts, mu, np.linalg.cholesky(cov).T


def laplace_kl(Z, pts, w, full=None):
    """The Laplace KL from the weighted coreset's posterior to the full data's."""
    full = model_lr.laplace_fit(Z, None) if full is None else full
    keep = w > 0
    muw, Sigw = model_lr.laplace_fit(pts[keep], w[keep])
    return gaussian_kl(muw, Sigw, full[0], full[1])


@pytest.mark.parametrize("seed", (1, 2, 3, 4, 5, 6))
def test_restatement_learns(seed):
    """K = 16, the default schedule, T = 200, 8 leapfrog steps, 200 sub-sampled rows per iteration: the final Laplace KL is at most
    1/10 of the uniform coreset's (observed with the prototype: at most 1/32)."""
    N, D, M, K, T, L, n_sub = 2000, 3, 20, 16, 200, 8, 200
    rs, Z, pts, mu, W = problem(seed, N, D, M)
    noise = rs.randn(T, K, 1, D + 3)
    tables = np.stack([rs.randint(N, size=n_sub) for _ in range(T)])
    ws, ths, accs = cr.run("logistic", Z, pts, D, mu, W, K, L, 1, T, noise, tables)
    full = model_lr.laplace_fit(Z, None)
    before, after = laplace_kl(Z, pts, np.full(M, N / M), full), laplace_kl(Z, pts, ws[-1], full)
    print("seed %d: Laplace KL uniform %.4g, learned %.4g (factor %.1f), accept rate %.2f" % (seed, before, after, before / after, accs.mean()))
    assert np.isfinite(ws).all() and (ws >= 0).all()
    assert after <= before / 10.0


@pytest.mark.parametrize("dtype", (np.float64, np.longdouble))
def test_one_chain_leaves_the_weights(dtype):
    """K = 1: V centred over one chain is zero, so is the gradient, and ADAM's step 0 / (eps + 0) is zero: the weights stay, exactly."""
    N, D, M, T = 300, 3, 7, 5
    rs, Z, pts, mu, W = problem(11, N, D, M)
    ws, ths, accs = cr.run("logistic", Z, pts, D, mu, W, 1, 4, 2, T, rs.randn(T, 1, 2, D + 3), np.stack([rs.randint(N, size=50) for _ in range(T)]),
                           dtype=dtype)
    assert np.all(ws == N / M)
    assert accs.any()                                                      # (the chain itself moved)


def test_step_is_nn_opt():
    """The restatement's gradient and ADAM step against ``bc.util.opt.nn_opt`` on the same gradient, over several steps."""
    from bayesiancoresets_amd.util.opt import nn_opt
    rs = np.random.RandomState(3)
    M, K, T, scaling = 9, 12, 6, 3.5
    Vs, ss = rs.randn(T, M, K) - 40.0, rs.randn(T, K)
    ss -= ss.mean(axis=1)[:, None]
    w0 = np.abs(rs.randn(M)) + 0.1
    sched = lambda i: 0.4 / (1.0 + i)
    calls = []

    def grd(w):
        i = len(calls)
        calls.append(i)
        Vc = Vs[i] - Vs[i].mean(axis=1)[:, None]
        return -Vc.dot(scaling * ss[i] - w.dot(Vc)) / K
    want = nn_opt(w0, grd, opt_itrs=T, step_sched=sched)
    w, m1, m2 = w0.copy(), np.zeros(M), np.zeros(M)
    for i in range(T):
        w, m1, m2 = cr.adam_step(w, cr.gradient(Vs[i], ss[i], w, scaling), m1, m2, i, sched(i))
    np.testing.assert_allclose(w, want, rtol=1e-12, atol=1e-14)
    # a NaN stays a NaN through the clamp
    g = np.zeros(M)
    g[2] = np.nan
    assert np.isnan(cr.adam_step(w0, g, np.zeros(M), np.zeros(M), 0, 0.1)[0][2])


def test_emit_centres_over_the_chains():
    rs, Z, pts, mu, W = problem(5, 200, 3, 6)
    th = rs.randn(4, 3)
    V, s, scale = cr.emit("logistic", pts, Z, np.array([3, 3, 7, 199]), th, 3)
    assert V.shape == (6, 4) and s.shape == (4,) and abs(s.sum()) <= 1e-12 * scale.max()
    raw = np.array([sum(-np.log1p(np.exp(-Z[r].dot(t))) for r in (3, 3, 7, 199)) for t in th])
    np.testing.assert_allclose(s, raw - raw.mean(), rtol=1e-12, atol=1e-12)


def test_symbols_declared_and_exported():
    from bayesiancoresets_amd import _native
    text = open(os.path.join(ROOT, "include", "bcx.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(bcx_[a-z_0-9]+)\s*\(", text))
    new = ("bcx_cmc_advance", "bcx_cmc_advance_ok", "bcx_cmc_advance_lds_bytes", "bcx_cmc_state_bytes")
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _native.load()
    for name in new:
        assert name in declared and name in _native.SYMBOLS and hasattr(lib, name), name
    assert lib.bcx_cmc_state_bytes(0) == -1 and lib.bcx_cmc_state_bytes(8193) == -1
    assert lib.bcx_cmc_state_bytes(3) == 3 * (6 * 32 + 16) * 8
    assert lib.bcx_cmc_advance_lds_bytes(10, 3) == (10 * 4 + 30) * 8 and lib.bcx_cmc_advance_lds_bytes(10, 33) == -1


def test_class_is_exported_and_needs_a_gpu():
    import torch
    import bayesiancoresets_amd as bc
    assert bc.CoresetMCMC is bc.coreset.CoresetMCMC and issubclass(bc.CoresetMCMC, bc.Coreset)
    Z = np.random.RandomState(0).randn(50, 3)
    for kw in (dict(family="linreg"), dict(chains=0), dict(leapfrog=0), dict(thin=0), dict(opt_itrs=-1), dict(n_subsample=0),
               dict(chains=8193)):
        args = dict(family="logistic")
        args.update(kw)
        with pytest.raises(ValueError):
            bc.CoresetMCMC(Z, **args)
    with pytest.raises(ValueError):
        bc.CoresetMCMC(np.random.RandomState(0).randn(50, 34), "logistic")    # D > 32
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            bc.CoresetMCMC(Z, "logistic")
