"""GPU: SparseVI's device samplers and loop against independent references, and what happens when a step goes wrong.

* csrc/laplace.hip against fixture F15 (tests/golden/poiss_golden.npz: the reference's own ``get_laplace`` outputs);
* the enqueued loop at the reference's coreset sizes against oracle/sparsevi_oracle.py driven by a NumPy sampler (the
  reference's ``sampler_w`` arithmetic, tests/models.py, pinned by F12) instead of the package's own sampler;
* failures that must stick: a failed D x D factorisation (csrc/lrpost.hip) or Laplace fit at one step of a loop is reported by
  the plan's ``check()`` even when later steps succeed, and a NaN that reaches the loop ends it with ``EngineError`` where the
  reference ends with NaN weights."""
import os

import numpy as np
import pytest

from models import linreg_sampler, linreg_weighted_post, make_linreg_data
from test_gpu_svi import _ReplaySampler, sys_path_examples

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bc():
    import bayesiancoresets_amd as bc
    return bc


def _model(rs, D):
    A0 = rs.randn(D, D)
    return 0.2 * rs.randn(D), 1.5 * (A0.dot(A0.T) / D + np.eye(D)), 0.8


# ---- A. independent references -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ("poiss_full", "poiss_wtd", "lr_full", "lr_wtd"))
def test_laplace_kernel_against_F15(bc, tag):
    """The device Laplace fit (csrc/laplace.hip, one launch) on the reference's own inputs: mode and covariance W^T W against
    its ``get_laplace`` at the CPU F15 tolerances (bounded by the reference's BFGS gtol, tests/test_poisson_model.py), and
    against the package's Newton ``laplace_fit`` on the same objective to 1e-10."""
    sys_path_examples()
    import model_lr
    import model_poiss
    g = np.load(os.path.join(ROOT, "tests", "golden", "poiss_golden.npz"))
    family, Z, fit = ("poisson", g["poiss_Z"], model_poiss.laplace_fit) if tag.startswith("poiss") else ("logistic", g["lr_Z"], model_lr.laplace_fit)
    full = tag.endswith("_full")
    w = np.ones(Z.shape[0]) if full else g["poiss_w"]
    D = Z.shape[1] - (1 if family == "poisson" else 0)
    smp = bc.LaplacePosteriorSampler(family, D, seed=2)
    mu, W = smp.posterior(w, Z)
    cov = W.T.dot(W)
    np.testing.assert_allclose(mu, g[tag + "_mu"], rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(cov, g[tag + "_cov"], rtol=2e-4, atol=1e-7)
    mu_h, cov_h = fit(Z, None if full else w)
    np.testing.assert_allclose(mu, mu_h, rtol=1e-10, atol=1e-10 * np.abs(mu_h).max())
    np.testing.assert_allclose(cov, cov_h, rtol=1e-10, atol=1e-10 * np.abs(cov_h).max())


@pytest.mark.parametrize("D,k,colsum", ((301, 28, "moments"), (24, 65, "mfma"), (24, 130, "moments"), (301, 300, "moments"), (12, 300, "mfma")))
def test_enqueued_loop_against_the_oracle_with_numpy_draws(bc, D, k, colsum):
    """As test_gpu_svi.py::test_enqueued_loop_against_the_oracle_at_reference_coreset_sizes, but the oracle's sampler is the
    reference's arithmetic in NumPy, mu_w + R U^T with (mu_w, U = L^-T) from tests/models.py linreg_weighted_post, fed the
    same normal numbers R: the device's D x D factorisation is checked end to end against LAPACK, not against itself.  Every
    case takes the D x D path (``plan.factored``), whose draw is the same form mu_w + R L^-1."""
    import torch
    from oracle.sparsevi_oracle import SparseVIOracle, linreg_loglik
    N, S, T = 4000, 32, 12
    rs = np.random.RandomState(100 * D + k)
    Z = make_linreg_data(13, N, D)
    mu0, Sig0, sigsq = _model(rs, D)
    idcs = np.sort(rs.choice(N, size=k, replace=False)).astype(np.int64)
    w0 = np.abs(rs.randn(k)) * (N / k)
    w0[::7] = 0.0
    g = torch.Generator(device="cuda")
    g.manual_seed(29)
    noise = torch.randn(T + 3, S, D + D % 2, dtype=torch.float64, device="cuda", generator=g)
    R = noise.cpu().numpy()[:, :, :D]
    S0inv, at = np.linalg.inv(Sig0), [0]

    def numpy_sampler(n, w, p):
        r = R[at[0]]
        at[0] += 1
        w = np.asarray(w, dtype=np.float64)
        if w.shape[0] == 0:
            return mu0 + r.dot(np.linalg.cholesky(Sig0).T)
        mu, U = linreg_weighted_post(mu0, S0inv, sigsq, p, w)
        return mu + r.dot(U.T)
    orc = SparseVIOracle(Z, numpy_sampler, lambda z, th: linreg_loglik(z, th, sigsq), S, opt_itrs=T)
    orc.wts, orc.idcs, orc.pts = w0.copy(), idcs.copy(), Z[idcs].copy()
    orc.optimize()
    smp = _ReplaySampler(bc.LinregPosteriorSampler(mu0, Sig0, sigsq), noise)
    alg = bc.SparseVICoreset(Z, bc.DeviceProjector("linreg", smp, S, sigsq=sigsq, colsum=colsum), opt_itrs=T)
    alg.wts, alg.idcs, alg.pts = w0.copy(), idcs.copy(), Z[idcs].copy()
    plan = alg._enqueue_plan()
    assert plan is not None and plan.factored and not plan.fast
    smp.at -= T
    alg._optimize()
    assert smp.at == at[0] == 1 + T
    assert (alg.wts > 0).sum() >= k // 2
    np.testing.assert_allclose(alg.wts, orc.wts, rtol=1e-7, atol=1e-9 * np.abs(orc.wts).max())


# ---- B. failures that stick ---------------------------------------------------------------------------------------------
def test_failed_factorisation_at_one_step_is_reported_after_the_loop(bc):
    """D x D plan (D = 301, k = 28): a NaN weight at step 0 only, finite weights after it.  The status word of
    csrc/lrpost.hip keeps the worst outcome since the plan started, so ``check()`` raises after the whole loop; a new plan and
    the call form start clean."""
    import torch
    D, k, S, T = 301, 28, 32, 6
    rs = np.random.RandomState(8)
    mu0, Sig0, sigsq = _model(rs, D)
    pts = make_linreg_data(3, k, D)
    smp = bc.LinregPosteriorSampler(mu0, Sig0, sigsq, seed=5)
    plan = smp.enqueue_plan(S, pts, T)
    assert plan is not None and plan.factored
    wts = np.abs(rs.randn(k)) * 20.0
    w_dev = torch.from_numpy(wts).cuda()
    w_dev[3] = float("nan")
    theta, _ = plan.draw(w_dev, 0)
    # (the failure happened at step 0: its pivots met the NaN, and its draws are NaN)
    with pytest.raises(bc._native.EngineError):
        plan.check()
    assert np.isnan(theta.cpu().numpy()).any()
    w_dev.copy_(torch.from_numpy(wts))
    for i in range(1, T):
        theta, _ = plan.draw(w_dev, i)
    assert np.isfinite(theta.cpu().numpy()).all()            # (the last step itself succeeded)
    with pytest.raises(bc._native.EngineError):
        plan.check()
    with pytest.raises(bc._native.EngineError):              # (reading does not clear)
        plan.check()
    plan2 = smp.enqueue_plan(S, pts, 2)
    plan2.draw(w_dev, 0)
    plan2.draw(w_dev, 1)
    plan2.check()
    assert np.isfinite(smp(S, wts, pts).cpu().numpy()).all()
    with pytest.raises(bc._native.EngineError):              # (the call form refuses weights that are not finite)
        smp(S, np.where(np.arange(k) == 0, np.nan, wts), pts)


@pytest.mark.parametrize("colsum", ("mfma", "moments"))
@pytest.mark.parametrize("D,k", ((12, 5), (12, 40)))
def test_nan_feature_in_the_coreset_ends_the_loop_with_an_error(bc, colsum, D, k):
    """A coreset point with a NaN feature (rank-k draws for k = 5, the D x D factorisation for k = 40): the reference's
    arithmetic (the oracle with the NumPy sampler) ends with NaN weights -- np.maximum keeps a NaN; both product loops
    (enqueued and host) raise EngineError instead of ending with finite, wrong weights."""
    from oracle.sparsevi_oracle import SparseVIOracle, linreg_loglik
    N, S, T = 3000, 32, 6
    rs = np.random.RandomState(7 * D + k)
    Z = make_linreg_data(21, N, D)
    mu0, Sig0, sigsq = _model(rs, D)
    idcs = np.sort(rs.choice(N, size=k, replace=False)).astype(np.int64)
    Z[idcs[1], 2] = np.nan
    w0 = np.abs(rs.randn(k)) * (N / k)
    np.random.seed(4)
    with np.errstate(invalid="ignore", over="ignore"):
        orc = SparseVIOracle(Z, linreg_sampler(mu0, Sig0, sigsq), lambda z, th: linreg_loglik(z, th, sigsq), S, opt_itrs=T)
        orc.wts, orc.idcs, orc.pts = w0.copy(), idcs.copy(), Z[idcs].copy()
        orc.optimize()
    assert np.isnan(orc.wts).all()
    for enqueue in (True, False):
        smp = bc.LinregPosteriorSampler(mu0, Sig0, sigsq, seed=9)
        alg = bc.SparseVICoreset(Z, bc.DeviceProjector("linreg", smp, S, sigsq=sigsq, colsum=colsum), opt_itrs=T)
        alg.ENQUEUE = enqueue
        alg.wts, alg.idcs, alg.pts = w0.copy(), idcs.copy(), Z[idcs].copy()
        plan = alg._enqueue_plan()
        assert (plan is not None) == enqueue
        if enqueue:
            assert plan.factored == (k == 40)
        with pytest.raises(bc._native.EngineError):
            alg._optimize()


def test_laplace_iteration_limit_at_one_step_is_reported_after_the_loop(bc):
    """Laplace plan with max_iter = 3 (logistic, D = 6): the cold fit of step 0 needs about nine Newton steps and stops at
    the limit, the warm-started fits after it converge.  The worst-status word keeps step 0's failure for ``check()``."""
    import torch
    sys_path_examples()
    import model_lr
    D, k, S, T = 6, 400, 16, 8
    rs = np.random.RandomState(3)
    pts = model_lr.synthetic_rows(k, D, rs)
    wts = np.abs(rs.randn(k)) * 3.0
    smp = bc.LaplacePosteriorSampler("logistic", D, seed=1, max_iter=3)
    plan = smp.enqueue_plan(S, pts, T)
    assert plan is not None
    w_dev = torch.from_numpy(wts).cuda()
    plan.draw(w_dev, 0)
    with pytest.raises(bc._native.EngineError, match="iteration limit"):       # (step 0 did stop at the limit)
        smp.check()
    for i in range(1, T):
        plan.draw(w_dev, i)
    smp.check()                                                                # (the last fit converged)
    with pytest.raises(bc._native.EngineError, match="iteration limit"):
        plan.check()
    plan2 = smp.enqueue_plan(S, pts, 2)                                        # (a new plan starts clean; warm from the mode)
    plan2.draw(w_dev, 1)
    plan2.check()
