"""GPU: BatchPSVI on the device (csrc/psvi.hip, DeviceProjector.project(P, grad=True) / psvi_gradient,
coreset/bpsvi.py) against fixture F17 (the reference's outputs) and against NumPy."""
import ctypes

import numpy as np
import pytest

import bayesiancoresets_amd as bc
from test_bpsvi_host import (LG, LR, golden, linreg_grad, linreg_run_inputs, logistic_grad, logistic_run_inputs,
                             restated_bpsvi)

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


FAM = {"lg": "logistic", "lin": "linreg", "poi": "poisson"}


# ---- 1. project(P, grad=True) on the device against the reference ---------------------------------------------------
@pytest.mark.parametrize("tag", ["lg", "lin", "poi"])
def test_device_grad_projection_matches_reference(tag):
    _torch()
    g = golden()
    P, th = g["proj_%s_P" % tag], g["proj_%s_theta" % tag]
    prj = bc.DeviceProjector(FAM[tag], lambda n, w, p: th, th.shape[0], sigsq=float(g["proj_lin_sigsq"]))
    lls, glls = prj.project(P, grad=True)
    assert lls.is_cuda and glls.is_cuda
    lls, glls = lls.cpu().numpy(), glls.cpu().numpy()
    want_l, want_g = g["proj_%s_lls" % tag], g["proj_%s_glls" % tag]
    assert glls.shape == want_g.shape
    # rtol 1e-12, plus an absolute floor of 1e-12 of the array's largest entry: both sides centre (over the samples, over the
    # coordinates) a sum that was rounded in another order, so an entry near zero keeps an absolute, not a relative, error
    np.testing.assert_allclose(glls, want_g, rtol=1e-12, atol=1e-12 * np.abs(want_g).max())
    np.testing.assert_allclose(lls, want_l, rtol=1e-12, atol=1e-12 * np.abs(want_l).max())


def test_device_grad_projection_host_callbacks_unchanged():
    _torch()
    g = golden()
    P, th = g["proj_lg_P"], g["proj_lg_theta"]
    calls = []

    def gll(z, t):
        calls.append(1)
        return logistic_grad(z, t)
    from lr_workload import log_likelihood
    prj = bc.DeviceProjector("logistic", lambda n, w, p: th, th.shape[0], loglikelihood=log_likelihood, grad_loglikelihood=gll)
    lls, glls = prj.project(P, grad=True)
    assert calls and isinstance(glls, np.ndarray)


# ---- 2. the fused gradient entry against NumPy --------------------------------------------------------------------------
def _fused(torch, fam, P, th, colsum, cv, w, scaling, sigsq):
    from bayesiancoresets_amd import _native
    lib = _native.load()
    dev = torch.device("cuda", 0)
    k, S = cv.shape
    D = th.shape[1]
    dz = D + 1 if fam == 2 else D
    Pd, td = torch.from_numpy(P).to(dev), torch.from_numpy(th).to(dev)
    cd, vd, wd = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (colsum, cv, w))
    out = torch.empty(S + k + k * dz, dtype=torch.float64, device=dev)
    work = torch.empty(int(lib.bcx_psvi_gradient_scratch_bytes(k, S)) // 8, dtype=torch.float64, device=dev)
    st = int(torch.cuda.current_stream(dev).cuda_stream)
    rc = lib.bcx_psvi_gradient(st, fam, Pd.data_ptr(), k, P.shape[1], D, -1 if fam == 0 else D, td.data_ptr(), S, D, sigsq,
                               cd.data_ptr(), vd.data_ptr(), S, wd.data_ptr(), scaling, out.data_ptr(), work.data_ptr())
    assert rc == 0, lib.bcx_project_last_error().decode()
    h = out.cpu().numpy()
    return h[:S], h[S:S + k], h[S + k:].reshape(k, dz)


@pytest.mark.parametrize("fam", [0, 2])
@pytest.mark.parametrize("D", [5, 301])
@pytest.mark.parametrize("S", [40, 256, 1000])
@pytest.mark.parametrize("k", [1, 7, 16, 300, 1024])
def test_fused_gradient_matches_numpy(k, S, D, fam):
    torch = _torch()
    rs = np.random.RandomState(k * 7 + S * 3 + D + fam)
    th = rs.randn(S, D) / np.sqrt(D)
    P = rs.randn(k, D + (fam == 2))
    colsum = rs.randn(S) * 50
    cv = rs.randn(k, S)
    w = rs.rand(k) * 3
    scaling, sigsq = 1.7, 0.6
    resid, wg, ug = _fused(torch, fam, P, th, colsum, cv, w, scaling, sigsq)
    r = scaling * colsum - w.dot(cv)
    tt = np.hstack((th, np.ones((S, 1)))) if fam == 2 else th
    t = P[:, :D].dot(th.T)
    if fam == 0:
        m = -t
        c = np.where(m < 100, np.exp(np.minimum(m, 100)) / (1 + np.exp(np.minimum(m, 100))), 1.0)
    else:
        c = (P[:, D:D + 1] - t) / sigsq
    A = c * r[None, :]
    want_u = -(w[:, None] * (A.dot(tt) - A.dot(tt.mean(axis=1))[:, None])) / S
    if k * S * tt.shape[1] <= 4e6:                 # the reference's own form where the k x S x dz tensor is small
        glls = (logistic_grad(P, th) if fam == 0 else linreg_grad(P, th, sigsq))
        glls = glls - glls.mean(axis=2)[:, :, None]
        want_lit = -(w[:, None, None] * glls * r[None, :, None]).sum(axis=1) / S
        np.testing.assert_allclose(want_u, want_lit, rtol=1e-9, atol=1e-12 * np.abs(want_lit).max())
    tol = lambda a: dict(rtol=1e-10, atol=1e-12 * np.abs(a).max())   # (entries near zero: an absolute floor)
    np.testing.assert_allclose(resid, r, **tol(r))
    np.testing.assert_allclose(wg, -cv.dot(r) / S, **tol(wg))
    np.testing.assert_allclose(ug, want_u, **tol(want_u))
    resid2, wg2, ug2 = _fused(torch, fam, P, th, colsum, cv, w, scaling, sigsq)
    assert np.array_equal(resid, resid2) and np.array_equal(wg, wg2) and np.array_equal(ug, ug2)


# ---- 2b. the fused gradient at its edges: Poisson, strided layouts with NaN padding, branch thresholds, the size limits -----
def _coef(fam, t, y, sigsq):
    """c(i, s) of every family in NumPy, branch by branch as the reference writes it (model_lr.py:52-56; model_poiss.py:25-29
    compute_s and :58-66 grad_z_log_likelihood; model_linreg.py:17)."""
    if fam == 0:
        m = -t
        with np.errstate(over="ignore"):
            e = np.exp(np.where(m < 100, m, 0.0))
        return np.where(m < 100, e / (1 + e), 1.0)
    if fam == 1:
        s = t.copy()
        big = s > -100
        s[big] = np.log(np.maximum(s[big], 0) + np.log1p(np.exp(-np.fabs(s[big]))))
        es = np.exp(s)
        g = y - es
        hi = es > 1e-15
        g[hi] = (y[hi] * np.exp(-s[hi]) - 1.0) * (1.0 - np.exp(-es[hi]))
        return g
    return (y - t) / sigsq


def _fused_strided(torch, fam, P, D, ycol, th, ldt, colsum, cv, ldcv, w, scaling, sigsq):
    """bcx_psvi_gradient with P (k x ldp), theta (S x ldt) and corevecs (k x ldcv) as given, every element outside
    the logical (k x cols, S x D, k x S) blocks set to NaN: a read of padding shows up in the output."""
    from bayesiancoresets_amd import _native
    lib = _native.load()
    dev = torch.device("cuda", 0)
    k, S = cv.shape
    dz = D + 1 if fam == 2 else D
    thp = np.full((S, ldt), np.nan)
    thp[:, :D] = th
    cvp = np.full((k, ldcv), np.nan)
    cvp[:, :S] = cv
    Pd, td, cd, vd, wd = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (P, thp, colsum, cvp, w))
    out = torch.full((S + k + k * dz + 8,), float("nan"), dtype=torch.float64, device=dev)
    work = torch.full((int(lib.bcx_psvi_gradient_scratch_bytes(k, S)) // 8,), float("nan"), dtype=torch.float64, device=dev)
    st = int(torch.cuda.current_stream(dev).cuda_stream)
    rc = lib.bcx_psvi_gradient(st, fam, Pd.data_ptr(), k, P.shape[1], D, ycol, td.data_ptr(), S, ldt, sigsq,
                               cd.data_ptr(), vd.data_ptr(), ldcv, wd.data_ptr(), scaling, out.data_ptr(), work.data_ptr())
    assert rc == 0, lib.bcx_project_last_error().decode()
    h = out.cpu().numpy()
    assert np.isnan(h[S + k + k * dz:]).all()                  # (nothing written past the output)
    return h[:S], h[S:S + k], h[S + k:S + k + k * dz].reshape(k, dz)


def _want(fam, P, D, ycol, th, colsum, cv, w, scaling, sigsq):
    """The NumPy fp64 product form of resid / wgrad / ugrad (the one test_fused_gradient_matches_numpy checks against the
    reference's k x S x dz form where that is small)."""
    k, S = cv.shape
    r = scaling * colsum - w.dot(cv)
    tt = np.hstack((th, np.ones((S, 1)))) if fam == 2 else th
    t = P[:, :D].dot(th.T)
    y = np.zeros_like(t) if fam == 0 else np.repeat(P[:, ycol:ycol + 1], S, axis=1)
    A = _coef(fam, t, y, sigsq) * r[None, :]
    return r, -cv.dot(r) / S, -(w[:, None] * (A.dot(tt) - A.dot(tt.mean(axis=1))[:, None])) / S


def _check_fused(got, want, rtol=1e-10):
    for g, wv in zip(got, want):
        assert np.isfinite(g).all()
        np.testing.assert_allclose(g, wv, rtol=rtol, atol=1e-12 * np.abs(wv).max())


@pytest.mark.parametrize("fam", [0, 1, 2])
@pytest.mark.parametrize("k,S,D", [(7, 40, 5), (33, 256, 301), (300, 1000, 64)])
@pytest.mark.parametrize("layout", ["samplers", "wide"])
def test_fused_gradient_strided_layouts(k, S, D, fam, layout):
    """Family 1 (Poisson, with Poisson-count responses) beside 0 and 2, and the layouts the product passes: ldt = D + D % 2
    (the samplers' draws) or wider, ldp > cols, ldcv > S, every padding element NaN."""
    torch = _torch()
    rs = np.random.RandomState(k + 5 * S + 11 * D + 101 * fam)
    cols = D + (fam != 0)
    ldp = cols + (3 if layout == "wide" else 1)
    ldt = D + D % 2 if layout == "samplers" else D + 5
    ldcv = S + (1 if layout == "samplers" else 17)
    th = rs.randn(S, D) / np.sqrt(D)
    P = np.full((k, ldp), np.nan)
    P[:, :D] = rs.randn(k, D)
    if fam == 1:
        P[:, D] = rs.poisson(3.0, size=k)
    elif fam == 2:
        P[:, D] = rs.randn(k)
    ycol = -1 if fam == 0 else D
    colsum, cv, w = rs.randn(S) * 50, rs.randn(k, S), rs.rand(k) * 3
    got = _fused_strided(torch, fam, P, D, ycol, th, ldt, colsum, cv, ldcv, w, 1.3, 0.6)
    _check_fused(got, _want(fam, P, D, ycol, th, colsum, cv, w, 1.3, 0.6))


def test_fused_gradient_at_the_branch_thresholds():
    """x . theta placed exactly (one non-zero feature, products exact in fp64) on both sides of every branch of the
    coefficient: logistic m = -t at 100, Poisson t at -100 and e^s at 1e-15 (t near log(1e-15): softplus(t) = e^t there)."""
    torch = _torch()
    D, S = 4, 64
    e15 = np.log(1e-15)
    ts = {0: [-100.0, -100.0 + 2 ** -40, -100.0 - 2 ** -40, -99.0, -101.0, -150.0, 30.0, 0.0],
          1: [-100.0, -100.0 + 2 ** -40, -100.0 - 2 ** -40, -99.5, -100.5, e15, e15 * (1 + 1e-12), e15 * (1 - 1e-12), e15 - 0.5, e15 + 0.5,
              -700.0, 0.0, 40.0]}
    rs = np.random.RandomState(12)
    for fam, tv in ts.items():
        k = len(tv)
        P = np.zeros((k, D + 1))
        P[:, 0] = tv                                            # x = (t, 0, 0, 0): t = x . theta_s for theta_s[0] = 1
        P[:, D] = rs.poisson(2.0, size=k)
        th = np.zeros((S, D))
        th[:, 0] = 1.0
        th[1:, 1:] = rs.randn(S - 1, D - 1)                     # (zero features: no contribution to t, but to the gradient)
        th[S // 2:, 0] = rs.choice([0.5, 2.0, 1.0 + 2 ** -20], size=S - S // 2)   # (exact products, t / 2, 2 t, ...)
        colsum, cv, w = rs.randn(S) * 10, rs.randn(k, S), rs.rand(k) + 0.5
        ycol = -1 if fam == 0 else D
        got = _fused_strided(torch, fam, P, D, ycol, th, D + D % 2, colsum, cv, S, w, 1.0, 1.0)
        _check_fused(got, _want(fam, P, D, ycol, th, colsum, cv, w, 1.0, 1.0))


@pytest.mark.parametrize("fam", [0, 1])
def test_fused_gradient_at_the_size_limits(fam):
    """k = 4096 pseudo-points, S = 8192 samples, D = 1024 features (BCX_PSVI_MAX_*) against the NumPy fp64 product form."""
    torch = _torch()
    k, S, D = 4096, 8192, 1024
    rs = np.random.RandomState(5 + fam)
    th = rs.randn(S, D) / np.sqrt(D)
    P = np.empty((k, D + 2))
    P[:, :D] = rs.randn(k, D)
    P[:, D] = rs.poisson(2.0, size=k)
    P[:, D + 1] = np.nan
    colsum, cv, w = rs.randn(S) * 50, rs.randn(k, S), rs.rand(k) * 3
    ycol = -1 if fam == 0 else D
    got = _fused_strided(torch, fam, P, D, ycol, th, D, colsum, cv, S, w, 1.1, 1.0)
    _check_fused(got, _want(fam, P, D, ycol, th, colsum, cv, w, 1.1, 1.0))


def test_limits_return_errors():
    torch = _torch()
    from bayesiancoresets_amd import _native
    lib = _native.load()
    buf = torch.zeros(64, dtype=torch.float64, device="cuda")
    p = buf.data_ptr()
    assert lib.bcx_psvi_gradient_scratch_bytes(4097, 10) == -1
    assert lib.bcx_psvi_gradient_scratch_bytes(10, 8193) == -1
    for k, S, D in ((4097, 8, 4), (0, 8, 4), (4, 8193, 4), (4, 8, 1025), (4, 8, 0)):
        rc = lib.bcx_psvi_gradient(None, 0, p, k, max(D, 1), D, -1, p, S, max(D, 1), 1.0, p, p, S, p, 1.0, p, p)
        assert rc == _native.ERR_ARG and lib.bcx_project_last_error()
        rc = lib.bcx_project_grad_points(None, 2, p, k, max(D, 1) + 1, D, D, p, S, max(D, 1), 1.0, p, p)
        assert rc == _native.ERR_ARG
    assert lib.bcx_project_grad_points(None, 7, p, 2, 4, 3, 3, p, 4, 3, 1.0, p, p) == _native.ERR_ARG


# ---- 3. BatchPSVICoreset against the reference's trajectories ------------------------------------------------------------
@pytest.mark.parametrize("colsum", ["mfma", "moments"])
@pytest.mark.parametrize("tag,nsub", [("full", None), ("sub", 500)])
def test_bpsvi_linreg_matches_reference(tag, nsub, colsum):
    _torch()
    g = golden()
    Z, smp, _, _ = linreg_run_inputs()
    np.random.seed(LR["np_seed"])
    prj = bc.DeviceProjector("linreg", smp, LR["S"], sigsq=LR["sigsq"], colsum=colsum)
    alg = bc.BatchPSVICoreset(Z, prj, LR["itrs"], n_subsample_opt=nsub, step_sched=LR["sched"])
    alg.build(LR["k"])
    np.testing.assert_allclose(alg.wts, g["lr_%s_wts" % tag], rtol=1e-7)
    np.testing.assert_allclose(alg.pts, g["lr_%s_pts" % tag], rtol=1e-6, atol=1e-8)
    if colsum == "moments" and nsub is None:
        assert prj.moments_info.get("rows") == LR["N"]          # the closed form served the standing data set
    wts, pts, idcs = alg.get()
    assert idcs.dtype == np.float64 and np.all(idcs == -1.0)
    assert isinstance(wts, np.ndarray) and isinstance(pts, np.ndarray)


def test_bpsvi_logistic_matches_reference():
    _torch()
    g = golden()
    Z, smp, _, _ = logistic_run_inputs()
    np.random.seed(LG["np_seed"])
    prj = bc.DeviceProjector("logistic", smp, LG["S"])
    alg = bc.BatchPSVICoreset(Z, prj, LG["itrs"], step_sched=LG["sched"])
    alg.build(LG["k"])
    np.testing.assert_allclose(alg.wts, g["lg_full_wts"], rtol=1e-7)
    np.testing.assert_allclose(alg.pts, g["lg_full_pts"], rtol=1e-6, atol=1e-8)


def test_bpsvi_device_tensor_data():
    torch = _torch()
    g = golden()
    Z, smp, _, _ = linreg_run_inputs()
    np.random.seed(LR["np_seed"])
    prj = bc.DeviceProjector("linreg", smp, LR["S"], sigsq=LR["sigsq"])
    alg = bc.BatchPSVICoreset(torch.from_numpy(Z).cuda(), prj, LR["itrs"], n_subsample_opt=500, step_sched=LR["sched"])
    alg.build(LR["k"])
    assert isinstance(alg.pts, np.ndarray)
    np.testing.assert_allclose(alg.wts, g["lr_sub_wts"], rtol=1e-7)
    np.testing.assert_allclose(alg.pts, g["lr_sub_pts"], rtol=1e-6, atol=1e-8)


# ---- 4. device samplers: their draws replayed into the host restatement ----------------------------------------------------
class _Recorder(object):
    def __init__(self, inner):
        self.inner, self.draws = inner, []

    def __call__(self, n, wts, pts):
        th = self.inner(n, wts, pts)
        self.draws.append(th.detach().cpu().numpy().copy() if hasattr(th, "detach") else np.array(th))
        return th


class _Replay(object):
    def __init__(self, draws):
        self.draws, self.i = draws, 0

    def __call__(self, n, wts, pts):
        th = self.draws[self.i]
        self.i += 1
        return th


@pytest.mark.parametrize("family", ["linreg", "logistic"])
def test_bpsvi_device_samplers_replayed(family):
    _torch()
    from lr_workload import log_likelihood as lg_ll
    from models import linreg_log_likelihood, make_linreg_data
    from bpsvi_models import make_logistic_data
    N, D, S, k, T, sigsq = 200000, 30, 128, 50, 20, 1.0
    if family == "linreg":
        Z = make_linreg_data(31, N, D)
        rec = _Recorder(bc.LinregPosteriorSampler(np.zeros(D), np.eye(D), sigsq, seed=5))
        ll, gll = (lambda z, t: linreg_log_likelihood(z, t, sigsq)), (lambda z, t: linreg_grad(z, t, sigsq))
    else:
        Z = make_logistic_data(31, N, D)
        rec = _Recorder(bc.LaplacePosteriorSampler("logistic", D, seed=5))
        ll, gll = lg_ll, logistic_grad
    sched = lambda i: 0.2 / (1.0 + i)
    np.random.seed(3)
    prj = bc.DeviceProjector(family, rec, S, sigsq=sigsq)
    alg = bc.BatchPSVICoreset(Z, prj, T, step_sched=sched)
    alg.build(k)
    assert len(rec.draws) == T + 1
    np.random.seed(3)
    w, P = restated_bpsvi(Z, _Replay(rec.draws), S, ll, gll, k, T, None, sched)
    np.testing.assert_allclose(alg.wts, w, rtol=1e-7)
    np.testing.assert_allclose(alg.pts, P, rtol=1e-6, atol=1e-8)


# ---- 5. behaviour ----------------------------------------------------------------------------------------------------------
def test_bpsvi_behaviour():
    _torch()
    Z, smp, _, _ = linreg_run_inputs()
    np.random.seed(1)
    prj = bc.DeviceProjector("linreg", smp, LR["S"], sigsq=LR["sigsq"])
    alg = bc.BatchPSVICoreset(Z, prj, 5)
    with pytest.raises(ValueError):
        alg.build(Z.shape[0] + 1)                     # np.random.choice without replacement
    alg.build(4)
    w1, p1 = alg.wts.copy(), alg.pts.copy()
    alg.build(4)                                      # starts again from a new random initialisation
    assert alg.wts.shape == (4,) and not np.array_equal(alg.pts, p1)
    w2, p2 = alg.wts.copy(), alg.pts.copy()
    alg.optimize()                                    # error() is 0: the run continues, nothing is reverted
    assert alg.error() == 0.0 and not alg.reached_numeric_limit
    assert not np.array_equal(alg.pts, p2)
    wts, pts, idcs = alg.get()
    assert idcs.dtype == np.float64 and np.all(idcs == -1.0) and pts.shape[1] == Z.shape[1]
    del w1, w2


def test_bpsvi_poisson_raises():
    _torch()
    Z = np.hstack((np.random.RandomState(0).randn(100, 3), np.ones((100, 1))))
    prj = bc.DeviceProjector("poisson", lambda n, w, p: np.zeros((n, 3)), 8)
    alg = bc.BatchPSVICoreset(Z, prj, 5)
    state = np.random.get_state()[1].copy()
    with pytest.raises(ValueError):
        alg.build(3)
    assert np.array_equal(np.random.get_state()[1], state)      # raised before any draw
