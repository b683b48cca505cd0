"""GPU: csrc/lik_point.h::lap_point -- ll, g, h of a point in its linear predictor -- against the long-double referee
(tests/lik_point_referee.py, itself held to 60 digits by tests/test_lik_point_referee_host.py), at the edges of its range.

* ll and g through ``bcx_log_joint_grad``: one row, D = 1, x = s, theta = 1, so that the prior adds exactly 0.5 and the outputs
  are the terms themselves;
* h through ONE Newton step of ``bcx_laplace_sampler`` and ``bcx_laplace_sampler_stream`` from a start where the gradient
  vanishes (tests/lik_point_cases.py::h_probe): the draw of unit noise returns W = (1 - sum_j w_j h_j x_j^2)^(-1/2);
* a whole fit from a warm start whose predictors lie where the Poisson h used to be 0 / 0;
* NaN in a feature, a parameter or a weight.

The bar is 16 x 2^-53 of every term's scale (Poisson: y (1 + |log rate|) + rate for ll, 1 + y for g and h; logistic: |ll|, 1,
1); the ratios an MI355X gives are printed by the tests and recorded in DESIGN.md 4.23."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lik_point_cases as cases  # noqa: E402
import lik_point_referee as ref  # noqa: E402

pytestmark = pytest.mark.gpu
LD = np.longdouble
U = ref.U
FAM = {"logistic": 0, "poisson": 1}


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def bc(torch):
    import bayesiancoresets_amd as bc
    return bc


@pytest.fixture(scope="module")
def lib(bc):
    from bayesiancoresets_amd import _native
    return _native.load()


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


# ---------------------------------------------------------------------------------------------------------------- ll and g
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_ll_and_g_at_the_edges(torch, lib, family):
    """value = w (ll(s) - log y!) - 0.5 - log(2 pi) / 2 and grad = w g(s) s - 1 of a single row [s, y] at theta = 1.  Per output:
    16 U of the term's scale times |w| (value) or |w s| (gradient), and 4 ulp of every other addend."""
    P = cases.device_predictors(family)
    ys = (0.0,) if family == "logistic" else cases.Y_VALUES
    s = np.repeat(P, len(ys))
    y = np.tile(np.array(ys), P.size)
    w = np.tile(np.array([1.0, 1.0, 0.375, 3.0]), (s.size + 3) // 4)[:s.size]
    M = s.size
    assert P.size >= 400
    ldz = 2 if family == "poisson" else 1
    Z = _dev(torch, np.stack((s, y), axis=1) if family == "poisson" else s[:, None])
    wd, th = _dev(torch, w), _dev(torch, [1.0])
    val = torch.full((M,), 7.25, dtype=torch.float64, device="cuda")
    grad = torch.full((M,), 7.25, dtype=torch.float64, device="cuda")
    work = torch.zeros(max(int(lib.bcx_log_joint_grad_scratch_bytes(1, 1, 1)), 8) // 8, dtype=torch.float64, device="cuda")
    st = int(torch.cuda.current_stream().cuda_stream)
    for i in range(M):
        rc = lib.bcx_log_joint_grad(st, FAM[family], Z.data_ptr() + 8 * ldz * i, 1, ldz, 1, wd.data_ptr() + 8 * i, th.data_ptr(), 1, 1,
                                    val.data_ptr() + 8 * i, grad.data_ptr() + 8 * i, work.data_ptr())
        assert rc == 0
    val, grad = val.cpu().numpy(), grad.cpu().numpy()
    ll, g, _ = ref.point_terms(family, s, y, with_h=False)
    sl, sg, _ = ref.scales(family, s, y)
    lf = ref.log_factorial(y) if family == "poisson" else np.zeros(M, dtype=LD)
    wl, half_log = w.astype(LD), ref.LOG_2PI / 2
    ref_v = wl * (ll - lf) - LD(0.5) - half_log
    ref_g = wl * g * s.astype(LD) - 1
    others_v = 4 * (np.spacing((wl * lf).astype(np.float64)) * (lf != 0) + np.spacing(0.5) + np.spacing(float(half_log)))
    others_g = 4 * np.spacing(1.0)
    assert np.all(np.isfinite(val)) and np.all(np.isfinite(grad))
    ev = np.maximum(np.abs(val.astype(LD) - ref_v) - others_v, 0) / (U * sl * np.abs(wl))
    with np.errstate(invalid="ignore", divide="ignore"):
        eg = np.maximum(np.abs(grad.astype(LD) - ref_g) - others_g, 0) / (U * sg * np.abs(wl * s))
    eg = np.where(s == 0, np.where(grad == -1.0, 0, np.inf), eg)           # (x = 0: the gradient is -theta, exactly)
    iv, ig = int(np.argmax(ev)), int(np.argmax(eg))
    print("%s: worst error in units of 2^-53 x scale over %d (s, y, w): ll %.2f (s = %r, y = %g), g %.2f (s = %r, y = %g); bar 16"
          % (family, M, float(ev[iv]), s[iv], y[iv], float(eg[ig]), s[ig], y[ig]))
    assert float(ev[iv]) <= 16.0, (s[iv], y[iv], w[iv], val[iv], ref_v[iv])
    assert float(eg[ig]) <= 16.0, (s[ig], y[ig], w[ig], grad[ig], ref_g[ig])


# ----------------------------------------------------------------------------------------------------------------------- h
def _one_newton_step(torch, bc, family, probes, streamed):
    """[(case, status, theta1, W)] of one Newton step per probe from its start: warm = 1, max_iter = 1, a tolerance no step
    exceeds.  The draw of noise 2^20 is theta1 + 2^20 W (W read back to 2^-53 of itself next to theta1 = 1)."""
    smp = bc.LaplacePosteriorSampler(family, 1, tol=1e300, max_iter=1, stream=streamed)
    smp._dev_force_stream = streamed
    assert smp._streams(2) == streamed
    big = 2.0 ** 20
    R, rbar = _dev(torch, [[big, 0.0]]), _dev(torch, [0.0, 0.0])
    theta = torch.zeros(1, smp.ld, dtype=torch.float64, device="cuda")
    work = smp._stream_work(2) if streamed else None
    out = []
    for c in probes:
        pts, wd = _dev(torch, c["Z"]), _dev(torch, c["w"])
        smp._mu.fill_(c["t0"])
        rc = smp._fn(work)(*smp._args(2, wd, pts, True, R, rbar, theta, work))
        assert rc == 0
        status = int(smp._status.cpu().numpy()[0])
        th1 = float(smp._mu.cpu().numpy()[0])
        out.append((c, status, th1, (float(theta.cpu().numpy()[0, 0]) - th1) / big))
    return out


@pytest.mark.parametrize("streamed", (False, True))
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_h_through_one_newton_step(torch, bc, family, streamed):
    """Every probe: status 0, a finite W within what moving the Newton-matrix entry by 16 U sum_j (1 + y_j) w_j x_j^2 (logistic:
    16 U sum_j w_j x_j^2) allows, and 8 ulp of W for the square root, the reciprocal and the read-back.  In the band
    -745 < s0 < -355 the first point's weight is 1, W = 1 to 1e-150, and the bound is |W - 1| <= 8 U (1 + y) s0^2."""
    probes = [cases.h_probe(family, s0, y) for s0, y in cases.h_probe_cases(family)]
    res = _one_newton_step(torch, bc, family, probes, streamed)
    worst, at, bad = 0.0, None, []
    for c, status, th1, W in res:
        ok = status == 0 and np.isfinite(W) and np.isfinite(th1) and abs(th1 - c["t0"]) <= 4 * cases.STEP_MARGIN
        if ok:
            want, lo, hi = cases.h_probe_expected(c, th1)
            slack = 8 * np.spacing(float(want))
            ok = float(lo) - slack <= W <= float(hi) + slack
            H, Hd = 1 / (want * want), 1 / (LD(W) * LD(W))
            ratio = float(abs(Hd - H) / ((1 / (lo * lo) - H) / 16))
            if ratio > worst:
                worst, at = ratio, (c["s0"], c["y"])
        if not ok:
            bad.append((c["s0"], c["y"], status, th1, W))
    print("%s %s: h in the Newton matrix, worst error in units of 2^-53 sum (scale_h w x^2) over %d probes: %.2f at (s0, y) = %r; bar 16"
          % (family, "streamed" if streamed else "LDS", len(res), worst, at))
    assert not bad, "%d of %d probes (s0, y, status, theta1, W), the first ones: %r" % (len(bad), len(res), bad[:6])


# --------------------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("streamed", (False, True))
def test_fit_from_a_warm_start_in_the_band(torch, bc, streamed):
    """Poisson, D = 2, k = 6, from a warm start at which two predictors lie in (-745, -373) and one in (-372, -356); against the
    referee's fit (which converges in 8 steps: tests/test_lik_point_referee_host.py) at the tolerances of
    tests/test_gpu_svi.py::test_laplace_sampler_against_the_host_fit."""
    Z, w, th0 = cases.end_to_end_case()
    D = 2
    smp = bc.LaplacePosteriorSampler("poisson", D, stream=streamed)
    smp._dev_force_stream = streamed
    assert smp._streams(6) == streamed and smp.max_iter == 100
    R = np.zeros((D + 1, smp.ld))
    R[:D, :D] = np.eye(D)
    Rd, rbar = _dev(torch, R), _dev(torch, np.zeros(smp.ld))
    theta = torch.zeros(D + 1, smp.ld, dtype=torch.float64, device="cuda")
    work = smp._stream_work(6) if streamed else None
    smp._mu.copy_(_dev(torch, th0))
    rc = smp._fn(work)(*smp._args(6, _dev(torch, w), _dev(torch, Z), True, Rd, rbar, theta, work))
    assert rc == 0
    status = smp._status.cpu().numpy()
    th = theta.cpu().numpy()[:, :D]
    mu, W = th[D], th[:D] - th[D]
    mu_ref, H_ref, steps_ref, ok = ref.laplace_fit("poisson", Z, w, th0)
    assert ok
    cov_ref = ref.inverse(H_ref).astype(np.float64)
    print("%s: status %d after %d Newton steps (the referee: %d), |mu - referee| max %.3e"
          % ("streamed" if streamed else "LDS", status[0], status[1], steps_ref, np.abs(mu - mu_ref.astype(np.float64)).max()))
    assert status[0] == 0
    np.testing.assert_allclose(mu, mu_ref.astype(np.float64), rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(W.T.dot(W), cov_ref, rtol=1e-6, atol=1e-9 * np.abs(cov_ref).max())
    assert np.all(np.triu(W, 1) == 0.0)
    np.testing.assert_array_equal(smp._mu.cpu().numpy(), mu)


# ------------------------------------------------------------------------------------------------------ non-finite inputs
def _nan_case(family):
    rs = np.random.RandomState(41)
    N, D, C = 200, 3, 10                                  # two workgroups of rows, two groups of columns
    X = rs.randn(N, D)
    Z = np.hstack((X, rs.poisson(2.0, N)[:, None].astype(np.float64))) if family == "poisson" else X
    return Z, rs.uniform(0.5, 2.0, N), 0.7 * rs.randn(C, D)


@pytest.mark.parametrize("where", ("feature", "theta", "weight"))
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_nan_reaches_the_value_and_every_gradient_coordinate(bc, family, where):
    """As NumPy's evaluation of the reference's formula (model_lr.py:59-64, model_poiss.py:69-74): a NaN predictor or weight
    makes the value and EVERY coordinate of the gradient of its columns NaN.  Columns it does not touch keep their bits."""
    Z, w, th = _nan_case(family)
    C = th.shape[0]
    v0, g0 = bc.log_joint_grad(family, Z, w, th)
    assert np.all(np.isfinite(v0)) and np.all(np.isfinite(g0))
    Zb, wb, thb = Z.copy(), w.copy(), th.copy()
    if where == "feature":
        Zb[137, 1] = np.nan
        hit = np.ones(C, dtype=bool)
    elif where == "weight":
        wb[137] = np.nan
        hit = np.ones(C, dtype=bool)
    else:
        thb[4, 1] = np.nan
        hit = np.arange(C) == 4
    v, g = bc.log_joint_grad(family, Zb, wb, thb)
    assert np.all(np.isnan(v[hit])), v
    assert np.all(np.isnan(g[hit])), g[hit]
    assert np.array_equal(v[~hit], v0[~hit]) and np.array_equal(g[~hit], g0[~hit])
    if where == "theta":                                  # ... and the bits of a call without the bad column
        v9, g9 = bc.log_joint_grad(family, Z, w, np.delete(th, 4, axis=0))
        assert np.array_equal(v[~hit], v9) and np.array_equal(g[~hit], g9)
