"""GPU: the streamed Laplace fit-and-draw (csrc/laplace_stream.hip; ``bc.LaplacePosteriorSampler(..., stream=True)``,
``bc.DeviceHMC(..., device_frame=True)``): the points stay in device memory and are streamed by many workgroups, beyond what one
workgroup's LDS holds.

* against the package's host ``laplace_fit`` (examples/common/model_lr.py / model_poiss.py) with the tolerances
  tests/test_gpu_svi.py::test_laplace_sampler_against_the_host_fit holds the LDS kernel to;
* against the LDS kernel where both apply, bit-reproducibility, device-tensor input without a copy to the host, the plans of
  SparseVI / BatchPSVI, failures that stick, and the HMC frame."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(1, os.path.join(ROOT, "bayesian-coresets_amd", "examples", "common"))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bc():
    import bayesiancoresets_amd as bc
    return bc


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _laplace_case(family, D, k, seed):
    """tests/test_gpu_svi.py::_laplace_case."""
    import model_lr
    import model_poiss
    rs = np.random.RandomState(seed)
    if family == "logistic":
        pts = model_lr.synthetic_rows(max(k, 1), D, rs)[:k]
        fit = model_lr.laplace_fit
    else:
        pts = model_poiss.synthetic_rows(max(k, 1), D, rs)[:k]
        fit = model_poiss.laplace_fit
    wts = np.abs(rs.randn(k)) * 3.0
    if k > 3:
        wts[1] = 0.0
    return pts, wts, fit


def _check_fit(mu, W, mu_ref, cov_ref):
    """The tolerances of test_laplace_sampler_against_the_host_fit."""
    np.testing.assert_allclose(mu, mu_ref, rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(W.T.dot(W), cov_ref, rtol=1e-6, atol=1e-9 * np.abs(cov_ref).max())
    assert np.all(np.triu(W, 1) == 0.0)


def _reference(fit, pts, wts, D):
    if len(wts) and (wts > 0).any():
        return fit(pts[wts > 0], wts[wts > 0])
    return np.zeros(D), np.eye(D)


_CASES = (
    ("logistic", 32, 333, False, None),      # the first size past the LDS limit (k = 332 at D = 32)
    ("poisson", 6, 3000, False, None),       # the shape a default sampler declines
    ("logistic", 10, 1, True, None),         # tile edges, forced stream: one row,
    ("logistic", 10, 127, True, None),       # one short tile,
    ("poisson", 5, 128, True, None),         # one full tile,
    ("logistic", 10, 129, True, None),       # a one-row tail tile,
    ("poisson", 5, 257, True, None),         # three workgroups, the last with one row
    ("logistic", 1, 200, True, None),        # padding of the 32 x 32 Newton matrix: D = 1
    ("poisson", 31, 400, True, None),        # ... and D = 31 (an even LDS row, one identity row)
    ("poisson", 5, 257, True, "wide"),       # a view of rows two columns wider than the model's
    ("logistic", 10, 129, True, "negative"),  # a zero and a negative weight
    ("logistic", 7, 0, True, None),          # no points: the prior
)


@pytest.mark.parametrize("family,D,k,force,variant", _CASES)
def test_stream_against_the_host_fit(bc, torch, family, D, k, force, variant):
    """Every case was run through a NumPy statement of the kernel's iteration (batches of four step lengths, lambda I on a failed
    Cholesky) before it was relied on: all converge in 4 - 10 Newton steps (60 allowed) to the host fit's mode within 1e-9, so
    none had to be replaced."""
    pts, wts, fit = _laplace_case(family, D, k, 50 * D + k)
    if variant == "negative":
        wts[2] = -1.5
    smp = bc.LaplacePosteriorSampler(family, D, seed=4, stream=True)
    smp._dev_force_stream = force
    assert smp.supports(8, k) and smp._streams(k)
    if variant == "wide":
        cols = pts.shape[1]
        wide = torch.full((k, cols + 2), float("nan"), dtype=torch.float64, device="cuda")       # (the padding must not be read)
        wide[:, :cols] = torch.from_numpy(pts).cuda()
        view = wide[:, :cols]
        assert view.stride(0) == cols + 2
        mu, W = smp.posterior(wts, view)
    else:
        mu, W = smp.posterior(wts if k else None, pts if k else None)
    mu_ref, cov_ref = _reference(fit, pts, np.maximum(wts, 0.0), D)
    print("%s D=%d k=%d %s: %d Newton steps, |mu - ref| max %.3e" % (family, D, k, variant, smp.newton_steps, np.abs(mu - mu_ref).max()))
    _check_fit(mu, W, mu_ref, cov_ref)
    assert smp.newton_steps <= 60
    if variant is None:
        n = 64
        th = smp(n, wts if k else None, pts if k else None)
        assert tuple(th.shape) == (n, D) and th.stride(0) == D + D % 2 and th.data_ptr() % 16 == 0
        t = th.cpu().numpy()
        assert np.all(np.isfinite(t))
        np.testing.assert_allclose(smp.mean.cpu().numpy(), t.mean(axis=0), rtol=1e-10, atol=1e-12)


def _probe_noise(torch, D, S, seed):
    """Rows of noise that return the factor (unit vectors), the mode (a zero row) and draws (normal rows; the padding column
    holds noise that must not matter)."""
    ld = D + D % 2
    R = np.zeros((S, ld))
    R[:D, :D] = np.eye(D)
    R[D + 1:] = np.random.RandomState(seed).randn(S - D - 1, ld)
    return R, torch.from_numpy(R).cuda()


@pytest.mark.parametrize("family,D,k", (("logistic", 10, 40), ("poisson", 5, 200)))
def test_forced_stream_against_the_lds_kernel(bc, torch, family, D, k):
    pts, wts, fit = _laplace_case(family, D, k, 50 * D + k)
    S = D + 20
    R, Rd = _probe_noise(torch, D, S, 3)
    out = {}
    for force in (False, True):
        smp = bc.LaplacePosteriorSampler(family, D, seed=4, stream=True)
        smp._dev_force_stream = force
        assert smp._streams(k) == force
        smp._noise = lambda n: Rd
        th = smp(S, wts, pts).cpu().numpy().copy()
        mu = th[D]
        W = th[:D] - mu
        want = mu + R[:, :D].dot(W)
        assert np.abs(th - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
        out[force] = (mu, W)
    mu_ref, cov_ref = _reference(fit, pts, wts, D)
    for force in (False, True):
        _check_fit(out[force][0], out[force][1], mu_ref, cov_ref)
    _check_fit(out[True][0], out[True][1], out[False][0], out[False][1].T.dot(out[False][1]))


def test_bit_reproducible(bc, torch):
    family, D, k, S = "poisson", 6, 3000, 40
    pts, wts, _ = _laplace_case(family, D, k, 50 * D + k)
    _, Rd = _probe_noise(torch, D, S, 5)
    got = []
    for _ in range(2):
        smp = bc.LaplacePosteriorSampler(family, D, seed=4, stream=True)
        smp._noise = lambda n: Rd
        th = smp(S, wts, pts)
        got.append([t.cpu().numpy().tobytes() for t in (smp._mu, th.contiguous(), smp._tbar)])
    assert got[0] == got[1]


@pytest.mark.parametrize("family", ("logistic", "poisson"))
def test_device_tensor_input_is_used_in_place(bc, torch, family):
    N, D = 20000, 10
    pts, _, fit = _laplace_case(family, D, N, 7)
    Z = torch.from_numpy(pts).cuda()

    def no_copy(*a, **k):
        raise AssertionError("the points were brought to the host")
    for name in ("cpu", "numpy", "tolist", "__array__"):
        setattr(Z, name, no_copy)
    smp = bc.LaplacePosteriorSampler(family, D, seed=4, stream=True)
    ptr = Z.data_ptr()
    mu, W = smp.posterior(None, Z)
    assert Z.data_ptr() == ptr
    mu_ref, cov_ref = fit(pts, None)
    _check_fit(mu, W, mu_ref, cov_ref)
    # a default sampler takes the tensor too, where the LDS kernel applies
    small = torch.from_numpy(pts[:50]).cuda()
    mu_s, W_s = bc.LaplacePosteriorSampler(family, D, seed=4).posterior(None, small)
    _check_fit(mu_s, W_s, *fit(pts[:50], None))


def test_enqueue_plan_against_the_call_form(bc, torch):
    """Three draws from device-resident weights that change between the draws; every draw after the first starts at the mode of
    the one before, the call form at zero."""
    family, D, k, steps = "logistic", 32, 340, 3
    pts, wts, _ = _laplace_case(family, D, k, 50 * D + k)
    S = D + 8
    R, Rd = _probe_noise(torch, D, S, 9)
    block = Rd.unsqueeze(0).repeat(steps, 1, 1).contiguous()
    smp = bc.LaplacePosteriorSampler(family, D, seed=4, stream=True)
    smp._noise_block = lambda st, n: block
    plan = smp.enqueue_plan(S, pts, steps)
    assert plan is not None and plan.work is not None
    call = bc.LaplacePosteriorSampler(family, D, seed=4, stream=True)
    call._noise = lambda n: Rd
    rs = np.random.RandomState(2)
    w_dev = torch.from_numpy(wts).cuda()
    for i in range(steps):
        w = wts * (1.0 + 0.1 * i * rs.rand(k))
        w_dev.copy_(torch.from_numpy(w))
        got = plan.draw(w_dev, i)[0].cpu().numpy().copy()
        want = call(S, w, pts).cpu().numpy()
        mu, W = got[D], got[:D] - got[D]
        mu_c, W_c = want[D], want[:D] - want[D]
        _check_fit(mu, W, mu_c, W_c.T.dot(W_c))
        assert np.abs(got - (mu + R[:, :D].dot(W))).max() <= 1e-12 * max(1.0, np.abs(got).max())
    plan.check()


# ---- BatchPSVI: the enqueued loop (enqueue_plan_moving) against the host loop, as tests/test_gpu_bpsvi_loop.py compares them ----
W_RTOL, P_RTOL, P_ATOL = 1e-7, 1e-6, 1e-8


class _ReplaySampler(object):
    def __init__(self, inner, noise):
        self.inner, self.noise, self.at = inner, noise, 0
        inner._noise = self._one
        inner._noise_block = self._block

    def _one(self, n):
        r = self.noise[self.at]
        self.at += 1
        return r

    def _block(self, steps, n):
        r = self.noise[self.at:self.at + steps]
        self.at += steps
        return r

    def __call__(self, n, wts, pts):
        return self.inner(n, wts, pts)

    def enqueue_plan(self, n, pts, steps):
        return self.inner.enqueue_plan(n, pts, steps)

    def enqueue_plan_moving(self, n, k, d, steps):
        return self.inner.enqueue_plan_moving(n, k, d, steps)


def test_bpsvi_enqueued_loop_matches_the_host_loop(bc, torch):
    from bpsvi_models import make_logistic_data
    N, D, S, k, T = 2000, 32, 64, 340, 3
    Z = make_logistic_data(11, N, D)
    g = torch.Generator(device="cuda")
    g.manual_seed(17)
    noise = torch.randn(2 * T + 4, S, D + D % 2, dtype=torch.float64, device="cuda", generator=g)
    sched = lambda i: 0.2 / (1.0 + i)
    out = {}
    for mode in (True, False):
        smp = _ReplaySampler(bc.LaplacePosteriorSampler("logistic", D, stream=True), noise)
        prj = bc.DeviceProjector("logistic", smp, S)
        alg = bc.BatchPSVICoreset(Z, prj, T, step_sched=sched)
        alg.ENQUEUE = mode
        np.random.seed(3)
        alg.build(k)
        state = np.random.get_state()[1].copy()
        used = smp.at
        if mode:
            assert alg._enqueue_plan() is not None                          # (the enqueued path is the one that ran)
        else:
            assert alg._enqueue_plan() is None
        out[mode] = (alg.wts.copy(), alg.pts.copy(), used, state)
        assert alg.pts.shape == (k, Z.shape[1])
    assert out[True][2] == out[False][2] == 1 + T
    assert np.array_equal(out[True][3], out[False][3])
    ew = np.abs(out[True][0] - out[False][0]) / np.abs(out[False][0])
    ep = np.abs(out[True][1] - out[False][1]) / (P_ATOL + P_RTOL * np.abs(out[False][1]))
    print("enqueued vs host: weights worst relative difference %.3e (bound %.0e); points worst |diff| / (atol + rtol |want|) %.3e (bound 1)"
          % (ew.max(), W_RTOL, ep.max()))
    np.testing.assert_allclose(out[True][0], out[False][0], rtol=W_RTOL)
    np.testing.assert_allclose(out[True][1], out[False][1], rtol=P_RTOL, atol=P_ATOL)


# ---- failures stick ---------------------------------------------------------------------------------------------------------
def test_failures_stick(bc, torch):
    from bayesiancoresets_amd import _native
    family, D, k, steps, S = "poisson", 6, 3000, 3, 16
    pts, wts, _ = _laplace_case(family, D, k, 50 * D + k)
    smp = bc.LaplacePosteriorSampler(family, D, seed=4, stream=True)
    plan = smp.enqueue_plan(S, pts, steps)
    assert plan is not None
    w_dev = torch.from_numpy(wts).cuda()
    bad = wts.copy()
    bad[5] = np.nan
    for i in range(steps):
        w_dev.copy_(torch.from_numpy(bad if i == 1 else wts))
        plan.draw(w_dev, i)
    with pytest.raises(_native.EngineError):
        plan.check()
    # the iteration limit, through check()
    one = bc.LaplacePosteriorSampler(family, D, seed=4, max_iter=1, stream=True)
    with pytest.raises(_native.EngineError, match="iteration limit"):
        one(S, wts, pts)
    assert one._status.cpu().numpy()[0] == 1
    # a default sampler keeps declining what does not fit the LDS
    assert bc.LaplacePosteriorSampler(family, D, seed=4).enqueue_plan(S, pts, steps) is None
    with pytest.raises(ValueError):
        bc.LaplacePosteriorSampler(family, D, seed=4)(S, wts, pts)


# ---- the HMC frame ----------------------------------------------------------------------------------------------------------
def test_device_hmc_device_frame(bc, torch):
    family, D, N = "logistic", 10, 5000
    pts, _, fit = _laplace_case(family, D, N, 9)
    Z = torch.from_numpy(pts).cuda()
    mu_ref, cov_ref = fit(pts, None)
    res = bc.DeviceHMC(family, D, chains=8, leapfrog=4, seed=1, device_frame=True).sample(Z, None, 10, 10)
    assert res.streamed and res.samples.shape == (8, 10, D) and np.all(np.isfinite(res.samples))
    _check_fit(res.center, res.transform, mu_ref, cov_ref)
    off = bc.DeviceHMC(family, D, chains=8, leapfrog=4, seed=1).sample(Z, None, 10, 10)
    assert not bc.DeviceHMC(family, D, chains=8, leapfrog=4, seed=1).device_frame
    assert type(off) is type(res)
    assert sorted(vars(off)) == sorted(vars(res))
    np.testing.assert_allclose(off.center, mu_ref, rtol=1e-7, atol=1e-9)          # (the host fit, as before)
    np.testing.assert_allclose(off.transform.T.dot(off.transform), cov_ref, rtol=1e-6, atol=1e-9 * np.abs(cov_ref).max())
    assert off.streamed and off.samples.shape == res.samples.shape and np.all(np.isfinite(off.samples))
