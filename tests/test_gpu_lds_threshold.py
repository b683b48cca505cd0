"""GPU: the three LDS-resident samplers across the size from which a kernel has to be given its dynamic LDS (csrc/launch_host.h:
raise_dynamic_lds with 16 KiB for csrc/hmc.hip and csrc/nuts.hip, 32 KiB for csrc/laplace.hip), in both directions and in one
process: the last size at the threshold, the first past it, a larger one, the first past it again.  When nothing ran before
these are: no request, the first request, a larger request, no request.  Every run takes the LDS kernel and agrees with the
streamed form of the same sampler at the tolerance the existing comparison of the two paths uses; the two runs of the repeated
size give the same bits."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bayesian-coresets_amd", "examples", "common"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import nuts_restatement as nr  # noqa: E402
from test_gpu_hmc import _teacher_forced as _hmc_teacher_forced, _tolerances  # noqa: E402
from test_gpu_laplace_stream import _check_fit, _laplace_case, _probe_noise, _reference  # noqa: E402
from test_gpu_nuts import _teacher_forced as _nuts_teacher_forced  # noqa: E402

pytestmark = pytest.mark.gpu
D = 2
HMC_SIZES = (341, 342, 1500, 342)          # 48 k bytes of points: 16368 <= 16 KiB < 16416, 72000
LAPLACE_SIZES = (585, 586, 1200, 586)      # 56 k bytes: 32760 <= 32 KiB < 32816, 67200
CLOSE = 1e-9


@pytest.fixture(scope="module")
def bc():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import bayesiancoresets_amd as bc
    return bc


_FRAMES = {}


def _points(k):
    """The first k of 1500 logistic rows with their weights, and the Laplace frame of that weighted posterior (host fit)."""
    import model_lr
    rs = np.random.RandomState(61)
    pts, wts = model_lr.synthetic_rows(max(HMC_SIZES), D, rs)[:k], rs.uniform(0.5, 2.0, max(HMC_SIZES))[:k]
    if k not in _FRAMES:
        mu, cov = model_lr.laplace_fit(pts, wts)
        _FRAMES[k] = (mu, np.linalg.cholesky(cov).T)
    return (pts, wts) + _FRAMES[k]


def test_hmc_across_the_threshold(bc):
    from bayesiancoresets_amd import _native
    lib = _native.load()
    assert [int(lib.bcx_hmc_coreset_lds_bytes(k, D)) for k in HMC_SIZES] == [16368, 16416, 72000, 16416]
    runs = []
    for k in HMC_SIZES:
        pts, wts, mu, Wm = _points(k)
        a, b = (bc.DeviceHMC("logistic", D, chains=4, leapfrog=3, seed=11).sample(pts, wts, 2, 2, center=mu, transform=Wm, keep_trace=True,
                                                                                 _dev_force_stream=force) for force in (False, True))
        assert not a.streamed and b.streamed and np.array_equal(a.trace["noise"], b.trace["noise"])
        _, f64, _, _ = _hmc_teacher_forced("logistic", pts, wts, D, 3, a, transitions=(0,))
        tol = _tolerances(f64)["proposal"]
        for name in ("proposal", "theta"):
            x, y = a.trace[name][:, 0], b.trace[name][:, 0]
            err = np.abs(x - y).max() / max(1.0, np.abs(x).max())
            print("hmc k=%d %s at transition 1: coreset vs streamed %.3g (tolerance %.3g)" % (k, name, err, tol))
            assert err <= tol, (k, name, err, tol)
        runs.append(a)
    for q in ("theta", "xi", "proposal", "diag"):
        assert runs[1].trace[q].tobytes() == runs[3].trace[q].tobytes(), q


def test_nuts_across_the_threshold(bc):
    from bayesiancoresets_amd import _native
    lib = _native.load()
    assert [int(lib.bcx_nuts_coreset_lds_bytes(k, D)) for k in HMC_SIZES] == [16368, 16416, 72000, 16416]
    J, runs = 3, []
    for k in HMC_SIZES:
        pts, wts, mu, Wm = _points(k)
        a, b = (bc.DeviceHMC("logistic", D, chains=4, seed=11, kernel="nuts", max_depth=J, stream=force).sample(
            pts, wts, 2, 2, center=mu, transform=Wm, keep_trace=True, _dev_force_stream=force) for force in (False, True))
        assert not a.streamed and b.streamed and np.array_equal(a.trace["noise"], b.trace["noise"])
        # the discrete outcomes where the long-double statement is sure of them, from the LDS run's states and steps
        tl = nr.Target("logistic", pts, wts, D, a.center, a.transform, np.longdouble)
        dg = a.trace["diag"]
        sure = np.zeros(dg.shape[:2], dtype=bool)
        for c in range(dg.shape[0]):
            for t in range(dg.shape[1]):
                xi = a.trace["xi"][c, t - 1] if t else np.zeros(D)
                base = dg[c, t - 1, 3] if t else a.trace["step0"]
                sure[c, t] = nr.transition_recursive(tl, xi, a.trace["noise"][c, t], base, J)["margin"] >= CLOSE
        print("nuts k=%d: %d of %d transitions with a margin >= 1e-9" % (k, sure.sum(), sure.size))
        assert sure[:, 0].any()
        for col in (1, 2, 6):                                   # depth, leapfrog steps, divergent
            assert np.array_equal(dg[:, :, col][sure], b.trace["diag"][:, :, col][sure]), (k, col)
        _, f64, _, _, _ = _nuts_teacher_forced("logistic", pts, wts, D, J, a)
        tol = _tolerances(f64)["xi"]
        x, y = a.trace["xi"][:, 0], b.trace["xi"][:, 0]
        err = np.abs(x - y).max() / max(1.0, np.abs(x).max())
        print("nuts k=%d first transition: LDS vs streamed xi %.3g (tolerance %.3g)" % (k, err, tol))
        assert err <= tol, (k, err, tol)
        runs.append(a)
    for q in ("theta", "xi", "diag"):
        assert runs[1].trace[q].tobytes() == runs[3].trace[q].tobytes(), q


def test_laplace_across_the_threshold(bc):
    import torch
    from bayesiancoresets_amd import _native
    lib = _native.load()
    assert [int(lib.bcx_laplace_sampler_lds_bytes(k, D)) for k in LAPLACE_SIZES] == [32760, 32816, 67200, 32816]
    S = D + 20
    R, Rd = _probe_noise(torch, D, S, 3)
    draws = []
    for k in LAPLACE_SIZES:
        pts, wts, fit = _laplace_case("logistic", D, k, 50 * D + k)
        out = {}
        for force in (False, True):
            smp = bc.LaplacePosteriorSampler("logistic", D, seed=4, stream=True)
            smp._dev_force_stream = force
            assert smp._streams(k) == force
            smp._noise = lambda n: Rd
            th = smp(S, wts, pts).cpu().numpy().copy()
            mu = th[D]
            W = th[:D] - mu
            want = mu + R[:, :D].dot(W)
            assert np.abs(th - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
            out[force] = (mu, W, th)
        mu_ref, cov_ref = _reference(fit, pts, wts, D)
        for force in (False, True):
            _check_fit(out[force][0], out[force][1], mu_ref, cov_ref)
        _check_fit(out[True][0], out[True][1], out[False][0], out[False][1].T.dot(out[False][1]))
        draws.append(out[False][2])
    assert draws[1].tobytes() == draws[3].tobytes()
