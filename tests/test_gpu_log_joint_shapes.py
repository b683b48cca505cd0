"""GPU: the launch shapes of the log-joint pass (csrc/hmc.hip: lj_partial_kernel, lj_finalize_kernel, lj_workgroups) that
tests/test_gpu_hmc.py does not reach -- one row and one-row tails, 127 / 128 / 129 rows, the loop over several tiles of a
workgroup (N > 65536), D = 1, 31, 32, C on both sides of the 8-column group and of the 256-column chunk (whose partials share
one scratch buffer), rows and parameter vectors wider than the model (ldz, ldt), signed and zero weights and none at all --
through ``bcx_log_joint_grad`` itself, against the long-double sums of tests/lik_point_referee.py.

Per output the bound is 16 U sum_j |w_j| scale_j (|x_jd|) + 4 n U (sum of the absolute addends), n = N + D + 1 and U = 2^-53:
the form of tests/test_gpu_hmc.py::_bounds with the point terms' scales in front.  The last test runs the streamed HMC (the
pass with ldt = 32 and without the constants) at a size where a workgroup walks two tiles."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lik_point_referee as ref  # noqa: E402

pytestmark = pytest.mark.gpu
FAM = {"logistic": 0, "poisson": 1}
SENTINEL = -7.25
GUARD = 64                        # doubles behind the scratch buffer that must keep the sentinel

# N, D, C, columns the rows are wider by, columns the parameter vectors are wider by
SHAPES = (
    (1, 1, 1, 0, 0),
    (127, 2, 7, 1, 0),
    (128, 31, 8, 0, 1),
    (129, 32, 9, 3, 0),
    (257, 5, 255, 0, 0),
    (900, 3, 256, 2, 29),         # ldt = 32: what bcx_hmc_stream passes
    (900, 3, 257, 0, 0),
    (1000, 32, 513, 0, 0),
    (65536, 4, 3, 0, 0),          # the last size with one tile per workgroup
    (65537, 32, 9, 1, 0),         # two tiles per workgroup, the last workgroup holds one row
    (200000, 7, 17, 0, 0),        # four tiles per workgroup
)


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def lib(torch):
    from bayesiancoresets_amd import _native
    return _native.load()


def _inputs(family, N, D, C):
    """Rows whose predictors cover +-30, one in a hundred out to +-400; signed weights, one in twenty zero."""
    rs = np.random.RandomState(1000 * D + C + N % 997)
    th = rs.randn(C, D) / np.sqrt(D)
    reach = 10.0 * rs.rand(N)
    reach[rs.rand(N) < 0.01] = 130.0
    if N == 1:
        reach[:] = 3.0
    X = rs.randn(N, D) * reach[:, None]
    Z = np.hstack((X, rs.poisson(3.0, N)[:, None].astype(np.float64))) if family == "poisson" else X
    w = 2.0 * rs.randn(N)
    w[rs.rand(N) < 0.05] = 0.0
    return Z, w, th


def _call(torch, lib, family, Z, w, th, padz, padt):
    """(values, gradients (C x ldt, padding included), the scratch buffer's guard) of one call on padded buffers: NaN in the
    padding of the inputs (it must not be read), the sentinel in the outputs' and behind the scratch."""
    N, cols = Z.shape
    C, D = th.shape
    ldz, ldt = cols + padz, D + padt
    Zp = np.full((N, ldz), np.nan)
    Zp[:, :cols] = Z
    Tp = np.full((C, ldt), np.nan)
    Tp[:, :D] = th
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    Zd, Td = dev(Zp), dev(Tp)
    wd = None if w is None else dev(w)
    need = int(lib.bcx_log_joint_grad_scratch_bytes(N, D, C))
    assert need > 0 and need % 8 == 0
    work = torch.full((need // 8 + GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
    val = torch.full((C,), SENTINEL, dtype=torch.float64, device="cuda")
    grad = torch.full((C, ldt), SENTINEL, dtype=torch.float64, device="cuda")
    rc = lib.bcx_log_joint_grad(int(torch.cuda.current_stream().cuda_stream), FAM[family], Zd.data_ptr(), N, ldz, D,
                                None if wd is None else wd.data_ptr(), Td.data_ptr(), C, ldt, val.data_ptr(), grad.data_ptr(), work.data_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    return val.cpu().numpy(), grad.cpu().numpy(), work[need // 8:].cpu().numpy()


@pytest.mark.parametrize("family", ref.FAMILIES)
@pytest.mark.parametrize("N,D,C,padz,padt", SHAPES)
def test_log_joint_grad_at_every_launch_shape(torch, lib, family, N, D, C, padz, padt):
    Z, w, th = _inputs(family, N, D, C)
    table = ref.point_table(family, Z, th)
    for wts in (w, None):
        what = "%s N=%d D=%d C=%d ldz+%d ldt+%d %s" % (family, N, D, C, padz, padt, "weighted" if wts is not None else "unweighted")
        val, grad, guard = _call(torch, lib, family, Z, wts, th, padz, padt)
        rv, rg, bv, bg = ref.log_joint_grad(family, Z, wts, th, with_bounds=True, table=table)
        assert np.all(np.isfinite(val)) and np.all(np.isfinite(grad[:, :D])), what
        ev = (np.abs(val.astype(ref.LD) - rv) / bv).max()
        eg = (np.abs(grad[:, :D].astype(ref.LD) - rg) / bg).max()
        print("%s: value error / bound %.3g, gradient error / bound %.3g" % (what, float(ev), float(eg)))
        assert ev <= 1.0 and eg <= 1.0, what
        assert np.all(grad[:, D:] == SENTINEL), what           # the words between D and ldt are not the kernel's
        assert np.all(guard == SENTINEL), what                 # nor anything behind bcx_log_joint_grad_scratch_bytes
        val2, grad2, _ = _call(torch, lib, family, Z, wts, th, padz, padt)
        assert np.array_equal(val, val2) and np.array_equal(grad, grad2), what
        if C > 8:                                              # the chunk and the group a column falls in do not matter
            val8, grad8, _ = _call(torch, lib, family, Z, wts, th[:8], padz, padt)
            assert np.array_equal(val[:8], val8) and np.array_equal(grad[:8], grad8), what


def test_streamed_hmc_over_two_tiles_per_workgroup(torch):
    """DeviceHMC on 65537 logistic rows of 32 parameters (they stream: one workgroup's LDS does not hold them), 9 chains, 2
    leapfrog steps, 3 transitions: every transition against tests/hmc_restatement.py in long double, teacher-forced, with the
    bars of tests/test_gpu_hmc.py::test_transitions_equal_restatement."""
    import bayesiancoresets_amd as bc
    from test_gpu_hmc import _teacher_forced, _tolerances
    N, D, L = 65537, 32, 2
    rs = np.random.RandomState(65537)
    truth = 0.3 * rs.randn(D)
    X = np.hstack((rs.randn(N, D - 1), np.ones((N, 1))))
    yv = np.where(rs.rand(N) < 1 / (1 + np.exp(-X.dot(truth))), 1.0, -1.0)
    pts = yv[:, None] * X
    # the frame: the posterior's scale is 2 / sqrt(N) a coordinate
    res = bc.DeviceHMC("logistic", D, chains=9, leapfrog=L, seed=12).sample(pts, None, 2, 1, center=truth, transform=np.eye(D) * (2.0 / np.sqrt(N)),
                                                                           keep_trace=True)
    assert res.streamed and res.trace["diag"].shape[:2] == (9, 3)
    dev, f64, wrong, close = _teacher_forced("logistic", pts, None, D, L, res)
    tol = _tolerances(f64)
    for q in ("proposal", "dH", "eps"):
        print("streamed HMC N=%d %s: device %.3g, float64 restatement %.3g, tolerance %.3g" % (N, q, dev[q], f64[q], tol[q]))
    for q in ("proposal", "dH", "eps"):
        assert dev[q] <= tol[q], (q, dev[q], tol[q])
    assert wrong == 0 and close <= 1
    assert np.all(np.isfinite(res.trace["diag"][:, :, 0]))
