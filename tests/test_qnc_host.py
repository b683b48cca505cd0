"""CPU-only: the yardsticks of the quasi-Newton coreset.  The NumPy restatement (tests/qnc_restatement.py)
against the cases with a closed form, in float64 and in long double (the referee of the device tests); the host loop of
``bc.QuasiNewtonCoreset`` against the restatement on replayed draws; ``build``'s bookkeeping; the compiled kernels' resources."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import bayesiancoresets_amd as bc
import qnc_restatement as restate
from models import linreg_log_likelihood, linreg_sampler, make_linreg_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = (np.longdouble, np.float64)


def test_the_referee_is_wider_than_double():
    assert np.finfo(np.longdouble).eps < 2.0 ** -60


# ---- the restatement against closed forms -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k,S", ((1, 2), (3, 9), (8, 9), (12, 40)))
def test_one_full_step_without_regularisation_is_least_squares(dtype, k, S):
    """tau = 0, gamma = 1, k <= S - 1 independent centred rows: w + d = (V V^T)^-1 V c, the least-squares solution of V^T w = c,
    from any w (here kept positive, so the clamp does not act)."""
    rs = np.random.RandomState(10 * k + S)
    V_raw = rs.randn(k, S) - 500.0
    V = V_raw - V_raw.mean(axis=1)[:, None]
    w_star = 1.0 + rs.rand(k)
    c = w_star.dot(V) + 0.01 * rs.randn(S)
    want = np.linalg.lstsq(V.T, c, rcond=None)[0]
    assert (want > 0).all()
    for w0 in (np.zeros(k), 5.0 * rs.rand(k), want.copy()):
        got, d = restate.step(c, V_raw, w0, 1.0, 0.0, dtype)
        assert got.dtype == dtype
        cond = np.linalg.cond(V.dot(V.T))
        assert np.abs(np.asarray(got, dtype=np.float64) - want).max() <= 64 * k * cond * 2.0 ** -53 * max(np.abs(want).max(), np.abs(w0).max())


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_residual_no_direction(dtype):
    rs = np.random.RandomState(1)
    V_raw = np.asarray(rs.randn(6, 20), dtype=dtype)
    w = np.asarray(rs.rand(6), dtype=dtype)
    V = V_raw - V_raw.mean(axis=1)[:, None]
    got, d = restate.step(w.dot(V), V_raw, w, 0.7, 1e-2, dtype)
    assert np.all(d == 0) and np.array_equal(got, w)


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_draw_gives_no_direction(dtype):
    """S = 1: a row centred over one draw is zero, G = 0, b = 0, and any tau > 0 gives d = 0."""
    rs = np.random.RandomState(2)
    w = rs.rand(5)
    for tau in (1e-2, 3.0):
        got, d = restate.step(rs.randn(1), rs.randn(5, 1), w, 1.0, tau, dtype)
        assert np.all(d == 0) and np.array_equal(np.asarray(got, dtype=np.float64), w)
    with pytest.raises(np.linalg.LinAlgError):
        restate.step(rs.randn(1), rs.randn(5, 1), w, 1.0, 0.0, dtype)      # (tau = 0: G = 0 has no factor)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_clamp_keeps_a_nan(dtype):
    rs = np.random.RandomState(3)
    c = rs.randn(12)
    c[4] = np.nan
    got, d = restate.step(c, rs.randn(4, 12), rs.rand(4), 1.0, 1e-2, dtype)
    assert np.isnan(np.asarray(got, dtype=np.float64)).all() and np.isnan(np.asarray(d, dtype=np.float64)).all()
    # and a direction that would take a weight below zero is cut there
    V_raw = rs.randn(2, 30)
    V = V_raw - V_raw.mean(axis=1)[:, None]
    got, d = restate.step(np.array([-3.0, 2.0]).dot(V), V_raw, np.array([0.5, 0.5]), 1.0, 0.0, dtype)
    assert got[0] == 0 and abs(float(got[1]) - 2.0) < 1e-9


def test_written_out_factorisation_against_lapack():
    rs = np.random.RandomState(4)
    B = rs.randn(9, 30)
    A = B.dot(B.T) / 30 + 1e-2 * np.eye(9)
    L = restate.cholesky(A)
    assert np.abs(L - np.linalg.cholesky(A)).max() <= 1e-13 * np.abs(L).max()
    b = rs.randn(9)
    x = restate.solve_upper(L.T, restate.solve_lower(L, b))
    assert np.abs(x - np.linalg.solve(A, b)).max() <= 1e-10 * np.abs(x).max()
    with pytest.raises(np.linalg.LinAlgError):
        restate.cholesky(np.array([[1.0, 2.0], [2.0, 1.0]]))
    with pytest.raises(np.linalg.LinAlgError):
        restate.cholesky(np.array([[np.nan]]))


# ---- the host loop of the class ---------------------------------------------------------------------------------------------------
class _HostSums(object):
    """Stand-in for the device engine behind a host projector (``SparseVICoreset._engine_for``: one ingest pass gives the column
    sums; needs a GPU).  Test infrastructure: NumPy's column sums."""

    def __init__(self, vecs):
        self.colsum = vecs.sum(axis=0)

    def vector(self, which):
        assert which == 0
        return self.colsum


def _tiny(seed=5):
    N, D, S, k, T = 200, 4, 32, 8, 5
    Z = make_linreg_data(seed, N, D)
    sigsq = 1.3
    return N, D, S, k, T, Z, sigsq


def _host_alg(Z, D, S, sigsq, **kw):
    prj = bc.BlackBoxProjector(linreg_sampler(np.zeros(D), 2.0 * np.eye(D), sigsq), S, lambda z, th: linreg_log_likelihood(z, th, sigsq))
    alg = bc.QuasiNewtonCoreset(Z, prj, **kw)
    alg._engine_for = _HostSums
    return alg


@pytest.mark.parametrize("n_sub", (None, 60))
def test_host_loop_against_the_restatement(n_sub):
    """N = 200, k = 8, S = 32, T = 5 with a ``BlackBoxProjector``: the class's host loop and ``loop(..., np.float64)`` consume
    NumPy's stream in the same order (the constructor's draw, ``choice``, then per step the sampler's ``randn`` and, with
    ``n_subsample_opt``, one ``randint``), so they see the same draws; same arithmetic, same library: 1e-12 relative."""
    N, D, S, k, T, Z, sigsq = _tiny()
    sched = lambda i: 1.0 / (1.0 + 0.5 * i)
    np.random.seed(7)
    alg = _host_alg(Z, D, S, sigsq, opt_itrs=T, tau=1e-2, step_sched=sched, n_subsample_opt=n_sub)
    assert alg._enqueue_plan() is None and alg._enqueue_plan_subsampled() is None
    alg.build(k)
    after = np.random.get_state()[1].copy()
    # the same stream again, by hand
    np.random.seed(7)
    smp = linreg_sampler(np.zeros(D), 2.0 * np.eye(D), sigsq)
    smp(S, np.array([]), np.array([]))                                    # BlackBoxProjector's constructor
    idcs = np.random.choice(N, size=k, replace=False)
    pts = Z[idcs]

    def inputs(i, w):
        th = smp(S, w, pts)
        data, scaling = (Z, 1.0) if n_sub is None else (Z[np.random.randint(N, size=n_sub)], N / n_sub)
        ll = linreg_log_likelihood(data, th, sigsq)
        ll -= ll.mean(axis=1)[:, None]
        return scaling * ll.sum(axis=0), linreg_log_likelihood(pts, th, sigsq)

    want = restate.loop(inputs, N / k * np.ones(k), [sched(i) for i in range(T)], 1e-2, np.float64)
    assert np.array_equal(np.random.get_state()[1], after)                # (both consumed the same number of draws)
    assert np.array_equal(alg.idcs, idcs) and np.array_equal(alg.pts, pts)
    dev = np.abs(alg.wts - want).max() / np.abs(want).max()
    print("host loop against the float64 restatement: %.3g relative" % dev)
    assert dev <= 1e-12
    assert (alg.wts >= 0).all() and not np.array_equal(alg.wts, N / k * np.ones(k))
    # optimize(): opt_itrs more steps from where build() stopped
    w1 = alg.wts.copy()
    alg.optimize()
    assert alg.wts.shape == (k,) and not np.array_equal(alg.wts, w1) and np.array_equal(alg.idcs, idcs)


def test_host_loop_failed_factorisation_raises():
    """tau = 0 with more points than draws: G is singular; the host loop names the step (LinAlgError -> EngineError(ERR_STATE))."""
    from bayesiancoresets_amd import _native
    N, D, S, k, T, Z, sigsq = _tiny()
    np.random.seed(8)
    alg = _host_alg(Z, D, 4, sigsq, opt_itrs=3, tau=0.0)
    with pytest.raises(_native.EngineError) as e:
        alg.build(12)
    assert e.value.code == _native.ERR_STATE and "step 0" in str(e.value)


def test_host_loop_weights_that_are_not_finite_raise():
    from bayesiancoresets_amd import _native
    N, D, S, k, T, Z, sigsq = _tiny()
    np.random.seed(9)
    alg = _host_alg(Z, D, S, sigsq, opt_itrs=1, step_sched=lambda i: float("nan"))
    with pytest.raises(_native.EngineError) as e:
        alg.build(k)
    assert e.value.code == _native.ERR_STATE and "not finite" in str(e.value)


# ---- build's bookkeeping ----------------------------------------------------------------------------------------------------------------
def test_build_bookkeeping():
    N, D, S, k, T, Z, sigsq = _tiny()
    np.random.seed(11)
    alg = _host_alg(Z, D, S, sigsq, opt_itrs=0)
    alg.build(k)
    assert alg.idcs.shape == (k,) and len(set(alg.idcs.tolist())) == k and alg.idcs.dtype == np.int64
    assert np.array_equal(alg.pts, Z[alg.idcs])
    assert alg.wts.sum() == N and np.all(alg.wts == N / k)               # (opt_itrs = 0: the initial weights)
    assert alg.error() == 0.0
    first = alg.idcs.copy()
    alg.build(k + 3)                                                       # a second build starts afresh
    assert alg.idcs.shape == (k + 3,) and len(set(alg.idcs.tolist())) == k + 3 and not np.array_equal(alg.idcs[:k], first)
    assert np.array_equal(alg.pts, Z[alg.idcs]) and alg.wts.sum() == pytest.approx(N, rel=1e-14)
    wts, pts, idcs = alg.get()
    assert wts.shape == (k + 3,) and np.array_equal(pts, Z[idcs])
    alg.reset()
    assert alg.size() == 0 and alg.pts.shape == (0, D + 1)


def test_argument_errors():
    N, D, S, k, T, Z, sigsq = _tiny()
    np.random.seed(12)
    for kw in ({"tau": -1e-3}, {"tau": float("nan")}, {"opt_itrs": -1}, {"group": object()}, {"row_offset": 100}, {"subsample": "gpu"}):
        with pytest.raises(ValueError):
            _host_alg(Z, D, S, sigsq, **kw)
    with pytest.raises(ValueError):
        _host_alg(Z, D, S, sigsq, subsample="device")                     # (needs a DeviceProjector, as in SparseVI)
    assert bc.QuasiNewtonCoreset is bc.coreset.QuasiNewtonCoreset and issubclass(bc.QuasiNewtonCoreset, bc.Coreset)


# ---- the compiled kernels ---------------------------------------------------------------------------------------------------------------
def test_no_spill_no_scratch_in_any_kernel():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"),
                          os.path.join(ROOT, "bayesian-coresets_amd", "csrc", "qn.hip")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    print(out.stdout)
    assert lines[-1] == "kernels with spills or scratch: 0"
    for name in ("qn_center_kernel", "qn_rhs_kernel", "qn_small_kernel", "qn_diag_kernel", "qn_panel_kernel", "qn_update_kernel",
                 "qn_back_kernel"):
        assert len([ln for ln in lines if name in ln]) == 1, (name, lines)
    assert len(lines) == 8, lines
    for ln in lines[:-1]:
        assert re.search(r"spill\s+0 scratch\s+0 B", ln), ln
