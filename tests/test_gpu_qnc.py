"""GPU: the quasi-Newton coreset (csrc/qn.hip, bayesiancoresets_amd/coreset/quasinewton.py).

* ``bcx_quasi_newton_step`` against the long-double restatement (tests/qnc_restatement.py) on every tile edge of a 32-wide panel,
  both sides of the single-workgroup threshold (128 | 129), k > S and S = 1; determinism; the error paths;
* the loops of ``bc.QuasiNewtonCoreset`` -- host and enqueued -- against the restatement on replayed draws;
* the build lowers the exact Gaussian KL of the linear-regression posterior."""
import os
import sys

import numpy as np
import pytest

import qnc_restatement as restate
from models import make_linreg_data, linreg_weighted_post

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble
MARGIN = 16          # the package's usual margin over the float64 restatement's own deviation


@pytest.fixture(scope="module")
def bc():
    import bayesiancoresets_amd as bc
    return bc


@pytest.fixture(scope="module")
def lib():
    from bayesiancoresets_amd import _native
    return _native.load()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _norm(x):
    return float(np.sqrt((np.asarray(x, dtype=LD) ** 2).sum()))


class _Step(object):
    """One set of device buffers for calls of bcx_quasi_newton_step at (k, S)."""

    def __init__(self, lib, k, S, colsum, core, w0, sched, steps=1, ldc=None):
        import torch
        self.lib, self.k, self.S = lib, k, S
        self.ldc = S if ldc is None else ldc
        self.col, self.core, self.w, self.sched = _dev(colsum), _dev(core), _dev(w0), _dev(sched)
        self.dir = torch.full((k,), 7.0, dtype=torch.float64, device="cuda")
        self.trace = torch.full((steps, k), -1.0, dtype=torch.float64, device="cuda")
        self.status = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.need = int(lib.bcx_quasi_newton_scratch_bytes(k, S))
        assert self.need > 0
        self.work = torch.full((self.need // 8 + 2,), float("nan"), dtype=torch.float64, device="cuda")      # (stale scratch must not matter)
        self.stream = int(torch.cuda.current_stream().cuda_stream)

    def __call__(self, step, tau, raw, scaling=1.0, k=None, S=None, work_bytes=None, col=None):
        return self.lib.bcx_quasi_newton_step(self.stream, self.k if k is None else k, self.S if S is None else S,
                                              (self.col if col is None else col).data_ptr(), scaling, self.core.data_ptr(), self.ldc, raw,
                                              self.w.data_ptr(), self.sched.data_ptr(), step, tau, self.dir.data_ptr(), self.trace.data_ptr(),
                                              self.status.data_ptr(), self.work.data_ptr(), self.need if work_bytes is None else work_bytes)


def _inputs(k, S, seed):
    rs = np.random.RandomState(seed)
    V0 = rs.randn(k, S)                                   # unit-variance rows
    colsum = 20.0 * rs.randn(S)
    w0 = np.abs(rs.randn(k)) + 0.1
    return V0, colsum, w0


# ---- 1. the step kernel against the referee -------------------------------------------------------------------------------------------
KS = (1, 2, 31, 32, 33, 65, 128, 129, 130, 257)
SS = (1, 7, 64, 200)
_ratios = []


@pytest.mark.parametrize("S", SS)
@pytest.mark.parametrize("k", KS)
def test_step_kernel_against_the_referee(lib, k, S):
    """||d_dev - d_ld|| / ||d_ld|| <= 16 max(the float64 restatement's own deviation, k cond_2(G + tau I) 2^-53), the textbook forward
    bound of a Cholesky solve; per weight |w'_dev - w'_ld| <= gamma x that bar x ||d_ld||; the trace row equals the weights."""
    V0, colsum, w0 = _inputs(k, S, 1000 * k + S)
    scaling = 1.5
    for raw in (0, 1):
        # raw: rows offset by -500 (log-likelihoods like -500 +- 1), centred by the kernel; else centred here, in float64
        core = V0 - 500.0 if raw else V0 - V0.mean(axis=1)[:, None]
        for tau in ((1e-2, 0.0) if k < S else (1e-2,)):
            Vc, A, b = restate.system(scaling * colsum, core, w0, tau, LD)
            cond = float(np.linalg.cond(np.asarray(A, dtype=np.float64)))
            assert cond <= 1e8, cond                                     # a condition on the inputs
            for gamma in (1.0, 0.3):
                w_ld, d_ld = restate.step(scaling * colsum, core, w0, gamma, tau, LD)
                w_64, d_64 = restate.step(scaling * colsum, core, w0, gamma, tau, np.float64)
                st = _Step(lib, k, S, colsum, core, w0, [gamma])
                assert st(0, tau, raw, scaling) == 0, lib.bcx_project_last_error()
                d_dev, w_dev, tr = st.dir.cpu().numpy(), st.w.cpu().numpy(), st.trace.cpu().numpy()
                assert int(st.status.item()) == 0
                assert np.array_equal(tr[0], w_dev)                      # bit for bit
                nd = _norm(d_ld)
                if nd == 0.0:                                            # S = 1: G = 0, b = 0
                    assert np.all(d_dev == 0.0) and np.array_equal(w_dev, w0)
                    continue
                dev64 = _norm(d_64 - d_ld) / nd
                bar = MARGIN * max(dev64, k * cond * U)
                err = _norm(d_dev - d_ld) / nd
                ratio = err / max(dev64, k * cond * U)
                _ratios.append((ratio, err / max(dev64, 1e-300), k, S, raw, tau, gamma))
                print("k %3d S %3d raw %d tau %.0e gamma %.1f: dev %.3g  float64 %.3g  k cond u %.3g  (ratio to the floor %.2f)"
                      % (k, S, raw, tau, gamma, err, dev64, k * cond * U, ratio))
                assert err <= bar, (err, bar)
                assert np.all(np.abs(np.asarray(w_dev, dtype=LD) - w_ld) <= gamma * bar * nd), float(np.abs(w_dev - np.asarray(w_ld, dtype=np.float64)).max())
                assert (w_dev >= 0).all()


def test_step_kernel_ratios_summary():
    """Not a check of its own: prints the largest ratios met above (they go into DESIGN.md 4.20)."""
    if _ratios:
        worst = max(_ratios)
        print("largest err / max(float64 deviation, k cond u): %.3g at k %d S %d raw %d tau %g gamma %g" % ((worst[0],) + worst[2:]))
        w2 = max(_ratios, key=lambda r: r[1])
        print("largest err / float64 deviation: %.3g at k %d S %d raw %d tau %g gamma %g" % ((w2[1],) + w2[2:]))


def test_trace_over_steps_and_row_stride(lib):
    """Three steps on one set of buffers, rows 11 doubles apart in memory (ldc > S, odd: rows not 16-byte aligned): trace row i
    equals w_dev after step i, and the loop equals the float64 restatement's to the loop's own rounding."""
    k, S, ldc, T = 40, 9, 11, 3
    V0, colsum, w0 = _inputs(k, S, 77)
    core = np.full((k, ldc), np.nan)
    core[:, :S] = V0 - 3.0
    sched = [1.0, 0.5, 0.25]
    st = _Step(lib, k, S, colsum, core, w0, sched, steps=T, ldc=ldc)
    w = np.asarray(w0, dtype=LD)
    bar = 0.0
    for i in range(T):
        assert st(i, 1e-2, 1) == 0
        got = st.w.cpu().numpy()
        assert np.array_equal(st.trace.cpu().numpy()[i], got)
        cond = float(np.linalg.cond(np.asarray(restate.system(colsum, core[:, :S], w, 1e-2, LD)[1], dtype=np.float64)))
        w, d = restate.step(colsum, core[:, :S], w, sched[i], 1e-2, LD)
        # an error e in w moves d by -(G + tau I)^-1 G e, no longer than e: it at most doubles; the step adds its own forward bound
        bar = 2.0 * bar + sched[i] * MARGIN * k * cond * U * _norm(d)
        assert float(np.abs(np.asarray(got, dtype=LD) - w).max()) <= bar
    assert np.all(st.trace.cpu().numpy()[:T] >= 0) and int(st.status.item()) == 0


# ---- 2. determinism ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,S", ((40, 64), (128, 100), (300, 256), (1000, 130)))
def test_same_call_same_bits(lib, k, S):
    V0, colsum, w0 = _inputs(k, S, 5 * k + S)
    out = []
    for rep in range(2):
        st = _Step(lib, k, S, colsum, V0 - 500.0, w0, [0.7])
        assert st(0, 1e-2, 1) == 0
        out.append((st.w.cpu().numpy(), st.dir.cpu().numpy()))
        assert int(st.status.item()) == 0
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert np.isfinite(out[0][0]).all() and not np.array_equal(out[0][0], w0)


# ---- 3. error paths (no fault involved) -------------------------------------------------------------------------------------------------
def test_singular_system_sets_the_status_and_keeps_the_weights(lib):
    """tau = 0 with k = 40 > S = 16: no Cholesky factor.  Status 1, w_dev bit-identical to its input -- and a following valid call
    on the same status word leaves w_dev untouched too (the word is sticky)."""
    k, S = 40, 16
    V0, colsum, w0 = _inputs(k, S, 3)
    st = _Step(lib, k, S, colsum, V0, w0, [1.0, 1.0], steps=2)
    assert st(0, 0.0, 1) == 0
    assert int(st.status.item()) == 1 and np.array_equal(st.w.cpu().numpy(), w0)
    assert np.all(st.dir.cpu().numpy() == 7.0)                            # (the direction is not handed out either)
    assert st(1, 1e-2, 1) == 0                                             # a valid call
    assert int(st.status.item()) == 1 and np.array_equal(st.w.cpu().numpy(), w0)
    st.status.zero_()
    assert st(1, 1e-2, 1) == 0
    assert int(st.status.item()) == 0 and not np.array_equal(st.w.cpu().numpy(), w0)


@pytest.mark.parametrize("k", (40, 200))
def test_singular_system_blocked_and_single(lib, k):
    S = 16
    V0, colsum, w0 = _inputs(k, S, 4)
    st = _Step(lib, k, S, colsum, V0, w0, [1.0])
    assert st(0, 0.0, 0) == 0
    assert int(st.status.item()) == 1 and np.array_equal(st.w.cpu().numpy(), w0)


@pytest.mark.parametrize("k", (12, 150))
def test_nan_in_the_column_sums_gives_nan_weights(lib, k):
    S = 32
    V0, colsum, w0 = _inputs(k, S, 5)
    colsum[3] = np.nan
    st = _Step(lib, k, S, colsum, V0, w0, [1.0])
    assert st(0, 1e-2, 1) == 0
    assert int(st.status.item()) == 0 and np.isnan(st.w.cpu().numpy()).all()


def test_argument_errors(lib):
    from bayesiancoresets_amd import _native
    k, S = 8, 16
    V0, colsum, w0 = _inputs(k, S, 6)
    st = _Step(lib, k, S, colsum, V0, w0, [1.0])
    assert lib.bcx_quasi_newton_scratch_bytes(4097, 16) == -1 and lib.bcx_quasi_newton_scratch_bytes(8, 8193) == -1
    assert lib.bcx_quasi_newton_scratch_bytes(0, 16) == -1 and lib.bcx_quasi_newton_scratch_bytes(8, 0) == -1
    assert lib.bcx_quasi_newton_scratch_bytes(4096, 8192) > 0
    for kw in ({"k": 4097}, {"S": 8193}, {"work_bytes": st.need - 1}, {"k": 0}):
        assert st(0, 1e-2, 1, **kw) == _native.ERR_ARG
        assert b"bcx_quasi_newton_step" in lib.bcx_project_last_error()
    assert st(0, -1e-3, 1) == _native.ERR_ARG and st(0, float("nan"), 1) == _native.ERR_ARG and st(-1, 1e-2, 1) == _native.ERR_ARG
    assert np.array_equal(st.w.cpu().numpy(), w0) and int(st.status.item()) == 0
    assert st(0, 1e-2, 1) == 0


# ---- 4. the loops on replayed draws ----------------------------------------------------------------------------------------------------
class _ReplaySampler(object):
    """Wraps a package sampler so that the call form and the enqueued form consume the SAME pre-drawn normal numbers."""

    def __init__(self, inner, noise, at=0):
        self.inner, self.noise, self.at = inner, noise, at
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


def _examples_on_path():
    p = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bayesian-coresets_amd", "examples", "common")
    if p not in sys.path:
        sys.path.insert(0, p)


def _loglik(family, Z, th, sigsq, dtype):
    if family == "linreg":
        Z, th = np.asarray(Z, dtype=dtype), np.asarray(th, dtype=dtype)
        r = Z[:, -1:] - Z[:, :-1].dot(th.T)
        return -(r * r) / (2 * dtype(sigsq))             # (the constant drops out of every centred row)
    import predictive_restatement
    return predictive_restatement.log_likelihood(family, Z, th, dtype)


def _loop_case(bc, family, N, D, S, k, T, colsum=None, n_sub=None, seed=0):
    """(referee, float64 restatement, host-loop class, enqueued class, draws consumed by the two class forms)."""
    import torch
    rs = np.random.RandomState(seed)
    sigsq, tau = 0.8, 1e-2
    if family == "linreg":
        Z = make_linreg_data(seed + 1, N, D)
        new_sampler = lambda: bc.LinregPosteriorSampler(np.zeros(D), 2.0 * np.eye(D), sigsq)
        kw = {"sigsq": sigsq, "colsum": colsum}
    else:
        _examples_on_path()
        import model_lr
        Z = model_lr.synthetic_rows(N, D, rs)
        new_sampler = lambda: bc.LaplacePosteriorSampler(family, D)
        kw = {}
    g = torch.Generator(device="cuda")
    g.manual_seed(100 + seed)
    noise = torch.randn(2 * T + 4, S, D + D % 2, dtype=torch.float64, device="cuda", generator=g)
    sched = lambda i: 1.0 / (1.0 + 0.25 * i)
    sub_kw = {} if n_sub is None else {"n_subsample_opt": n_sub, "subsample": "device"}
    out, used = {}, {}
    for mode in (False, True):
        np.random.seed(seed + 50)
        smp = _ReplaySampler(new_sampler(), noise)
        alg = bc.QuasiNewtonCoreset(Z, bc.DeviceProjector(family, smp, S, **kw), opt_itrs=T, tau=tau, step_sched=sched, **sub_kw)
        alg.ENQUEUE = mode
        alg.build(k)
        out[mode], used[mode] = alg.wts.copy(), smp.at
        idcs = alg.idcs.copy()
        if mode:
            assert (alg._enqueue_plan() if n_sub is None else alg._enqueue_plan_subsampled()) is not None      # (it was the enqueued loop)
    # the restatement on the same draws: the device sampler's call form at the float64 weights, the log-likelihoods on the host
    np.random.seed(seed + 50)
    assert np.array_equal(np.random.choice(N, size=k, replace=False), idcs)
    pts = Z[idcs]
    table = None if n_sub is None else [np.random.randint(N, size=n_sub) for _ in range(T)]
    res = {}
    for dtype in (LD, np.float64):
        ref = _ReplaySampler(new_sampler(), noise, at=1)            # (noise[0] went to the projector's constructor)

        def inputs(i, w):
            th = ref(S, w, pts).cpu().numpy().copy()
            data, scaling = (Z, 1.0) if table is None else (Z[table[i]], N / n_sub)
            ll = _loglik(family, data, th, sigsq, dtype)
            ll = ll - ll.mean(axis=1)[:, None]
            return dtype(scaling) * ll.sum(axis=0), _loglik(family, pts, th, sigsq, dtype)
        res[dtype] = restate.loop(inputs, N / k * np.ones(k), [sched(i) for i in range(T)], tau, dtype)
        assert ref.at == 1 + T
    return res[LD], res[np.float64], out[False], out[True], used


def _check_loops(tag, w_ld, w_64, host, enq, used, T):
    assert used[False] == used[True] == 1 + T                      # both forms consume the same number of draws
    top = float(np.abs(w_ld).max())
    own = float(np.abs(np.asarray(w_64, dtype=LD) - w_ld).max())
    bar = 64 * max(own, 1e-12 * top)
    e_host = float(np.abs(np.asarray(host, dtype=LD) - w_ld).max())
    e_enq = float(np.abs(np.asarray(enq, dtype=LD) - w_ld).max())
    print("%s: max|w| %.3g  float64 restatement %.3g  host loop %.3g  enqueued %.3g  (ratios to max(own, 1e-12 max|w|): %.2f / %.2f)"
          % (tag, top, own, e_host, e_enq, e_host / (bar / 64), e_enq / (bar / 64)))
    assert e_host <= bar and e_enq <= bar, (e_host, e_enq, bar)
    assert (enq >= 0).all() and (enq > 0).any()


@pytest.mark.parametrize("colsum", ("mfma", "moments"))
def test_loops_linreg(bc, colsum):
    T = 10
    r = _loop_case(bc, "linreg", 20000, 12, 64, 40, T, colsum=colsum, seed=1)
    _check_loops("linreg " + colsum, *r, T)


def test_loops_logistic_laplace(bc):
    T = 8
    r = _loop_case(bc, "logistic", 5000, 6, 64, 24, T, seed=2)
    _check_loops("logistic", *r, T)


def test_loops_blocked_path(bc):
    T = 4
    r = _loop_case(bc, "linreg", 20000, 12, 64, 130, T, colsum="mfma", seed=3)
    _check_loops("linreg k = 130", *r, T)


def test_loops_device_subsample(bc):
    T = 6
    r = _loop_case(bc, "linreg", 20000, 12, 64, 40, T, colsum="mfma", n_sub=2000, seed=4)
    _check_loops("linreg n_subsample_opt = 2000", *r, T)


def test_enqueued_loop_raises_on_a_failed_factorisation(bc):
    from bayesiancoresets_amd import _native
    D, N, S = 6, 5000, 16
    Z = make_linreg_data(9, N, D)
    np.random.seed(3)
    smp = bc.LinregPosteriorSampler(np.zeros(D), np.eye(D), 1.0, seed=1)
    alg = bc.QuasiNewtonCoreset(Z, bc.DeviceProjector("linreg", smp, S, sigsq=1.0), opt_itrs=3, tau=0.0)
    with pytest.raises(_native.EngineError) as e:
        alg.build(40)
    assert e.value.code == _native.ERR_STATE and "pivot" in str(e.value)


# ---- 5. it does what it is for -------------------------------------------------------------------------------------------------------------
def _gauss_kl(mu_a, Sig_a, mu_b, Sig_b):
    """KL(N(mu_a, Sig_a) || N(mu_b, Sig_b))."""
    Sb_inv = np.linalg.inv(Sig_b)
    dm = mu_b - mu_a
    return 0.5 * (np.trace(Sb_inv.dot(Sig_a)) + dm.dot(Sb_inv).dot(dm) - mu_a.shape[0] + np.linalg.slogdet(Sig_b)[1] - np.linalg.slogdet(Sig_a)[1])


def test_build_lowers_the_exact_kl(bc):
    N, D, S, M, sigsq = 20000, 10, 256, 50, 1.0
    Z = make_linreg_data(21, N, D)
    mu0, Sig0 = np.zeros(D), 4.0 * np.eye(D)
    S0inv = np.linalg.inv(Sig0)
    mu_f, U_f = linreg_weighted_post(mu0, S0inv, sigsq, Z, np.ones(N))
    np.random.seed(5)
    smp = bc.LinregPosteriorSampler(mu0, Sig0, sigsq, seed=2)
    alg = bc.QuasiNewtonCoreset(Z, bc.DeviceProjector("linreg", smp, S, sigsq=sigsq), opt_itrs=20)
    alg.build(M)
    assert alg._enqueue_plan() is not None

    def kl(w):
        mu, Uw = linreg_weighted_post(mu0, S0inv, sigsq, alg.pts, w)
        return _gauss_kl(mu, Uw.dot(Uw.T), mu_f, U_f.dot(U_f.T))
    before, after = kl(N / M * np.ones(M)), kl(alg.wts)
    print("KL(pi_w || pi): %.4g at the initial weights N / M, %.4g after build(%d) with opt_itrs = 20 (ratio %.3g)" % (before, after, M, after / before))
    assert after < before
    assert np.array_equal(alg.pts, Z[alg.idcs]) and len(set(alg.idcs.tolist())) == M
