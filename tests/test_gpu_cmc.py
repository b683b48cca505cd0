"""GPU: Coreset MCMC (bc.CoresetMCMC, csrc/hmc.hip cmc_advance_kernel / cmc_centre_kernel) against (1) the
existing coreset HMC kernel with the weights frozen, bit for bit, (2) the NumPy restatement teacher-forced over every transition
while the weights move, (3) the restatement of what the launch emits and of the weight step, (4) the shapes where its loops can
go wrong, (5) itself: reproducible, and continued by ``optimize()``, (6) failures that stick, (7) the point of it: it learns."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bayesian-coresets_amd", "examples", "common"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cmc_restatement as cr  # noqa: E402
import hmc_restatement as hr  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -53


@pytest.fixture(scope="module")
def bc():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import bayesiancoresets_amd as bc
    return bc


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "mcmc_golden.npz"))


def _rows(gold, family):
    return (gold["lr_Z"], 3) if family == "logistic" else (gold["poiss_Z"], 4)


def _synthetic(family, N, D, seed):
    """Seeded rows with a unit-scale linear predictor: logistic y x, Poisson [x, y]."""
    rs = np.random.RandomState(seed)
    X = np.hstack((rs.randn(N, D - 1), np.ones((N, 1)))) if D > 1 else np.ones((N, 1))
    th = rs.randn(D) / np.sqrt(D)
    if family == "logistic":
        return np.where(rs.rand(N) < 1.0 / (1.0 + np.exp(-X.dot(th))), 1.0, -1.0)[:, None] * X
    return np.hstack((X, rs.poisson(np.log1p(np.exp(X.dot(th)))).astype(np.float64)[:, None]))


def _build(bc, family, Z, M, seed, **kw):
    np.random.seed(seed)                    # (build draws the points, then the row tables, from NumPy's stream)
    build_kw = {k: kw.pop(k) for k in ("keep_trace", "_dev_noise") if k in kw}
    alg = bc.CoresetMCMC(Z, family, seed=seed, **kw)
    alg.build(M, **build_kw)
    return alg


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("thin", (1, 3))
def test_frozen_weights_equal_the_coreset_kernel(bc, gold, thin):
    """A schedule of zeros leaves the weights at N / M, and the K chains of T iterations x thin transitions are the chains of ONE
    bcx_hmc_coreset launch of T thin transitions with n_warmup = n_adapt thin on the same normals: the carried state, the target
    evaluated again at it, the life-long index of the dual averaging and the noise's layout, bit for bit."""
    import torch
    from bayesiancoresets_amd import _native
    lib = _native.load()
    Z, D = _rows(gold, "logistic")
    M, K, T, L, n_adapt = 30, 8, 24, 8, 10
    noise = torch.from_numpy(np.random.RandomState(5).randn(T, K, thin, D + 3)).cuda()
    alg = _build(bc, "logistic", Z, M, 3, chains=K, leapfrog=L, thin=thin, opt_itrs=T, n_subsample=64, step_sched=lambda i: 0.0,
                 n_adapt=n_adapt, keep_trace=True, _dev_noise=noise)
    tr = alg.trace
    assert np.all(alg.wts == Z.shape[0] / M) and np.all(tr["weights"] == Z.shape[0] / M)
    ld, TT = alg.ld, T * thin
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
    pts, w, mu, W = d(alg.pts), d(alg.wts), d(alg.result.center), d(alg.result.transform)
    flat = noise.permute(1, 0, 2, 3).reshape(K, TT, D + 3).contiguous()
    f64 = dict(dtype=torch.float64, device="cuda")
    samples, xis, props = (torch.empty(K, TT, ld, **f64) for _ in range(3))
    diag, acc, eps = torch.empty(K, TT, 6, **f64), torch.empty(K, **f64), torch.empty(K, **f64)
    status = torch.zeros(2, dtype=torch.int32, device="cuda")
    rc = lib.bcx_hmc_coreset(int(torch.cuda.current_stream().cuda_stream), 0, M, D, w.data_ptr(), pts.data_ptr(), pts.stride(0), mu.data_ptr(),
                             W.data_ptr(), D, K, n_adapt * thin, TT - n_adapt * thin, L, bc.DeviceHMC.STEP0, 0.0, flat.data_ptr(), ld,
                             samples.data_ptr(), xis.data_ptr(), props.data_ptr(), diag.data_ptr(), acc.data_ptr(), eps.data_ptr(),
                             status.data_ptr())
    assert rc == 0
    chainwise = lambda a: np.ascontiguousarray(a.transpose(1, 0, 2, 3)).reshape(K, TT, -1)
    assert np.array_equal(chainwise(tr["xi"]), xis[:, :, :D].cpu().numpy())
    assert np.array_equal(chainwise(tr["proposal"]), props[:, :, :D].cpu().numpy())
    assert np.array_equal(chainwise(tr["diag"]), diag.cpu().numpy())
    assert np.array_equal(chainwise(tr["theta"]), samples[:, :, :D].cpu().numpy())
    assert np.array_equal(alg.result.step_size, eps.cpu().numpy())
    assert 0.3 < tr["diag"][..., 1].mean() < 1.0 and status.cpu().numpy()[0] == 0     # (both outcomes occurred)


# ------------------------------------------------------------------------------------------------------------ 2, 3, 4
def _teacher_forced(alg, family, Z, D, L):
    """Every transition of the device run restarted in the restatement (long double: the referee; float64) from the device's
    previous xi, step and dual-averaging state at the device's weights of that iteration; then what the launch emitted and the
    weight step from the device's own V, s, weights.  Returns the device's and the float64 restatement's largest deviations
    from the referee per quantity in units of its scale, the wrong / too-close accept decisions, and the weight step's deviation."""
    tr = alg.trace
    T, K, thin = tr["diag"].shape[:3]
    N, M = Z.shape[0], alg.pts.shape[0]
    mu, Wm, eps0 = alg.result.center, alg.result.transform, tr["step0"]
    nad = alg.n_adapt * thin
    dev = dict(proposal=0.0, dH=0.0, eps=0.0, V=0.0, s=0.0)
    f64 = dict(proposal=0.0, dH=0.0, eps=0.0, V=0.0, s=0.0)
    wrong, close = 0, 0
    w = np.full(M, N / M)
    m1, m2 = np.zeros(M), np.zeros(M)
    step_dev = 0.0
    for i in range(T):
        tl = hr.Target(family, alg.pts, w, D, mu, Wm, np.longdouble)
        td = hr.Target(family, alg.pts, w, D, mu, Wm, np.float64)
        for c in range(K):
            for j in range(thin):
                prev = (i, c, j - 1) if j else (i - 1, c, thin - 1)
                xi = tr["xi"][prev] if i or j else np.zeros(D)
                base, hbar, lebar = tr["diag"][prev][3:6] if i or j else (eps0, 0.0, 0.0)
                z, got = tr["noise"][i, c, j], tr["diag"][i, c, j]
                rl, rd = hr.transition(tl, xi, z, base, L), hr.transition(td, xi, z, base, L)
                sp = max(1.0, float(np.abs(rl["proposal"]).max()))
                sh = max(1.0, float(abs(rl["H0"])), float(abs(rl["H1"])))
                dev["proposal"] = max(dev["proposal"], float(np.abs(tr["proposal"][i, c, j] - rl["proposal"]).max()) / sp)
                f64["proposal"] = max(f64["proposal"], float(np.abs(rd["proposal"] - rl["proposal"]).max()) / sp)
                dev["dH"] = max(dev["dH"], float(abs(got[0] - rl["dH"])) / sh)
                f64["dH"] = max(f64["dH"], float(abs(rd["dH"] - rl["dH"])) / sh)
                assert float(abs(got[2] - rl["eps_t"])) <= 32 * EPS * float(rl["eps_t"])
                life = (i * thin + j)
                if life < nad:
                    nl = hr.dual_average(life + 1, rl["dH"], hbar, lebar, eps0, life + 1 == nad, np.longdouble)[0]
                    nd = hr.dual_average(life + 1, rd["dH"], hbar, lebar, eps0, life + 1 == nad, np.float64)[0]
                    dev["eps"] = max(dev["eps"], float(abs(got[3] - nl) / nl))
                    f64["eps"] = max(f64["eps"], float(abs(nd - nl) / nl))
                else:
                    assert got[3] == base
                if abs(float(rl["dH"] - rl["e"])) > 1e-9 * max(1.0, float(rl["e"])):
                    wrong += bool(got[1] > 0.5) != rl["accepted"]
                else:
                    close += 1
                want = tr["proposal"][i, c, j] if got[1] > 0.5 else xi
                assert np.array_equal(tr["xi"][i, c, j], want)
        # what the launch emitted at the device's own states
        th = tr["theta"][i, :, thin - 1]
        rows = None if tr["table"] is None else tr["table"][i]
        Vl, sl, scale = cr.emit(family, alg.pts, Z, rows, th, D, np.longdouble)
        Vd, sd, _ = cr.emit(family, alg.pts, Z, rows, th, D, np.float64)
        sv = np.maximum(1.0, np.abs(Vl).astype(np.float64))
        dev["V"] = max(dev["V"], float((np.abs(tr["V"][i] - Vl).astype(np.float64) / sv).max()))
        f64["V"] = max(f64["V"], float((np.abs(Vd - Vl).astype(np.float64) / sv).max()))
        ss = float(scale.max())
        dev["s"] = max(dev["s"], float(np.abs(tr["s"][i] - sl).max()) / ss)
        f64["s"] = max(f64["s"], float(np.abs(sd - sl).max()) / ss)
        if K == 1:
            assert tr["s"][i, 0] == 0.0
        # the weight step from the device's own V, s, weights (moments carried here)
        scaling = 1.0 if rows is None else N / len(rows)
        w_next, m1, m2 = cr.adam_step(w, cr.gradient(tr["V"][i], tr["s"][i], w, scaling), m1, m2, i, tr["sched"][i, 0])
        step_dev = max(step_dev, float(np.abs(tr["weights"][i] - w_next).max()))
        np.testing.assert_allclose(tr["weights"][i], w_next, rtol=1e-9, atol=1e-12)      # (tests/test_gpu_svi.py's tolerance for the step)
        w = tr["weights"][i]
    assert np.array_equal(alg.wts, w)
    return dev, f64, wrong, close, step_dev


def _tolerances(f64):
    """16 x the float64 restatement's own deviation from the long-double one, per quantity, at least 32 ulp of the scale
    (the rule of tests/test_gpu_hmc.py)."""
    return {q: max(16.0 * f64[q], 32 * 2.0 ** -52) for q in f64}


def _check(what, dev, f64, wrong, close):
    tol = _tolerances(f64)
    for q in sorted(dev):
        print("%s %s: device %.3g, float64 restatement %.3g (ratio %.2f), tolerance %.3g"
              % (what, q, dev[q], f64[q], dev[q] / max(f64[q], 1e-300), tol[q]))
    for q in dev:
        assert dev[q] <= tol[q], (q, dev[q], tol[q])
    assert wrong == 0
    assert close <= 1


# Observed on an MI355X: DESIGN.md 4.21.
@pytest.mark.parametrize("family", ("logistic", "poisson"))
def test_moving_weights_equal_restatement(bc, gold, family):
    """M = 40, K = 16, thin = 2, leapfrog = 4, T = 30, 64 of 900 rows per iteration: proposals, dH and next steps (2), V, the centred
    s and the weights after every step (3).  dH agrees only if H0 was taken at the iteration's weights."""
    Z, D = _rows(gold, family)
    alg = _build(bc, family, Z, 40, 7, chains=16, leapfrog=4, thin=2, opt_itrs=30, n_subsample=64, keep_trace=True)
    assert alg.status in (0, 1) and alg.trace["table"].shape == (30, 64)
    dev, f64, wrong, close, step_dev = _teacher_forced(alg, family, Z, D, 4)
    print("%s: largest deviation of a weight after its step %.3g; weights moved by up to %.3g" %
          (family, step_dev, np.abs(alg.wts - 900 / 40).max()))
    _check(family, dev, f64, wrong, close)
    assert not np.array_equal(alg.trace["weights"][0], alg.trace["weights"][-1])          # (the weights did move)
    acc = alg.trace["diag"][..., 1].mean()
    print("%s: acceptance rate %.3f" % (family, acc))
    assert 0.5 < acc < 0.99, acc
    wts, pts, idcs = alg.get()
    assert np.array_equal(pts, Z[idcs]) and (wts > 0).all() and alg.error() == 0.0
    assert alg.samples().shape == (16, 15, D) and alg.samples(burn=0).shape == (16, 30, D)
    assert np.array_equal(alg.samples(burn=0), alg.trace["theta"][:, :, 1].transpose(1, 0, 2))
    res = alg.result
    assert res.samples.shape == (16, 15, D) and res.accept_rate.shape == (16,) and res.step_size.shape == (16,) and res.rhat.shape == (D,)
    assert res.delta_h.shape == (16, 30) and res.accepted.shape == (16, 30)


_SHAPES = (
    # family, N, M, D, K, n_sub (None: all rows; "repeat": more draws than rows)
    ("logistic", 900, 1, 3, 3, 1),
    ("poisson", 900, 7, 1, 3, 257),
    ("logistic", 900, 300, 3, 3, None),
    ("poisson", 900, 7, 32, 1, 257),
    ("logistic", 900, 300, 32, 3, 1),
    ("poisson", 900, 7, 3, 1, None),
    ("logistic", 20, 7, 3, 3, "repeat"),
)


@pytest.mark.parametrize("family,N,M,D,K,n_sub", _SHAPES)
def test_shapes_where_the_loops_can_go_wrong(bc, family, N, M, D, K, n_sub):
    """Teacher-forced for 3 iterations: one point, points past one pass of the 256 threads, D = 1 and D = 32, one chain (the centred
    s and the gradient are zero), one gathered row, rows past one pass, every row without a table, a table that repeats rows."""
    Z = _synthetic(family, N, D, 100 * M + D)
    repeat = n_sub == "repeat"
    alg = _build(bc, family, Z, M, 11, chains=K, leapfrog=3, thin=2, opt_itrs=3, n_subsample=257 if repeat else n_sub, n_adapt=2,
                 keep_trace=True)
    if repeat:
        assert all(len(set(r.tolist())) < len(r) for r in alg.trace["table"])
    if n_sub is None:
        assert alg.trace["table"] is None
    dev, f64, wrong, close, step_dev = _teacher_forced(alg, family, Z, D, 3)
    _check("%s N %d M %d D %d K %d n_sub %s" % (family, N, M, D, K, n_sub), dev, f64, wrong, close)
    if K == 1:
        assert np.all(alg.wts == N / M)


def test_points_that_do_not_fit_raise_before_any_launch(bc):
    from bayesiancoresets_amd import _native
    lib = _native.load()
    Z = _synthetic("logistic", 4200, 32, 1)
    assert lib.bcx_cmc_advance_ok(300, 32) and not lib.bcx_cmc_advance_ok(4096, 32) and not lib.bcx_cmc_advance_ok(0, 3)
    assert not lib.bcx_cmc_advance_ok(4097, 1) and not lib.bcx_cmc_advance_ok(10, 33)
    alg = bc.CoresetMCMC(Z, "logistic", chains=4, opt_itrs=2)
    for M in (4096, 4097):
        with pytest.raises(ValueError):
            alg.build(M)
        assert alg.size() == 0 and alg._run_state is None
    # the entry point's own argument check
    assert lib.bcx_cmc_advance(None, 0, 4096, 32, None, None, 33, None, None, 32, 4, 1, 1, 0.5, 0, 0, 1, None, None, None, 10, 33, None, 0,
                               None, 4, None, 32, None, None, None, None, None) == _native.ERR_ARG


# ---------------------------------------------------------------------------------------------------------------- 5
def test_reproducible_and_continued(bc, gold):
    Z, D = _rows(gold, "poisson")
    kw = dict(chains=8, leapfrog=4, thin=2, n_subsample=50, n_adapt=10)
    a = _build(bc, "poisson", Z, 25, 9, opt_itrs=40, **kw)
    b = _build(bc, "poisson", Z, 25, 9, opt_itrs=40, **kw)
    assert np.array_equal(a.wts, b.wts) and np.array_equal(a.samples(burn=0), b.samples(burn=0)) and np.array_equal(a.idcs, b.idcs)
    np.random.seed(9)                                                      # (the same points and tables, another noise seed)
    c = bc.CoresetMCMC(Z, "poisson", seed=10, opt_itrs=40, **kw)
    c.build(25)
    assert np.array_equal(a.idcs, c.idcs) and not np.array_equal(a.wts, c.wts) and not np.array_equal(a.samples(burn=0), c.samples(burn=0))
    # 20 + 20 iterations are the 40
    h = _build(bc, "poisson", Z, 25, 9, opt_itrs=20, **kw)
    assert not np.array_equal(h.wts, a.wts)
    h.optimize()
    assert np.array_equal(h.wts, a.wts) and np.array_equal(h.samples(burn=0), a.samples(burn=0))
    assert np.array_equal(h.result.step_size, a.result.step_size) and np.array_equal(h.result.delta_h, a.result.delta_h)
    assert h.samples().shape == (8, 30, D)


# ---------------------------------------------------------------------------------------------------------------- 6
def test_failures_stick(bc, gold):
    """A NaN in a coreset point: every launch's log joint at its start is not finite, the status word says so, and the loop ends in
    EngineError.  (The point is poisoned on the device behind ``build``: the Laplace fit of the frame would refuse it first.)
    Nothing else runs on the device in this test after it."""
    from bayesiancoresets_amd import _native
    Z, D = _rows(gold, "logistic")
    np.random.seed(4)
    alg = bc.CoresetMCMC(Z, "logistic", chains=4, leapfrog=2, opt_itrs=0, n_subsample=16, seed=4)
    alg.build(12)
    assert alg.size() == 12 and np.all(alg.wts == 900 / 12)
    alg._run_state["pts"][5, 1] = float("nan")
    alg.opt_itrs = 3
    with pytest.raises(_native.EngineError) as e:
        alg._optimize()
    assert e.value.code == _native.ERR_STATE and alg.status == 2


# ---------------------------------------------------------------------------------------------------------------- 7
# Observed on an MI355X: DESIGN.md 4.21.
@pytest.mark.parametrize("seed", (1, 2, 3))
def test_it_learns(bc, seed):
    """The host test's problem on the device (tests/test_cmc_host.py: logistic, N = 2000, D = 3, M = 20, 8 leapfrog steps, 200 rows
    per iteration), K = 16, T = 200: the Laplace KL of the learned coreset is at most 1/10 of the uniform one's, and split-R-hat of
    ``samples()`` is below 1.2 in every coordinate."""
    import model_lr
    from test_cmc_host import laplace_kl
    N, D, M = 2000, 3, 20
    rs = np.random.RandomState(seed)
    X = rs.randn(N, D)
    Z = np.where(rs.rand(N) < 1.0 / (1.0 + np.exp(-X.sum(axis=1))), 1.0, -1.0)[:, None] * X
    alg = _build(bc, "logistic", Z, M, seed, chains=16, leapfrog=8, opt_itrs=200, n_subsample=200)
    full = model_lr.laplace_fit(Z, None)
    before, after = laplace_kl(Z, alg.pts, np.full(M, N / M), full), laplace_kl(Z, alg.pts, alg.wts, full)
    rhat = alg.result.rhat
    print("seed %d: Laplace KL uniform %.4g, learned %.4g (factor %.1f); split R-hat %s; accept rate %.2f"
          % (seed, before, after, before / after, np.array2string(rhat, precision=3), alg.result.accept_rate.mean()))
    assert after <= before / 10.0
    assert alg.samples().shape == (16, 100, D) and np.all(rhat < 1.2), rhat
