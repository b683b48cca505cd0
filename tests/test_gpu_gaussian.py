"""GPU: the device projector's Gaussian-mean family (csrc/proj.hip FAM_GAUSSIAN, csrc/gauss.hip, csrc/psvi.hip PS_GAUSSIAN) and
bc.GaussianPosteriorSampler against the reference's values (fixture F18, tests/golden/gaussian_device_golden.npz) and against
np.longdouble evaluations; tolerances are those of tests/test_gpu_projection.py / tests/test_gpu_bpsvi.py."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bayesian-coresets_amd"))
sys.path.insert(1, os.path.join(ROOT, "bayesian-coresets_amd", "examples", "common"))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bc():
    import bayesiancoresets_amd as m
    return m


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(ROOT, "tests", "golden", "gaussian_device_golden.npz"))


def truth(x, th, Siginv):
    """The centred log-likelihoods in 80-bit arithmetic (the literal form: x . Siginv theta - theta' Siginv theta / 2, centred)."""
    L = np.longdouble
    x, th, Sg = x.astype(L), th.astype(L), Siginv.astype(L)
    gs = th.dot(Sg)
    v = x.dot(gs.T) - 0.5 * (th * gs).sum(axis=1)
    return (v - v.mean(axis=1)[:, None])


def close(got, want, rtol, floor):
    want = np.asarray(want, dtype=np.float64)
    atol = floor * float(np.abs(want).max()) if want.size else 0.0
    err = np.abs(np.asarray(got, dtype=np.float64) - want) - (atol + rtol * np.abs(want))
    print("max |got - want| = %.3e, largest entry %.3e, worst margin %.3e" % (
        float(np.abs(got - want).max()) if want.size else 0.0, float(np.abs(want).max()) if want.size else 0.0, float(err.max()) if want.size else 0.0))
    assert (err <= 0).all()


def fixed(th):
    return lambda n, w, p: th


def spd(rs, D):
    A = rs.randn(D, D)
    return A.dot(A.T) / D + 0.5 * np.eye(D)


def make(rs, N, D, S, full):
    """Data around a mean far from 0 and draws tight around it, as a posterior at large N gives."""
    Siginv = spd(rs, D) if full else None
    centre = 3.0 + rs.rand(D)
    x = centre + rs.randn(N, D)
    th = centre + 0.05 * rs.randn(S, D)
    return x, th, Siginv


# ---- projection -------------------------------------------------------------------------------------------------------------------
def test_project_matches_the_reference_fixture(bc, g):
    Siginv = np.linalg.inv(g["Sig"])
    prj = bc.DeviceProjector("gaussian", fixed(g["th"]), g["th"].shape[0], Siginv=Siginv)
    close(prj.project(g["x"]).cpu().numpy(), g["proj_x"], 1e-11, 1e-12)
    close(prj.project(g["P"]).cpu().numpy(), g["proj_P_lls"], 1e-11, 1e-12)


@pytest.mark.parametrize("N,D,S,full", ((1, 5, 7, True), (3, 6, 64, False), (4095, 33, 100, True), (4097, 200, 100, False),
                                        (4097, 301, 130, True), (300, 17, 256, True), (300000, 20, 64, True)))
def test_project_matches_long_double(bc, N, D, S, full):
    rs = np.random.RandomState(N + D)
    x, th, Siginv = make(rs, N, D, S, full)
    prj = bc.DeviceProjector("gaussian", fixed(th), S, Siginv=Siginv)
    want = truth(x, th, np.eye(D) if Siginv is None else Siginv).astype(np.float64)
    close(prj.project(x).cpu().numpy(), want, 1e-11, 1e-12)
    if N <= 4097:
        import torch
        xt = torch.from_numpy(np.hstack((x, np.zeros((N, 3))))).cuda()[:, :D]         # a strided device tensor
        close(prj.project(xt).cpu().numpy(), want, 1e-11, 1e-12)
        raw = prj.project_uncentred(x).cpu().numpy()
        close(raw - raw.mean(axis=1)[:, None], want, 1e-11, 1e-12)


@pytest.mark.parametrize("N,D,S,full", ((3, 6, 64, False), (4097, 33, 100, True), (20000, 200, 100, False), (300000, 21, 192, True)))
def test_colsum_and_select(bc, N, D, S, full):
    rs = np.random.RandomState(7 * N + D)
    x, th, Siginv = make(rs, N, D, S, full)
    want = truth(x, th, np.eye(D) if Siginv is None else Siginv)
    wsum = want.sum(axis=0).astype(np.float64)
    cols = {}
    for mode in ("mfma", "moments", "auto"):
        prj = bc.DeviceProjector("gaussian", fixed(th), S, Siginv=Siginv, colsum=mode)
        for _ in range(3):                                   # ("auto" forms the closed form on the second sight of the data)
            cols[mode] = prj.project_colsum(x)
            np.testing.assert_allclose(cols[mode], wsum, rtol=1e-9, atol=1e-9 * np.abs(wsum).max())
        if N >= 4096 and mode != "mfma":
            assert prj.moments_info.get("rows") == N and (mode == "moments" or prj.moments_info["accepted"])
    assert np.abs(cols["mfma"] - cols["moments"]).max() <= 1e-10 * np.abs(wsum).max()
    resid = rs.randn(S)
    w64 = want.astype(np.float64)
    corrs = w64.dot(resid) / np.sqrt((w64 ** 2).sum(axis=1)) / S
    best, row = prj.project_select(x, resid)
    assert row == int(np.argmax(corrs))
    np.testing.assert_allclose(best, corrs.max(), rtol=1e-7)
    col, core = prj.colsum_and_core(x, x[:5])
    np.testing.assert_allclose(col, wsum, rtol=1e-9, atol=1e-9 * np.abs(wsum).max())
    close(core, w64[:5], 1e-11, 1e-12)


@pytest.mark.parametrize("S", (1, 64))
def test_select_zero_vector_is_numpys_nan_pick(bc, S):
    rs = np.random.RandomState(2)
    x = 1.0 + rs.randn(500, 6)
    th = np.repeat(rs.randn(1, 6), S, axis=0)               # all draws equal: every projected vector is zero
    prj = bc.DeviceProjector("gaussian", fixed(th), S)
    vecs = prj.project(x).cpu().numpy()
    assert not vecs.any()
    resid = rs.randn(S)
    with np.errstate(invalid="ignore", divide="ignore"):
        corrs = vecs.dot(resid) / np.sqrt((vecs ** 2).sum(axis=1)) / S
    best, row = prj.project_select(x, resid)
    assert row == int(np.argmax(corrs)) == 0 and np.isnan(best)


def test_family_3_is_refused_where_it_is_not_implemented(bc):
    import torch
    from bayesiancoresets_amd import _native
    lib = _native.load()
    t = torch.zeros(64, 8, dtype=torch.float64, device="cuda")
    rc = lib.bcx_project_grad_points(0, 3, t.data_ptr(), 4, 8, 6, -1, t.data_ptr(), 8, 8, 1.0, t.data_ptr(), t.data_ptr())
    assert rc == _native.ERR_ARG and b"family 3" in lib.bcx_project_last_error()
    rc = lib.bcx_project_write(0, 3, t.data_ptr(), 4, 8, 8, -1, t.data_ptr(), 8, 8, 1.0, t.data_ptr(), 8, None)   # ldt < D + 1
    assert rc == _native.ERR_ARG
    rc = lib.bcx_project_write(0, 4, t.data_ptr(), 4, 8, 6, -1, t.data_ptr(), 8, 8, 1.0, t.data_ptr(), 8, None)
    assert rc == _native.ERR_ARG and b"unknown" in lib.bcx_project_last_error()


# ---- pseudo-point gradients ---------------------------------------------------------------------------------------------------------
def test_project_grad_matches_the_reference_fixture(bc, g):
    import torch
    Siginv = np.linalg.inv(g["Sig"])
    prj = bc.DeviceProjector("gaussian", fixed(g["th"]), g["th"].shape[0], Siginv=Siginv)
    for P in (g["P"], torch.from_numpy(np.hstack((g["P"], np.ones((g["P"].shape[0], 2))))).cuda()[:, :6]):
        lls, glls = prj.project(P, grad=True)
        close(lls.cpu().numpy(), g["proj_P_lls"], 1e-11, 1e-12)
        close(glls.cpu().numpy(), g["proj_P_glls"], 1e-12, 1e-12)
    again = prj.project(g["P"], grad=True)[1]
    assert torch.equal(again, prj.project(g["P"], grad=True)[1])


@pytest.mark.parametrize("k,D,S,full", ((7, 6, 40, True), (1, 5, 3, False), (70, 33, 100, True), (300, 200, 100, False)))
def test_psvi_gradient_is_the_literal_bpsvi_gradient(bc, k, D, S, full):
    import torch
    rs = np.random.RandomState(k + D)
    x, th, Siginv = make(rs, 5000, D, S, full)
    Sg = np.eye(D) if Siginv is None else Siginv
    P, w = x[:k] + 0.1 * rs.randn(k, D), rs.rand(k) * 5000.0 / k
    vecs, corevecs = truth(x, th, Sg).astype(np.float64), truth(P, th, Sg).astype(np.float64)
    pgrads = th.dot(Sg)[None, :, :] - P.dot(Sg)[:, None, :]
    pgrads = pgrads - pgrads.mean(axis=2)[:, :, None]
    scaling = 1.7
    resid = scaling * vecs.sum(axis=0) - w.dot(corevecs)                                                       # bpsvi.py:51-53
    wgrad = -corevecs.dot(resid) / corevecs.shape[1]
    ugrad = -(w[:, None, None] * pgrads * resid[None, :, None]).sum(axis=1) / corevecs.shape[1]
    prj = bc.DeviceProjector("gaussian", fixed(th), S, Siginv=Siginv)
    outs = []
    for Pin in (P, torch.from_numpy(np.hstack((P, np.ones((k, 1))))).cuda()[:, :D]):
        wg, ug = prj.psvi_gradient(x, Pin, w, scaling)
        close(wg, wgrad, 1e-10, 1e-12)
        close(ug, ugrad, 1e-10, 1e-12)
        outs.append((wg, ug))
    # (colsum "auto" takes the closed-form column sums from the second sight of the data on: compare two calls that both do)
    wg2, ug2 = prj.psvi_gradient(x, P, w, scaling)
    wg3, ug3 = prj.psvi_gradient(x, P, w, scaling)
    assert np.array_equal(wg2, wg3) and np.array_equal(ug2, ug3)
    fix = bc.DeviceProjector("gaussian", fixed(th), S, Siginv=Siginv, colsum="mfma")
    a, b = fix.psvi_gradient(x, P, w, scaling), fix.psvi_gradient(x, P, w, scaling)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_psvi_limits_are_errors(bc):
    from bayesiancoresets_amd import _native
    rs = np.random.RandomState(0)
    th = rs.randn(8, 4)
    prj = bc.DeviceProjector("gaussian", fixed(th), 8)
    with pytest.raises(ValueError):
        prj.psvi_gradient(rs.randn(100, 4), rs.randn(4097, 4), np.ones(4097))
    lib = _native.load()
    assert lib.bcx_psvi_gradient_gaussian(0, 1, 8193, 6, 4, 1, 4, 6, 1, 1, 8193, 1, 1.0, 1, 1) == _native.ERR_ARG
    assert lib.bcx_project_grad_points_gaussian(0, 1, 8, 6, 4, 1, 4097, 6, 1, 1) == _native.ERR_ARG
    assert lib.bcx_project_grad_points_gaussian(0, 1, 8, 6, 1025, 1, 4, 6, 1, 1) == _native.ERR_ARG


# ---- the posterior sampler ------------------------------------------------------------------------------------------------------------
class _Replay(object):
    def __init__(self, inner, noise):
        self.inner, self.noise, self.at = inner, noise, 0
        inner._noise, inner._noise_block = self._one, self._block

    def _one(self, n):
        self.at += 1
        return self.noise[self.at - 1]

    def _block(self, steps, n):
        self.at += steps
        return self.noise[self.at - steps:self.at]

    def __call__(self, n, wts, pts):
        return self.inner(n, wts, pts)

    def enqueue_plan(self, n, pts, steps):
        return self.inner.enqueue_plan(n, pts, steps)


@pytest.mark.parametrize("k,D,zero", ((0, 6, False), (4, 6, False), (300, 6, False), (5, 7, True), (3, 33, False)))
def test_sampler_mean_and_factor(bc, k, D, zero):
    import torch
    import model_gaussian
    rs = np.random.RandomState(40 + k + D)
    mu0, Sig0inv, Siginv = 0.3 * rs.randn(D), spd(rs, D), spd(rs, D)
    S = 50
    R = rs.randn(S, D + D % 2)
    smp = bc.GaussianPosteriorSampler(mu0, Sig0inv, Siginv)
    smp._noise = lambda n: torch.from_numpy(R).cuda()
    pts, w = 1.0 + rs.randn(k, D), (np.zeros(k) if zero else rs.rand(k) * 10.0)
    theta = smp(S, w, pts).cpu().numpy()
    mu, U = model_gaussian.weighted_posterior(mu0, Sig0inv, Siginv, pts if k else np.zeros((1, D)), w if k else np.zeros(1))
    prec = Sig0inv + w.sum() * Siginv
    np.testing.assert_allclose(np.linalg.solve(prec, Sig0inv.dot(mu0) + Siginv.dot((w[:, None] * pts).sum(axis=0))), mu, rtol=1e-9, atol=1e-12)
    F = smp.W / np.sqrt(smp.lam + w.sum())                      # the sampler's factor: F F' = Sigma_w
    np.testing.assert_allclose(F.dot(F.T), np.linalg.inv(prec), rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(theta - mu, R[:, :D].dot(F.T), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(smp.mean.cpu().numpy(), theta.mean(axis=0), rtol=1e-10, atol=1e-12)


def test_sampler_statistics_and_errors(bc):
    import model_gaussian
    from bayesiancoresets_amd import _native
    rs = np.random.RandomState(5)
    D = 6
    mu0, Sig0inv, Siginv = 0.3 * rs.randn(D), spd(rs, D), spd(rs, D)
    smp = bc.GaussianPosteriorSampler(mu0, Sig0inv, Siginv, seed=3)
    pts, w = 1.0 + rs.randn(5, D), rs.rand(5) * 4.0
    draws = np.vstack([smp(4000, w, pts).cpu().numpy() for _ in range(5)])
    mu, U = model_gaussian.weighted_posterior(mu0, Sig0inv, Siginv, pts, w)
    se = np.sqrt(np.diag(U.dot(U.T)) / draws.shape[0])
    assert (np.abs(draws.mean(axis=0) - mu) <= 6.0 * se).all()
    np.testing.assert_allclose(np.cov(draws.T), U.dot(U.T), atol=0.1 * np.abs(U.dot(U.T)).max())
    with pytest.raises(_native.EngineError):
        smp(8, np.array([-(smp.lam.min() + 1.0), 0.0]), pts[:2])
    with pytest.raises(_native.EngineError):
        smp(8, np.array([1.0, np.nan]), pts[:2])
    assert np.isfinite(smp(8, w, pts).cpu().numpy()).all()                  # (and the sampler is usable again)


# ---- end to end against the reference's runs -------------------------------------------------------------------------------------------
def _reference_sampler(g):
    import model_gaussian
    mu0, Sig0inv, Siginv = g["mu0"], g["Sig0inv"], np.linalg.inv(g["Sig"])

    def sampler_w(n, wts, pts):                                             # examples/gaussian/main.py:107-112
        if wts is None or pts is None or np.asarray(pts).shape[0] == 0:
            wts, pts = np.zeros(1), np.zeros((1, mu0.shape[0]))
        mu, U = model_gaussian.weighted_posterior(mu0, Sig0inv, Siginv, np.atleast_2d(pts), np.asarray(wts, dtype=np.float64))
        return mu + np.random.randn(n, mu.shape[0]).dot(U.T)
    return sampler_w, Siginv


def test_sparsevi_reproduces_the_reference_run(bc, g):
    smp, Siginv = _reference_sampler(g)
    np.random.seed(5)
    alg = bc.SparseVICoreset(g["x"], bc.DeviceProjector("gaussian", smp, 50, Siginv=Siginv), opt_itrs=12, step_sched=lambda i: 1.0 / (1.0 + i))
    for t in range(g["svi_wts_steps"].shape[0]):
        alg.build(1)
        k = alg.wts.shape[0]
        assert np.array_equal(alg.idcs, g["svi_idcs_order"][:k]), (t, alg.idcs)
        np.testing.assert_allclose(alg.wts, g["svi_wts_steps"][t, :k], rtol=1e-5, atol=1e-8)
        assert not g["svi_wts_steps"][t, k:].any()


@pytest.mark.parametrize("tag,nsub", (("full", None), ("sub", 100)))
def test_bpsvi_reproduces_the_reference_run(bc, g, tag, nsub):
    smp, Siginv = _reference_sampler(g)
    np.random.seed(9)
    alg = bc.BatchPSVICoreset(g["x"], bc.DeviceProjector("gaussian", smp, 50, Siginv=Siginv), opt_itrs=30, n_subsample_opt=nsub,
                              step_sched=lambda i: 0.5 / (1.0 + i))
    alg.build(8)
    np.testing.assert_allclose(alg.wts, g["psvi_%s_wts" % tag], rtol=1e-7)
    np.testing.assert_allclose(alg.pts, g["psvi_%s_pts" % tag], rtol=1e-6, atol=1e-8)


def test_hilbert_giga_reproduces_the_reference_run(bc, g):
    import model_gaussian
    Siginv = np.linalg.inv(g["Sig"])
    x = g["x"]
    mup, Up = model_gaussian.weighted_posterior(g["mu0"], g["Sig0inv"], Siginv, x, np.ones(x.shape[0]))
    np.random.seed(3)
    prj = bc.DeviceProjector("gaussian", lambda n, w, p: mup + np.random.randn(n, 6).dot(Up.T), 50, Siginv=Siginv)
    h = bc.HilbertCoreset(x, prj)
    h.build(10)
    wts, pts, idcs = h.get()
    assert np.array_equal(idcs, g["giga_idcs"])
    np.testing.assert_allclose(wts, g["giga_wts"], rtol=1e-5)


@pytest.mark.parametrize("colsum", ("mfma", "moments"))
def test_enqueued_loop_matches_the_host_loop(bc, colsum):
    import torch
    D, N, S, T, steps = 12, 20000, 64, 30, 3
    rs = np.random.RandomState(11)
    Siginv, Sig0inv, mu0 = spd(rs, D), spd(rs, D), 0.1 * rs.randn(D)
    x = 1.0 + rs.randn(N, D)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(17)
    noise = torch.randn(steps * (T + 1) + 4 + T, S, D + D % 2, dtype=torch.float64, device="cuda", generator=gen)
    out = {}
    for mode in (True, False):
        smp = _Replay(bc.GaussianPosteriorSampler(mu0, Sig0inv, Siginv), noise)
        alg = bc.SparseVICoreset(x, bc.DeviceProjector("gaussian", smp, S, Siginv=Siginv, colsum=colsum), opt_itrs=T)
        alg.ENQUEUE = mode
        alg.build(steps)
        out[mode] = (alg.wts.copy(), alg.idcs.copy(), alg.pts.copy(), smp.at)
        if mode:
            assert alg._enqueue_plan() is not None                          # (the enqueued path is the one that ran)
    assert out[True][3] == out[False][3] == 1 + steps * (T + 1)
    assert np.array_equal(out[True][1], out[False][1]) and out[True][1].shape[0] >= 2
    assert np.array_equal(out[True][2], out[False][2])
    np.testing.assert_allclose(out[True][0], out[False][0], rtol=1e-8, atol=1e-12)
    assert (out[True][0] > 0).any()


# ---- two ranks sharing the GPU -------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _shard_worker(rank, world, port, out_dir):
    for p in (ROOT, os.path.join(ROOT, "bayesian-coresets_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import bayesiancoresets_amd as bc
    rs = np.random.RandomState(8)
    N, D, S = 9001, 11, 70
    x, th, Siginv = make(rs, N, D, S, True)
    resid = rs.randn(S)
    per = (N + world - 1) // world
    lo, hi = rank * per, min(N, (rank + 1) * per)
    res = {}
    for mode in ("mfma", "moments"):
        prj = bc.DeviceProjector("gaussian", fixed(th), S, Siginv=Siginv, colsum=mode, group=dist.group.WORLD, row_offset=lo)
        shard = x[lo:hi]
        res["col_" + mode] = prj.project_colsum(shard)
        best, row = prj.project_select(shard, resid)
        res["sel_" + mode] = np.array([best, row])
    np.savez(os.path.join(out_dir, "gs_w%d_r%d.npz" % (world, rank)), **res)
    dist.barrier()
    dist.destroy_process_group()


def test_two_shards_equal_one(tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_shard_worker, args=(1, _free_port(), str(tmp_path)), nprocs=1, join=True)
    mp.spawn(_shard_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    ref = np.load(tmp_path / "gs_w1_r0.npz")
    for rank in range(2):
        r = np.load(tmp_path / ("gs_w2_r%d.npz" % rank))
        for mode in ("mfma", "moments"):
            scale = np.abs(ref["col_" + mode]).max()
            np.testing.assert_allclose(r["col_" + mode], ref["col_" + mode], rtol=1e-9, atol=1e-10 * scale)
            assert r["sel_" + mode][1] == ref["sel_" + mode][1]
            np.testing.assert_allclose(r["sel_" + mode][0], ref["sel_" + mode][0], rtol=1e-7)


# ---- the example ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ("SVI", "GIGA-OPT", "GIGA-REAL", "PSVI"))
def test_gaussian_example_cli_device_projector(tmp_path, alg):
    """The sizes of tests/test_gaussian_model.py::test_gaussian_example_cli.  PSVI gets a step schedule of its own, 0.1 / (1 + i):
    projected ADAM moves every coordinate of every pseudo-point by about the step size, and the harness default of 1 / (1 + i)
    -- the spread of the data itself -- throws the M = 30 points further from the data mean than they started; the REFERENCE's
    BatchPSVICoreset on the CPU, same sizes and seed, ends at a forward KL of 859 with the default against 69.3 for the empty
    coreset, and at 37.4 with 0.1 / (1 + i)."""
    import pandas as pd
    script = os.path.join(ROOT, "bayesian-coresets_amd", "examples", "gaussian", "main.py")
    folder = str(tmp_path / "results") + "/"
    cmd = [sys.executable, script, "--alg", alg, "--projector", "device", "--trial", "1", "--data_num", "1000", "--data_dim", "20",
           "--proj_dim", "60", "--coreset_size_max", "30", "--coreset_num_sizes", "4", "--opt_itrs", "15", "--results_folder", folder, "run"]
    if alg == "PSVI":
        cmd[-1:-1] = ["--step_sched", "lambda i : 0.1/(1+i)"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    files = [f for f in os.listdir(folder) if f != "manifest.csv"]
    assert len(files) == 1
    t = pd.read_csv(os.path.join(folder, files[0]))
    for col in ("csizes", "Ms", "cputs", "rklw", "fklw", "mu_errs", "Sig_errs"):
        assert col in t.columns, col
    assert t["Ms"].iloc[0] == 0 and t["csizes"].iloc[0] == 0
    assert np.isfinite(t["rklw"]).all() and np.isfinite(t["fklw"]).all()
    assert t["csizes"].iloc[-1] >= 1
    print(alg, "forward KL", list(t["fklw"]))
    assert t["fklw"].iloc[-1] < t["fklw"].iloc[0]
