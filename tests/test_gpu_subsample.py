"""GPU: the fused consumers on INDEXED rows of a standing data set (csrc/proj.hip GATHER instantiations, ``DeviceProjector``'s
``rows=``) and the ``subsample="device"`` paths of SparseVICoreset / BatchPSVICoreset.

The gathered kernel only changes addresses, so everything it returns has to equal, bit for bit, what the contiguous entry returns on
a device copy of the indexed rows with the same leading dimension; the coresets' sub-sampled host loops therefore reproduce the
default ones exactly, and the sub-sampled enqueued loops are held to the host loops by the tolerances the full-data enqueued loops
already have (tests/test_gpu_svi.py:403, tests/test_gpu_bpsvi_loop.py:29)."""
import numpy as np
import pytest

import bayesiancoresets_amd as bc
from bayesiancoresets_amd import _native
from models import (logistic_log_likelihood, poisson_log_likelihood, linreg_log_likelihood, make_linreg_data, make_poisson_data,
                    linreg_sampler)
from lr_workload import make_data as make_lr_data
from test_gpu_bpsvi_loop import W_RTOL, P_RTOL, P_ATOL, _ReplaySampler, _noise, _model, _report
from test_bpsvi_host import LR, golden, linreg_run_inputs

pytestmark = pytest.mark.gpu

FAMILIES = ("logistic", "poisson", "linreg", "gaussian")
N_STANDING = 50000


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _data(family, D, seed=3):
    """(Z, number of parameters): N_STANDING rows of D features, with the family's response column where it has one."""
    if family == "logistic":
        return make_lr_data(seed, N_STANDING, D), D
    if family == "poisson":
        return make_poisson_data(seed, N_STANDING, D), D
    if family == "linreg":
        return make_linreg_data(seed, N_STANDING, D), D
    return 1.0 + np.random.RandomState(seed).randn(N_STANDING, D), D


def _projector(family, theta, **kw):
    if family == "gaussian":
        rs = np.random.RandomState(1)
        A = rs.randn(theta.shape[1], theta.shape[1])
        kw["Siginv"] = A.dot(A.T) / theta.shape[1] + np.eye(theta.shape[1])
    return bc.DeviceProjector(family, lambda n, w, p: theta, theta.shape[0], sigsq=0.7, **kw)


def _index_arrays(rs, n_rows):
    idx = rs.randint(N_STANDING, size=n_rows)
    out = [("randint", idx)]
    if n_rows == 4097:
        out += [("sorted", np.sort(idx)), ("reversed", np.sort(idx)[::-1].copy()), ("all-equal", np.full(n_rows, idx[0]))]
    return out


# ---- 1. the gathered consumers are the copy's, bit for bit -----------------------------------------------------------------------------
@pytest.mark.parametrize("force_copy", (False, True))
@pytest.mark.parametrize("D", (10, 33))
@pytest.mark.parametrize("family", FAMILIES)
def test_gathered_consumers_equal_the_copys_bit_for_bit(family, D, force_copy, monkeypatch):
    """D = 10: the rows of logistic / gaussian data are 16-byte aligned (even leading dimension) and those of poisson / linreg
    (D + 1 columns) are not; D = 33 the other way round -- both request paths of every family.  S = 256 makes the planner pick
    the 128-column tile where the family has one, S = 100 the 64-column one.  ``force_copy``: the fallback (device gather + the
    contiguous entry) through the same assertions."""
    torch = _torch()
    Zh, Dp = _data(family, D)
    Z = torch.from_numpy(Zh).cuda()
    rs = np.random.RandomState(7)
    monkeypatch.setattr(bc.DeviceProjector, "ROWS_FORCE_COPY", force_copy)
    sizes = (1, 127, 128, 129, 4097, 20000) if not force_copy else (129, 4097)
    for S in (8, 64, 100, 256):
        theta = 0.3 * rs.randn(S, Dp)
        resid = rs.randn(S)
        prj = _projector(family, theta, colsum="mfma")
        for n_rows in sizes:
            for tag, idx in _index_arrays(rs, n_rows):
                if n_rows >= 4097 and tag == "randint":
                    assert np.unique(idx).size < idx.size                      # duplicates present: the case is not vacuous
                it = torch.from_numpy(idx).cuda()
                copy = Z[it]                                                   # gathered on the device, same leading dimension
                assert copy.stride(0) == Z.stride(0)
                got = prj.gather_rows(Z, idx)
                assert torch.equal(got, copy), (family, S, n_rows, tag)
                want_col = prj.project_colsum(copy)
                for rows in (idx, it):
                    assert np.array_equal(prj.project_colsum(Z, rows=rows), want_col), (family, S, n_rows, tag)
                want_sel = prj.project_select(copy, resid)
                got_sel = prj.project_select(Z, resid, rows=idx)
                assert got_sel[1] == want_sel[1] and (got_sel[0] == want_sel[0] or (np.isnan(got_sel[0]) and np.isnan(want_sel[0]))), \
                    (family, S, n_rows, tag, got_sel, want_sel)
                if tag == "all-equal":
                    assert got_sel[1] == 0
    assert np.array_equal(prj.project_colsum(Z, rows=np.zeros(0, dtype=np.int64)), np.zeros(S))
    assert prj.project_select(Z, resid, rows=np.zeros(0, dtype=np.int64)) == (-np.inf, -1)


@pytest.mark.parametrize("S", (100, 256))
@pytest.mark.parametrize("aligned", (True, False))
@pytest.mark.parametrize("family", FAMILIES)
def test_every_combination_is_fused(family, aligned, S):
    """The C entries themselves, for every (consumer, family, alignment, tile width): BCX_OK -- every gathered instantiation is
    built (none takes the fallback) -- and the values of the contiguous entries on the copy."""
    torch = _torch()
    lib = _native.load()
    D = 12
    Zh, Dp = _data(family, D)
    cols = Zh.shape[1]
    ld = cols + (cols % 2) if aligned else cols + 1 - (cols % 2)
    buf = torch.zeros((N_STANDING, ld), dtype=torch.float64, device="cuda")
    buf[:, :cols] = torch.from_numpy(Zh).cuda()
    Z = buf[:, :cols]
    rs = np.random.RandomState(2)
    theta, resid = 0.3 * rs.randn(S, Dp), rs.randn(S)
    prj = _projector(family, theta, colsum="mfma")
    idx = torch.from_numpy(rs.randint(N_STANDING, size=5000)).cuda()
    cbuf = torch.zeros((5000, ld), dtype=torch.float64, device="cuda")
    assert lib.bcx_gather_rows(prj._stream(), Z.data_ptr(), ld, cols, idx.data_ptr(), 5000, cbuf.data_ptr(), ld) == 0
    copy = cbuf[:, :cols]
    assert torch.equal(copy, Z[idx])
    col = torch.empty(S, dtype=torch.float64, device="cuda")
    rc = lib.bcx_project_colsum_rows(*(prj._common(Z) + [idx.data_ptr(), 5000, col.data_ptr(), prj._workspace(S).data_ptr()]))
    assert rc == _native.OK, lib.bcx_project_last_error().decode()
    assert np.array_equal(col.cpu().numpy(), prj.project_colsum(copy))
    need = int(lib.bcx_project_select_rows_scratch_bytes(prj._fam, 5000, S))
    work = torch.empty(need // 8 + 1, dtype=torch.float64, device="cuda")
    res = torch.empty(2, dtype=torch.float64, device="cuda")
    r = torch.from_numpy(resid).cuda()
    rc = lib.bcx_project_select_rows_ws(*(prj._common(Z) + [idx.data_ptr(), 5000, r.data_ptr(), float(resid.sum()), res.data_ptr(),
                                                            work.data_ptr(), work.numel() * 8]))
    assert rc == _native.OK, lib.bcx_project_last_error().decode()
    h = res.cpu()
    assert (float(h[0]), int(h[1:2].view(torch.int64)[0])) == prj.project_select(copy, resid)
    # scratch one byte short, and a matrix beyond the 32-bit reach of the requests (argument check only: nothing is launched)
    assert lib.bcx_project_select_rows_ws(*(prj._common(Z) + [idx.data_ptr(), 5000, r.data_ptr(), 0.0, res.data_ptr(), work.data_ptr(),
                                                              need - 1])) == _native.ERR_ARG
    far = prj._common(Z)
    far[3] = (1 << 33) // ld * (2 if aligned else 1) + 2
    assert lib.bcx_project_colsum_rows(*(far + [idx.data_ptr(), 5000, col.data_ptr(), prj._workspace(S).data_ptr()])) == _native.ERR_ARG


# ---- 2. against the likelihoods ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ("logistic", "poisson", "linreg"))
def test_gathered_consumers_against_numpy(family):
    """The NumPy restatements of tests/models.py on Z[idx], with the tolerances tests/test_gpu_projection.py:43-48 holds the
    contiguous consumers to: column sums rtol 1e-9 + atol 1e-9 of the mean absolute column sum, the arg-max row exact, its value rtol 1e-7."""
    _torch()
    D = 10
    Zh, Dp = _data(family, D, seed=5)
    rs = np.random.RandomState(5)
    theta = (0.3 if family == "poisson" else 1.0) * rs.randn(64, Dp)
    ll = {"logistic": logistic_log_likelihood, "poisson": poisson_log_likelihood,
          "linreg": lambda z, th: linreg_log_likelihood(z, th, 0.7)}[family]
    prj = _projector(family, theta)
    idx = rs.randint(N_STANDING, size=6007)
    want = ll(Zh[idx], theta)
    want = want - want.mean(axis=1)[:, None]
    np.testing.assert_allclose(prj.project_colsum(Zh, rows=idx), want.sum(axis=0), rtol=1e-9, atol=1e-9 * np.abs(want).sum() / want.shape[1])
    resid = np.random.RandomState(9).randn(theta.shape[0])
    corrs = want.dot(resid) / np.sqrt((want ** 2).sum(axis=1)) / want.shape[1]
    best, pos = prj.project_select(Zh, resid, rows=idx)
    assert pos == int(np.argmax(corrs))
    np.testing.assert_allclose(best, corrs.max(), rtol=1e-7)


# ---- 3. host loops: "device" = "host" ----------------------------------------------------------------------------------------------------
def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.mark.parametrize("nsub", (600, 5000))
@pytest.mark.parametrize("colsum", ("auto", "mfma"))
@pytest.mark.parametrize("family", ("logistic", "linreg"))
def test_sparsevi_host_loop_device_equals_host(family, colsum, nsub):
    _torch()
    D, S = 6, 32
    if family == "linreg":
        Z = make_linreg_data(2, 20000, D)
        smp = linreg_sampler(np.zeros(D), np.eye(D), 1.0)
    else:
        Z = make_lr_data(2, 20000, D)
        smp = lambda n, w, p: np.random.randn(n, D)
    out = {}
    for mode in ("host", "device"):
        np.random.seed(8)
        prj = bc.DeviceProjector(family, smp, S, sigsq=1.0, colsum=colsum)
        alg = bc.SparseVICoreset(Z, prj, n_subsample_select=nsub, n_subsample_opt=nsub, opt_itrs=6, subsample=mode)
        alg.build(4)
        assert alg._enqueue_plan() is None
        out[mode] = (alg.idcs.copy(), alg.wts.copy(), alg.pts.copy(), np.random.get_state())
    assert out["host"][0].size >= 2
    for a, b in zip(out["host"][:3], out["device"][:3]):
        assert np.array_equal(a, b)
    assert _same_state(out["host"][3], out["device"][3])


@pytest.mark.parametrize("nsub", (600, 5000))
@pytest.mark.parametrize("colsum", ("auto", "mfma"))
@pytest.mark.parametrize("family", ("linreg", "gaussian"))
def test_bpsvi_host_loop_device_equals_host(family, colsum, nsub):
    _torch()
    N, D, S, k, T = 20000, 6, 32, 8, 6
    Z, make, kw, _, _ = _model(family, N, D, 2, sampler_seed=9)
    out = {}
    for mode in ("host", "device"):
        s = make()
        alg = bc.BatchPSVICoreset(Z, bc.DeviceProjector(family, lambda n, w, p: s(n, w, p), S, colsum=colsum, **kw), T,
                                  n_subsample_opt=nsub, step_sched=lambda i: 0.2 / (1.0 + i), subsample=mode)
        np.random.seed(4)
        alg.build(k)
        assert alg._enqueue_plan() is None and alg._enqueue_plan_subsampled() is None      # callback sampler: host loop
        out[mode] = (alg.wts.copy(), alg.pts.copy(), np.random.get_state())
    assert np.array_equal(out["host"][0], out["device"][0]) and np.array_equal(out["host"][1], out["device"][1])
    assert _same_state(out["host"][2], out["device"][2])


# ---- 4. the reference's fixture ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("colsum", ("mfma", "moments"))
def test_bpsvi_reference_fixture_with_device_subsampling(colsum):
    """tests/test_gpu_bpsvi.py:262-273 with ``subsample="device"``: the reference's trajectory at n_subsample_opt = 500 through the
    replayed NumPy sampler, under that test's tolerances."""
    _torch()
    g = golden()
    Z, smp, _, _ = linreg_run_inputs()
    np.random.seed(LR["np_seed"])
    prj = bc.DeviceProjector("linreg", smp, LR["S"], sigsq=LR["sigsq"], colsum=colsum)
    alg = bc.BatchPSVICoreset(Z, prj, LR["itrs"], n_subsample_opt=500, step_sched=LR["sched"], subsample="device")
    alg.build(LR["k"])
    np.testing.assert_allclose(alg.wts, g["lr_sub_wts"], rtol=1e-7)
    np.testing.assert_allclose(alg.pts, g["lr_sub_pts"], rtol=1e-6, atol=1e-8)


# ---- 5. the enqueued sub-sampled loops against the host loops ---------------------------------------------------------------------------------
class _RandintRecorder(object):
    def __init__(self, monkeypatch):
        self.real, self.calls = np.random.randint, []
        monkeypatch.setattr(np.random, "randint", self)

    def __call__(self, *a, **kw):
        r = self.real(*a, **kw)
        self.calls.append(np.array(r))
        return r


@pytest.mark.parametrize("family", ("linreg", "gaussian", "logistic"))
def test_bpsvi_enqueued_subsampled_loop_matches_the_host_loop(family, monkeypatch):
    """As test_enqueued_loop_matches_the_host_loop (tests/test_gpu_bpsvi_loop.py:319) with n_subsample_opt: k = 20 >= D + 1 and, for
    linreg, > 4 + 2 ceil(D / 32), so both loops draw alike -- inside the referee's stated domain."""
    torch = _torch()
    N, D, S, k, T, nsub = 20000, 12, 64, 20, 15, 3000
    Z, make, kw, _, _ = _model(family, N, D, 11)
    noise = _noise(torch, 2 * T + 4, S, D, 17)
    rec = _RandintRecorder(monkeypatch)
    out = {}
    for mode in (True, False):
        smp = _ReplaySampler(make(), noise)
        prj = bc.DeviceProjector(family, smp, S, **kw)
        alg = bc.BatchPSVICoreset(Z, prj, T, n_subsample_opt=nsub, step_sched=lambda i: 0.2 / (1.0 + i), subsample="device")
        alg.ENQUEUE = mode
        np.random.seed(3)
        rec.calls = []
        alg.build(k)
        state, tables, used = np.random.get_state(), list(rec.calls), smp.at
        assert alg._enqueue_plan() is None                                    # (n_subsample_opt: never the full-data plan)
        assert (alg._enqueue_plan_subsampled() is not None) == mode           # the loop under test was the enqueued one / the host one
        out[mode] = (alg.wts.copy(), alg.pts.copy(), used, state, tables)
    assert out[True][2] == out[False][2] == 1 + T
    assert _same_state(out[True][3], out[False][3])                          # the same calls in the same order
    assert len(out[True][4]) == len(out[False][4]) == T and all(np.array_equal(a, b) for a, b in zip(out[True][4], out[False][4]))
    _report("%s sub-sampled enqueued vs host" % family, out[True][0], out[True][1], out[False][0], out[False][1])
    np.testing.assert_allclose(out[True][0], out[False][0], rtol=W_RTOL)
    np.testing.assert_allclose(out[True][1], out[False][1], rtol=P_RTOL, atol=P_ATOL)


@pytest.mark.parametrize("sampler", ("linreg", "laplace"))
@pytest.mark.parametrize("k", (8, 65))
def test_sparsevi_enqueued_subsampled_loop_matches_the_host_loop(k, sampler, monkeypatch):
    """The weight optimisation of a seeded coreset of k points with n_subsample_opt, enqueued against the host loop on the same
    normal numbers and the same index draws: rtol 1e-7, atol 1e-9 of the largest weight (tests/test_gpu_svi.py:403)."""
    torch = _torch()
    N, D, S, T, nsub = 20000, 12, 32, 10, 3000
    rs = np.random.RandomState(100 + k)
    if sampler == "linreg":
        Z, family = make_linreg_data(13, N, D), "linreg"
        make = lambda: bc.LinregPosteriorSampler(np.zeros(D), np.eye(D), 0.8)
    else:
        Z, family = make_lr_data(13, N, D), "logistic"
        make = lambda: bc.LaplacePosteriorSampler("logistic", D)
    idcs = np.sort(rs.choice(N, size=k, replace=False)).astype(np.int64)
    w0 = np.abs(rs.randn(k)) * (N / k)
    noise = _noise(torch, 2 * T + 4, S, D, 29)
    rec = _RandintRecorder(monkeypatch)
    out = {}
    for mode in (True, False):
        smp = _ReplaySampler(make(), noise)
        alg = bc.SparseVICoreset(Z, bc.DeviceProjector(family, smp, S, sigsq=0.8), n_subsample_opt=nsub, opt_itrs=T, subsample="device")
        alg.ENQUEUE = mode
        alg.wts, alg.idcs, alg.pts = w0.copy(), idcs.copy(), Z[idcs].copy()
        assert alg._enqueue_plan() is None
        plan = alg._enqueue_plan_subsampled()
        assert (plan is not None) == mode
        smp.at = 1                                                            # (the constructor's draw; the probe took a plan's worth)
        np.random.seed(6)
        rec.calls = []
        alg._optimize()
        out[mode] = (alg.wts.copy(), np.random.get_state(), list(rec.calls), smp.at)
    assert out[True][3] == out[False][3] == 1 + T
    assert _same_state(out[True][1], out[False][1])
    assert len(out[True][2]) == T and all(np.array_equal(a, b) for a, b in zip(out[True][2], out[False][2]))
    np.testing.assert_allclose(out[True][0], out[False][0], rtol=1e-7, atol=1e-9 * np.abs(out[False][0]).max())


# ---- 6. fallbacks and failures ---------------------------------------------------------------------------------------------------------------
def test_index_budget_and_validation(monkeypatch):
    torch = _torch()
    N, D, S, k, T, nsub = 20000, 6, 32, 8, 6, 600
    Z, make, kw, _, _ = _model("linreg", N, D, 2, sampler_seed=9)

    def build(budget=None, enqueue=True):
        alg = bc.BatchPSVICoreset(Z, bc.DeviceProjector("linreg", make(), S, **kw), T, n_subsample_opt=nsub,
                                  step_sched=lambda i: 0.2 / (1.0 + i), subsample="device")
        alg.ENQUEUE = enqueue
        if budget is not None:
            alg.INDEX_BUDGET = budget
        np.random.seed(4)
        alg.build(k)
        return alg
    over, host = build(budget=8 * T * nsub - 1), build(enqueue=False)
    assert over._enqueue_plan_subsampled() is None
    assert np.array_equal(over.wts, host.wts) and np.array_equal(over.pts, host.pts)     # over the budget: the host loop itself
    assert build()._enqueue_plan_subsampled() is not None
    # an index outside [0, N): refused on the host, before any launch
    prj = bc.DeviceProjector("linreg", lambda n, w, p: np.zeros((n, D)), S)
    for bad in (np.array([0, N]), np.array([-1, 3]), torch.tensor([5, N], device="cuda")):
        with pytest.raises(ValueError):
            prj.project_colsum(Z, rows=bad)
        with pytest.raises(ValueError):
            prj.project_select(Z, np.ones(S), rows=bad)
    with pytest.raises(ValueError):
        prj.project_colsum(Z, rows=np.array([0.5, 1.0]))
    # constructor refusals
    bbp = bc.BlackBoxProjector(lambda n, w, p: np.zeros((n, D)), S, lambda z, th: linreg_log_likelihood(z, th, 1.0))
    with pytest.raises(ValueError):
        bc.SparseVICoreset(Z, bbp, subsample="device")
    with pytest.raises(ValueError):
        bc.SparseVICoreset(Z, prj, subsample="device", group=object())


def test_a_failed_step_in_the_middle_still_raises_after_the_subsampled_loop():
    """The status of the sampler's plan is sticky (tests/test_gpu_bpsvi_loop.py:539): a plan whose ``check()`` raises because a
    middle step failed raises after the sub-sampled loop too -- the loop calls it once, after its read-back."""
    _torch()
    N, D, S, k, T, nsub = 6000, 6, 32, 8, 5, 500
    Z, make, kw, _, _ = _model("linreg", N, D, 2, sampler_seed=9)
    smp = make()
    alg = bc.BatchPSVICoreset(Z, bc.DeviceProjector("linreg", smp, S, **kw), T, n_subsample_opt=nsub, subsample="device")
    np.random.seed(4)
    alg.build(k)
    plan = alg._enqueue_plan_subsampled()
    seen = []

    class Failing(object):
        def __getattr__(self, name):
            return getattr(plan, name)

        def draw(self, w, i):
            seen.append(i)
            return plan.draw(w, i)

        def check(self):
            raise _native.EngineError(_native.ERR_STATE, "step 2 failed")
    with pytest.raises(_native.EngineError):
        alg._optimize_enqueued(Failing(), n_sub=nsub)
    assert seen == list(range(T))                                             # the loop ran to its end before the status was read
