"""GPU: many weighted posteriors in one NUTS launch -- bc.DeviceHMC(kernel="nuts").sample_many (csrc/nuts.hip nuts_batch_kernel,
bcx_nuts_batch).  The contract is bit-identity: every field of every result, trace included, equals what the
corresponding `sample` call returns, `seconds_per_iteration` excepted.  (1) plain NUTS on problems listed by ascending k, so the
dispatch order (k descending) is a real permutation -- the prior, one point, no weights, more points than one stride of the
256-thread loop, explicit and missing frames -- with the sampler's own stream and with per-problem seeds; (2) Poisson's extra
column and the widest frame; (3) the learned metric, diag and dense, with one window and with none; (4) more workgroups than the
device has CUs; (5) a start that is not finite is attributed to its problem; (6) every ValueError; (7) reproducibility."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
FIELDS = ("samples", "accept_rate", "step_size", "rhat", "delta_h", "accepted", "accept_stat", "tree_depth", "n_leapfrog", "divergent",
          "leapfrog_total", "center", "transform")
SCALARS = ("streamed", "nonfinite_rejected", "n_warmup", "kernel", "max_depth", "adapt_metric")
TRACE = ("noise", "theta", "xi", "proposal", "diag")


@pytest.fixture(scope="module")
def bc():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import bayesiancoresets_amd as bc
    return bc


def _logistic(k, D, rs):
    X = np.hstack((rs.randn(k, D - 1), np.ones((k, 1))))
    y = np.where(rs.rand(k) < 1.0 / (1.0 + np.exp(-X.dot(np.ones(D) / np.sqrt(D)))), 1.0, -1.0)
    return y[:, None] * X


def _poisson(k, D, rs):
    X = np.hstack((0.5 * rs.randn(k, D - 1), np.ones((k, 1))))
    return np.hstack((X, rs.poisson(np.log1p(np.exp(X.dot(np.ones(D) / D))))[:, None].astype(np.float64)))


def _same(a, b, trace, adapt=False):
    """Every field of result b equals result a's (the single call's), but the wall time."""
    for q in FIELDS + (("metric", "metric_windows") if adapt else ()):
        assert np.array_equal(getattr(a, q), getattr(b, q), equal_nan=(q == "rhat")), q
    for q in SCALARS:
        assert getattr(a, q) == getattr(b, q), q
    assert set(a.__dict__) | {"batch_seconds"} == set(b.__dict__)
    if not trace:
        assert a.trace is None and b.trace is None
        return
    assert set(a.trace) == set(b.trace) and a.trace["step0"] == b.trace["step0"]
    for q in TRACE + (("frames",) if adapt else ()):
        assert np.array_equal(a.trace[q], b.trace[q]), q


def _single(hmc, q, ns, nw, trace):
    return hmc.sample(q.get("pts"), q.get("wts"), ns, nw, center=q.get("center"), transform=q.get("transform"), keep_trace=trace)


@pytest.fixture(scope="module")
def five():
    """Logistic, D = 5 (ld = 6), ascending k: the prior; one point; 7 with a centre and no transform; 40 without weights; 300 (two
    strides of the point loop) with a centre and a full, non-triangular transform."""
    rs, D = np.random.RandomState(11), 5
    full = 0.3 * np.eye(D) + 0.05 * rs.randn(D, D)
    return D, [dict(pts=None, wts=None),
               dict(pts=_logistic(1, D, rs), wts=np.array([2.5])),
               dict(pts=_logistic(7, D, rs), wts=rs.uniform(1.0, 4.0, 7), center=0.2 * rs.randn(D), transform=None),
               dict(pts=_logistic(40, D, rs), wts=None),
               dict(pts=_logistic(300, D, rs), wts=rs.uniform(0.5, 3.0, 300), center=0.1 * rs.randn(D), transform=full)]


# ---------------------------------------------------------------------------------------------------------------- 1
def test_plain_nuts_equals_successive_sample_calls(bc, five):
    D, problems = five
    kw = dict(chains=4, seed=7, kernel="nuts", max_depth=5)
    one, many = bc.DeviceHMC("logistic", D, **kw), bc.DeviceHMC("logistic", D, **kw)
    want = [_single(one, q, 20, 30, True) for q in problems]
    got = many.sample_many(problems, 20, 30, keep_trace=True)
    assert len(got) == 5 and many._offset == one._offset
    for a, b in zip(want, got):
        _same(a, b, True)
    assert len({b.seconds_per_iteration for b in got}) == 1 and got[0].batch_seconds == got[0].seconds_per_iteration * 50
    assert not np.array_equal(got[2].samples, got[3].samples)
    # the next call goes on in the stream where five sample calls would have left it; tuples in place of dicts
    pairs = [(q["pts"], q["wts"]) for q in (problems[3], problems[1], problems[0])]
    for a, b in zip([one.sample(p, w, 5, 5) for p, w in pairs], many.sample_many(pairs, 5, 5)):
        _same(a, b, False)


def test_seeds_read_fresh_samplers_and_leave_the_stream(bc, five):
    D, problems = five
    seeds = [3, 3, 9, 9, 1]
    kw = dict(chains=4, kernel="nuts", max_depth=5)
    many = bc.DeviceHMC("logistic", D, seed=7, **kw)
    got = many.sample_many(problems, 20, 30, seeds=seeds, keep_trace=True)
    assert many._offset == 0
    for q, s, b in zip(problems, seeds, got):
        _same(_single(bc.DeviceHMC("logistic", D, seed=s, **kw), q, 20, 30, True), b, True)
    assert np.array_equal(got[0].trace["noise"], got[1].trace["noise"]) and not np.array_equal(got[1].trace["noise"], got[2].trace["noise"])


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("D,sizes", ((4, (3, 60)), (32, (2,))))
def test_poisson(bc, D, sizes):
    rs = np.random.RandomState(5)
    problems = [dict(pts=_poisson(k, D, rs), wts=rs.uniform(0.5, 2.0, k)) for k in sizes]
    kw = dict(chains=4, seed=2, kernel="nuts", max_depth=5)
    one, many = bc.DeviceHMC("poisson", D, **kw), bc.DeviceHMC("poisson", D, **kw)
    want = [_single(one, q, 20, 30, True) for q in problems]
    for a, b in zip(want, many.sample_many(problems, 20, 30, keep_trace=True)):
        _same(a, b, True)


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("metric", ("diag", "dense"))
@pytest.mark.parametrize("n_warmup,windows", ((150, [[75, 100]]), (19, [])))
def test_learned_metric(bc, metric, n_warmup, windows):
    rs, D = np.random.RandomState(8), 5
    problems = [dict(pts=_logistic(k, D, rs), wts=rs.uniform(0.5, 3.0, k)) for k in (12, 40)]
    problems[1].update(center=np.zeros(D), transform=np.eye(D))                # (a frame the metric has something to learn in)
    kw = dict(chains=4, seed=4, kernel="nuts", max_depth=5, adapt_metric=metric)
    one, many = bc.DeviceHMC("logistic", D, **kw), bc.DeviceHMC("logistic", D, **kw)
    want = [_single(one, q, 20, n_warmup, True) for q in problems]
    got = many.sample_many(problems, 20, n_warmup, keep_trace=True)
    for a, b in zip(want, got):
        assert b.metric_windows.tolist() == windows and b.trace["frames"].shape == (4, len(windows), D, D)
        _same(a, b, True, adapt=True)
    if windows:
        assert not np.array_equal(got[1].metric, np.broadcast_to(np.eye(D), (4, D, D)))


# ---------------------------------------------------------------------------------------------------------------- 4
def test_more_workgroups_than_cus(bc):
    rs, D = np.random.RandomState(21), 3
    problems = [dict(pts=_logistic(k, D, rs), wts=rs.uniform(0.5, 3.0, k)) for k in (2, 5, 9, 14, 20)]
    kw = dict(chains=64, seed=6, kernel="nuts", max_depth=4)
    one, many = bc.DeviceHMC("logistic", D, **kw), bc.DeviceHMC("logistic", D, **kw)
    want = [_single(one, q, 10, 10, False) for q in problems]
    for a, b in zip(want, many.sample_many(problems, 10, 10)):
        _same(a, b, False)


# ---------------------------------------------------------------------------------------------------------------- 5
def test_a_start_that_is_not_finite_is_its_problems(bc):
    import re
    from bayesiancoresets_amd import _native
    rs, D = np.random.RandomState(9), 3
    problems = [dict(pts=_logistic(6, D, rs), wts=rs.uniform(0.5, 3.0, 6), center=np.zeros(D), transform=np.eye(D)) for _ in range(3)]
    problems[1]["wts"] = problems[1]["wts"].copy()
    problems[1]["wts"][2] = np.nan
    hmc = bc.DeviceHMC("logistic", D, chains=4, seed=1, kernel="nuts", max_depth=4)
    with pytest.raises(_native.EngineError) as err:
        hmc.sample_many(problems, 5, 5)
    assert err.value.code == _native.ERR_STATE
    named = [int(s) for s in re.findall(r"\d+", str(err.value).split("problem", 1)[1])]
    assert named == [1]


# ---------------------------------------------------------------------------------------------------------------- 6
def test_value_errors(bc, five, monkeypatch):
    D, problems = five
    with pytest.raises(ValueError, match="nuts"):
        bc.DeviceHMC("logistic", D, chains=4).sample_many(problems, 5, 5)
    with pytest.raises(ValueError, match="stream"):
        bc.DeviceHMC("logistic", D, chains=4, kernel="nuts", stream=True).sample_many(problems, 5, 5)
    hmc = bc.DeviceHMC("logistic", D, chains=4, seed=3, kernel="nuts", max_depth=5)
    with pytest.raises(ValueError, match="no problems"):
        hmc.sample_many([], 5, 5)
    with pytest.raises(ValueError, match="4 seeds for 5"):
        hmc.sample_many(problems, 5, 5, seeds=[1, 2, 3, 4])
    k = 1
    while hmc.nuts_path(2 * k):
        k *= 2
    big = np.zeros((2 * k, D))
    with pytest.raises(ValueError, match="problem 2:"):
        hmc.sample_many(problems[:2] + [dict(pts=big, wts=None, center=np.zeros(D), transform=np.eye(D))], 5, 5)
    dense = bc.DeviceHMC("logistic", D, chains=4, seed=3, kernel="nuts", max_depth=5, adapt_metric="dense")
    ka = 2 * k
    while not dense.adapt_path(ka):
        ka -= 64
    assert hmc.nuts_path(ka + 64)                                               # (the plain kernel holds what the adapting one does not)
    with pytest.raises(ValueError, match="problem 1:.*adapt_metric"):
        dense.sample_many([problems[1], dict(pts=np.zeros((ka + 64, D)), wts=None, center=np.zeros(D), transform=np.eye(D))], 5, 5)
    # the noise is summed over the problems: each of the five is within the limit, the five together are not
    R = D + 3 * 5 + 2 * (2 ** 5 - 1)
    import bayesiancoresets_amd.mcmc as lib_mcmc
    monkeypatch.setattr(lib_mcmc, "NUTS_NOISE_BYTES_MAX", 8 * 4 * 10 * R * 5 - 1)
    with pytest.raises(ValueError, match="noise"):
        hmc.sample_many(problems, 5, 5)
    assert len(hmc.sample_many(problems[:4], 5, 5)) == 4
    monkeypatch.undo()
    before = hmc._offset
    hmc.sample_many(problems, 5, 5, seeds=[1, 2, 3, 4, 5])
    assert hmc._offset == before and before > 0


# ---------------------------------------------------------------------------------------------------------------- 7
def test_reproducible(bc, five):
    D, problems = five
    kw = dict(chains=4, seed=12, kernel="nuts", max_depth=5)
    a = bc.DeviceHMC("logistic", D, **kw).sample_many(problems, 10, 10, keep_trace=True)
    b = bc.DeviceHMC("logistic", D, **kw).sample_many(problems, 10, 10, keep_trace=True)
    for x, y in zip(a, b):
        _same(x, y, True)
        assert np.all(np.isfinite(x.samples))
