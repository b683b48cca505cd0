"""GPU: bc.log_predictive (csrc/predict.hip) -- the held-out log predictive density lppd[n] = logsumexp_s ll(z_n,
theta_s) - log S and mean_ll[n] -- against the reference's table (tests/golden/predictive_golden.npz), against the long-double
restatement (tests/predictive_restatement.py) at the shapes where the kernel changes path, over input layouts, with non-finite
input, against bc.log_joint_grad, and at its limits.

Measured on an MI355X, the largest deviation from the long-double referee over the edge cases of test 2 in units of u = 2^-53 of
max(1, |value|), the float64 restatement's own beside it: lppd 9.9 u (float64: 6.1 u), mean_ll 50.8 u (float64: 5.3 u) -- the
latter on rows whose ll is nearly the same for all S = 1000 draws, where a lane's serial sum of 250 like terms drifts one way
and NumPy's pairwise sum does not; the floor there is 1064 u.  Against the fixture (test 1): lppd 9 u, mean_ll 4.4 u."""
import itertools
import os

import numpy as np
import pytest

import predictive_restatement as restate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
FAMILIES = ("logistic", "poisson")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bc():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import bayesiancoresets_amd as bc
    return bc


def _dev(got, want):
    """Largest deviation in units of max(1, |want|); a NaN or an inf that the referee does not have is inf."""
    want = np.asarray(want, dtype=np.longdouble)
    got = np.asarray(got, dtype=np.longdouble)
    same = (got == want)                                                        # (equal infinities)
    d = np.where(same, 0, np.abs(got - want) / np.maximum(1, np.abs(want)))
    d = np.where(np.isnan(d), np.inf, d)
    return float(d.max()) if d.size else 0.0


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "predictive_golden.npz"))


@pytest.mark.parametrize("tag,family", (("lr", "logistic"), ("poiss", "poisson")))
@pytest.mark.parametrize("splits", (0, 1, 2, 3, 7))
def test_golden(bc, gold, tag, family, splits):
    """The device against the reference's table reduced by scipy.  Bound: the fixture's table is within 16 u of the referee per
    entry (asserted at generation) and its reduction of S same-sign terms within S u; the device's floor is (S + 64) u (test 2):
    2 (S + 64) u in all.  S = 96 over 7 ranges: 13 or 14 draws each, uneven and below one MFMA tile."""
    Z, th = gold[tag + "_Z"], gold[tag + "_th"]
    S = th.shape[0]
    res = bc.log_predictive(family, Z, th, _dev_splits=splits)
    assert res.n_draws == S and res.lppd.shape == res.mean_ll.shape == (Z.shape[0],)
    d_lppd, d_mean = _dev(res.lppd, gold[tag + "_lppd"]), _dev(res.mean_ll, gold[tag + "_mean_ll"])
    print("golden %s splits %d: lppd %.3g u, mean_ll %.3g u" % (tag, splits, d_lppd / U, d_mean / U))
    assert d_lppd <= 2 * (S + 64) * U and d_mean <= 2 * (S + 64) * U
    assert res.elpd == pytest.approx(gold[tag + "_lppd"].sum(), rel=1e-12)


# ---------------------------------------------------------------------------------------------------------------- 2
NS = (1, 15, 16, 17, 127, 128, 129, 300)
SS = (1, 3, 4, 5, 63, 64, 65, 1000)
DS = (1, 3, 4, 31, 32)
# 40 of the 320 shapes: every N five times, every S five times (the offset i // 8 moves S against N), every D eight times
EDGE_SHAPES = tuple((NS[i % 8], SS[(i + i // 8) % 8], DS[i % 5]) for i in range(40))
assert {c[0] for c in EDGE_SHAPES} == set(NS) and {c[1] for c in EDGE_SHAPES} == set(SS) and {c[2] for c in EDGE_SHAPES} == set(DS)
assert len(set(EDGE_SHAPES)) == 40

LOGISTIC_PREDICTORS = tuple(sg * v for v in (0.1, 30.0, 99.9, 100.1, 800.0) for sg in (1.0, -1.0))
POISSON_PREDICTORS = tuple(itertools.product((-150.0, -99.9, -30.0, 0.0, 30.0), (0.0, 1.0, 7.0, 255.0, 256.0, 300.0)))

SEEN = {"device": {"lppd": 0.0, "mean_ll": 0.0}, "float64": {"lppd": 0.0, "mean_ll": 0.0}}


def edge_inputs(family, N, S, D, seed):
    """Seeded rows and draws.  The draws scatter about a unit vector t0: the first half tightly (2e-4), the second half widely
    (0.3 / sqrt D).  The first rows are multiples c t0, so that their predictor is c to 2e-4 relative under the tight draws and
    every branch of the likelihood is taken (logistic: the linear tail from -s = 100; Poisson: s <= -100, counts on both sides
    of 255); the list is rotated by the seed so that small N see all of it over the cases.  The other rows are standard normal."""
    rs = np.random.RandomState(seed)
    t0 = rs.randn(D)
    t0 /= np.linalg.norm(t0)
    sig = np.where(np.arange(S) < (S + 1) // 2, 2e-4, 0.3 / np.sqrt(D))
    th = t0 + sig[:, None] * rs.randn(S, D)
    X = rs.randn(N, D)
    if family == "logistic":
        special = np.roll(np.array(LOGISTIC_PREDICTORS), seed)
        k = min(N, len(special))
        X[:k] = special[:k, None] * t0
        return X, th
    y = rs.poisson(np.log1p(np.exp(np.clip(X.dot(t0), -30, 5)))).astype(np.float64)
    special = np.roll(np.array(POISSON_PREDICTORS), 7 * seed, axis=0)
    k = min(N, len(special))
    X[:k] = special[:k, :1] * t0
    y[:k] = special[:k, 1]
    return np.hstack((X, y[:, None])), th


def _held_to_the_referee(bc, family, Z, th, splits_list, label):
    """Per quantity: the float64 restatement's deviation from the long-double referee, the bar 16 x that with the floor
    (S + 64) u -- S same-sign terms summed in any order lose at most (S - 1) u, 64 u for the evaluation of a term -- and the
    device at every `splits` under the bar."""
    S = th.shape[0]
    ref = dict(zip(("lppd", "mean_ll"), restate.log_predictive(family, Z, th, np.longdouble)))
    f64 = dict(zip(("lppd", "mean_ll"), restate.log_predictive(family, Z, th, np.float64)))
    for splits in splits_list:
        res = bc.log_predictive(family, Z, th, _dev_splits=splits)
        got = {"lppd": res.lppd, "mean_ll": res.mean_ll}
        for q in ("lppd", "mean_ll"):
            d64, ddev = _dev(f64[q], ref[q]), _dev(got[q], ref[q])
            bar = max(16.0 * d64, (S + 64) * U)
            SEEN["device"][q], SEEN["float64"][q] = max(SEEN["device"][q], ddev), max(SEEN["float64"][q], d64)
            print("%s splits %d %s: device %.3g u, float64 %.3g u, bar %.3g u | so far device %.3g u float64 %.3g u"
                  % (label, splits, q, ddev / U, d64 / U, bar / U, SEEN["device"][q] / U, SEEN["float64"][q] / U))
            assert ddev <= bar, (label, splits, q, ddev / U, bar / U)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", range(40))
def test_edges_against_the_long_double_referee(bc, family, case):
    N, S, D = EDGE_SHAPES[case]
    Z, th = edge_inputs(family, N, S, D, case)
    _held_to_the_referee(bc, family, Z, th, (1, 3), "%s N %d S %d D %d" % (family, N, S, D))


@pytest.mark.parametrize("family", FAMILIES)
def test_a_row_with_half_its_draws_800_below(bc, family):
    """Row 0 is the first unit vector (Poisson: y = 1); the first coordinate of the draws is about -1 for the even draws and about
    -801 for the odd ones: ll ~ s on that side of either model, so the odd draws sit 800 below and add exact zeros; lppd is
    logsumexp of the even ones - log S."""
    rs = np.random.RandomState(11)
    N, S, D = 17, 64, 3
    th = 0.1 * rs.randn(S, D)
    th[:, 0] += np.where(np.arange(S) % 2 == 0, -1.0, -801.0)
    X = 0.01 * rs.randn(N, D)
    X[0] = (1.0, 0.0, 0.0)
    Z = X if family == "logistic" else np.hstack((X, np.ones((N, 1))))
    ll = restate.log_likelihood(family, Z, th)
    assert np.all(ll[0, 1::2] < ll[0, 0::2].max() - 790)
    _held_to_the_referee(bc, family, Z, th, (1, 3), "%s half at -800" % family)
    res = bc.log_predictive(family, Z, th, _dev_splits=2)
    even = bc.log_predictive(family, Z[:1], th[0::2], _dev_splits=1)
    assert abs(res.lppd[0] - (even.lppd[0] - np.log(2.0))) <= 64 * U * abs(res.lppd[0])


@pytest.mark.parametrize("splits", (1, 3))
def test_every_ll_at_minus_800_is_minus_800(bc, splits):
    # logistic, -s >= 100: ll = s exactly; x = 1 and every draw -800 (row 1: -0.5, ll = -400)
    res = bc.log_predictive("logistic", np.array([[1.0], [0.5]]), np.full((50, 1), -800.0), _dev_splits=splits)
    assert np.array_equal(res.lppd, [-800.0, -400.0]) and np.array_equal(res.mean_ll, [-800.0, -400.0])


@pytest.mark.parametrize("family", FAMILIES)
def test_one_draw_and_equal_draws(bc, family):
    rs = np.random.RandomState(5)
    D = 4
    X = rs.randn(30, D)
    Z = X if family == "logistic" else np.hstack((X, rs.poisson(2.0, 30)[:, None].astype(np.float64)))
    th = 0.5 * rs.randn(1, D)
    one = bc.log_predictive(family, Z, th, _dev_splits=3)                       # (two of the three ranges are empty)
    assert np.array_equal(one.lppd, one.mean_ll)
    assert _dev(one.lppd, restate.log_likelihood(family, Z, th)[:, 0]) <= 65 * U
    many = bc.log_predictive(family, Z, np.repeat(th, 8, axis=0), _dev_splits=2)
    assert np.array_equal(many.lppd, one.lppd)                                  # (8 equal terms: the sum of ones is exact)
    assert _dev(many.mean_ll, one.mean_ll) <= 8 * U                             # (3 ll, 5 ll ... round)


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("splits", (0, 3))
def test_layouts_agree_bit_for_bit(bc, family, splits):
    import torch
    rs = np.random.RandomState(21)
    N, D, chains, draws = 150, 5, 4, 33
    cols = D + (1 if family == "poisson" else 0)
    X = rs.randn(N, D)
    Z = X if family == "logistic" else np.hstack((X, rs.poisson(3.0, N)[:, None].astype(np.float64)))
    th3 = 0.4 * rs.randn(chains, draws, D)
    base = bc.log_predictive(family, Z, th3.reshape(-1, D), _dev_splits=splits)
    assert isinstance(base.lppd, np.ndarray) and base.n_draws == chains * draws
    again = bc.log_predictive(family, Z, th3.reshape(-1, D), _dev_splits=splits)
    assert np.array_equal(base.lppd, again.lppd) and np.array_equal(base.mean_ll, again.mean_ll)
    wide = torch.full((N, cols + 5), float("nan"), dtype=torch.float64, device="cuda")
    wide[:, 2:2 + cols] = torch.from_numpy(Z).cuda()
    view = wide[:, 2:2 + cols]
    assert view.stride(0) == cols + 5 and not view.is_contiguous()
    for pts, samples in ((view, th3), (view, torch.from_numpy(th3).cuda()), (Z, torch.from_numpy(th3).cuda()), (Z, th3),
                         (torch.from_numpy(Z).cuda(), th3.reshape(-1, D))):
        res = bc.log_predictive(family, pts, samples, _dev_splits=splits)
        on_device = isinstance(pts, torch.Tensor)
        assert isinstance(res.lppd, torch.Tensor if on_device else np.ndarray)
        assert isinstance(res.mean_ll, torch.Tensor if on_device else np.ndarray)
        lppd, mean = (res.lppd.cpu().numpy(), res.mean_ll.cpu().numpy()) if on_device else (res.lppd, res.mean_ll)
        assert np.array_equal(lppd, base.lppd) and np.array_equal(mean, base.mean_ll)
        assert res.elpd == base.elpd and res.n_draws == base.n_draws


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("splits", (1, 3))
def test_non_finite_input(bc, family, splits):
    rs = np.random.RandomState(31)
    N, S, D = 40, 50, 3
    X = rs.randn(N, D)
    Z = X if family == "logistic" else np.hstack((X, rs.poisson(2.0, N)[:, None].astype(np.float64)))
    th = 0.5 * rs.randn(S, D)
    clean = bc.log_predictive(family, Z, th, _dev_splits=splits)
    assert np.all(np.isfinite(clean.lppd)) and np.all(np.isfinite(clean.mean_ll))
    # a NaN in row 5: that row's outputs alone, the others bit for bit
    bad = Z.copy()
    bad[5, 1] = np.nan
    res = bc.log_predictive(family, bad, th, _dev_splits=splits)
    others = np.arange(N) != 5
    assert np.isnan(res.lppd[5]) and np.isnan(res.mean_ll[5])
    assert np.array_equal(res.lppd[others], clean.lppd[others]) and np.array_equal(res.mean_ll[others], clean.mean_ll[others])
    # a NaN in one draw: every row
    badth = th.copy()
    badth[17, 2] = np.nan
    res = bc.log_predictive(family, Z, badth, _dev_splits=splits)
    assert np.all(np.isnan(res.lppd)) and np.all(np.isnan(res.mean_ll))


@pytest.mark.parametrize("splits", (1, 3))
def test_a_draw_of_probability_zero_leaves_lppd_finite(bc, splits):
    """Logistic: row 0 has an infinite first coordinate, draw 9 a coefficient on it of the losing sign: s = -inf, ll = -inf for
    that one draw (the others have a zero coefficient there... which against inf is NaN, so they carry a positive one: s = +inf,
    ll = 0).  lppd = log((S - 1) / S), mean_ll = -inf; the other rows are as without the infinity."""
    rs = np.random.RandomState(32)
    N, S, D = 20, 30, 3
    Z = rs.randn(N, D)
    th = np.abs(0.5 * rs.randn(S, D)) + 0.1
    th[9, 0] = -0.7
    clean = bc.log_predictive("logistic", Z, th, _dev_splits=splits)
    Zi = Z.copy()
    Zi[0, 0] = np.inf
    res = bc.log_predictive("logistic", Zi, th, _dev_splits=splits)
    assert np.isfinite(res.lppd[0]) and abs(res.lppd[0] - np.log((S - 1.0) / S)) <= 4 * U
    assert res.mean_ll[0] == -np.inf
    assert np.array_equal(res.lppd[1:], clean.lppd[1:]) and np.array_equal(res.mean_ll[1:], clean.mean_ll[1:])


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("tag,family", (("lr", "logistic"), ("poiss", "poisson")))
def test_mean_ll_sums_to_the_log_joint(bc, tag, family):
    """sum_n mean_ll[n] = mean over the draws of (log joint + |theta|^2 / 2 + D/2 log 2 pi) with unit weights: the likelihood text
    of every sampler, -log y! included.  Both sides are fp64 sums of ~10^3 same-sign terms: rtol 1e-12."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "mcmc_golden.npz"))
    Z, th = g[tag + "_Z"], g[tag + "_th"]
    D = th.shape[1]
    values, _ = bc.log_joint_grad(family, Z, None, th)
    want = (values + 0.5 * (th ** 2).sum(axis=1) + 0.5 * D * np.log(2.0 * np.pi)).mean()
    for splits in (0, 2):
        got = bc.log_predictive(family, Z, th, _dev_splits=splits).mean_ll.sum()
        print("%s: sum mean_ll %.17g, from the log joint %.17g" % (tag, got, want))
        np.testing.assert_allclose(got, want, rtol=1e-12)


# ---------------------------------------------------------------------------------------------------------------- 6
def test_limits(bc):
    import torch
    from bayesiancoresets_amd import _native
    rs = np.random.RandomState(41)
    with pytest.raises(ValueError):
        bc.log_predictive("logistic", rs.randn(5, 33), rs.randn(4, 33))
    with pytest.raises(ValueError):
        bc.log_predictive("logistic", rs.randn(5, 4), rs.randn(4, 3))
    with pytest.raises(ValueError):
        bc.log_predictive("poisson", rs.randn(5, 3), rs.randn(4, 3))            # (Poisson rows carry y: 4 columns)
    with pytest.raises(ValueError):
        bc.log_predictive("logistic", rs.randn(5, 3), np.zeros((0, 3)))
    with pytest.raises(ValueError):
        bc.log_predictive("probit", rs.randn(5, 3), rs.randn(4, 3))
    empty = bc.log_predictive("logistic", np.zeros((0, 3)), rs.randn(4, 3))
    assert empty.lppd.shape == empty.mean_ll.shape == (0,) and empty.elpd == 0.0 and empty.n_draws == 4
    empty = bc.log_predictive("poisson", torch.zeros(0, 4, dtype=torch.float64, device="cuda"), rs.randn(4, 3))
    assert isinstance(empty.lppd, torch.Tensor) and empty.lppd.shape == (0,)

    # the entry point itself
    lib = _native.load()
    N, S, D = 10, 6, 3
    Z = torch.from_numpy(rs.randn(N, D)).cuda()
    th = torch.from_numpy(rs.randn(S, D)).cuda()
    lppd, mean = torch.empty(N, dtype=torch.float64, device="cuda"), torch.empty(N, dtype=torch.float64, device="cuda")
    need = int(lib.bcx_log_predictive_scratch_bytes(N, D, S, 2))
    assert need == 2 * N * 3 * 8
    assert lib.bcx_log_predictive_scratch_bytes(N, D, S, -1) == -1 and lib.bcx_log_predictive_scratch_bytes(N, 33, S, 1) == -1
    assert lib.bcx_log_predictive_scratch_bytes(N, D, 0, 1) == -1
    work = torch.empty(need // 8, dtype=torch.float64, device="cuda")
    stream = int(torch.cuda.current_stream().cuda_stream)

    def call(splits=2, ldt=D, work_bytes=need, family=0, mean_ptr=mean.data_ptr()):
        return lib.bcx_log_predictive(stream, family, Z.data_ptr(), N, D, D, th.data_ptr(), S, ldt, splits, lppd.data_ptr(), mean_ptr,
                                      work.data_ptr(), work_bytes)

    for kw in (dict(splits=-1), dict(ldt=D - 1), dict(work_bytes=need - 8), dict(family=2)):
        assert call(**kw) == _native.ERR_ARG, kw
        assert b"bcx_log_predictive" in lib.bcx_project_last_error()
    assert call() == _native.OK
    both = lppd.cpu().numpy().copy()
    assert call(mean_ptr=None) == _native.OK                                    # (mean_dev may be NULL)
    torch.cuda.synchronize()
    assert np.array_equal(lppd.cpu().numpy(), both)
    want = bc.log_predictive("logistic", Z, th, _dev_splits=2)
    assert np.array_equal(want.lppd.cpu().numpy(), both) and np.array_equal(want.mean_ll.cpu().numpy(), mean.cpu().numpy())
