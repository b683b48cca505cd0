"""GPU: bc.energy_distance / bc.stein_discrepancy and the pair-statistic kernel under them (csrc/pairstat.hip)
against the long-double restatement (tests/discrepancy_restatement.py) at the shapes where the kernel changes path, on duplicated
draws, with scores of size 1e6, over input forms, with non-finite input, through the transform, with computed scores, and at its
limits.

The bar of tests 1, 2, 3 and 8 is the project's rule: 16 x the float64 restatement's own deviation from the long-double referee,
with a floor.  Every sum's deviation is relative to the sum of its absolute elementary terms (discrepancy_restatement.py; for
distances the sum itself).  The floor, in u = 2^-53, follows from the order csrc/pairstat.hip fixes:

    16 ceil(T / 64)   a thread adds 16 values per 64-row tile of the second operand (15 roundings, and one for the tile's sum
                      onto its running sum; the doubling of an off-diagonal tile is exact), serially over at most all tiles
    + 9               the workgroup's tree: six halving steps over the lanes, three additions over the waves
    + 9               pair_total_kernel's tree; its serial part is empty here (fewer than 256 records)
    + 2               the division by S T and the conversion of the long-double referee
    + 4 D + 32        one term: r_k one rounding, |r|^2 and the two dot products D FMAs each on factors that carry up to 2 u
                      ((D + 2) u each), q = c^2 + |r|^2 two more, the reciprocal square root 2 u on half of q's error, its third
                      and fifth powers 3 and 5 times that plus their multiplications, the four parts joined by three more: the
                      worst part, 3 |r|^2 q^(-5/2), comes to (3.5 D + 31) u

so FLOOR(T, D) = 16 ceil(T / 64) + 4 D + 52.  energy^2 = 2 m_xy - m_xx - m_yy is held relative to m_xy + m_xx + m_yy to twice the
means' floor plus 3 u (the worst case puts all of it on m_xy, which counts twice; three operations join them).

Measured on an MI355X, the largest deviations over tests 1, 2, 3 and 8, the device's / the float64 restatement's own, against
bars of 72 u and more (energy^2: 147 u): sums of distances 2.11 u / 2.25 u, sums of Stein terms 1.84 u / 1.84 u, their diagonal
2.27 u / 2.16 u, mean_xy 2.33 u / 1.95 u, mean_xx 1.93 u / 1.72 u, mean_yy 1.86 u / 1.67 u, energy^2 2.09 u / 1.85 u, ksd^2
1.84 u / 1.84 u; the U-statistic of test 4 0.13 u / 0.13 u."""
import math
import os

import numpy as np
import pytest

import discrepancy_restatement as restate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
SPLITS = (0, 1, 2, 3, 7)
LD = np.longdouble

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bc():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import bayesiancoresets_amd as bc
    return bc


@pytest.fixture(scope="module")
def pair_stat(bc):
    from bayesiancoresets_amd import discrepancy
    return discrepancy._pair_stat


def FLOOR(T, D):
    return 16 * ((T + 63) // 64) + 4 * D + 52


SEEN = {"device": {}, "float64": {}}


def _held(label, what, got, ref, f64, mag, floor_u):
    """One quantity against the referee: its deviation and the float64 restatement's in units of `mag`, the bar, the assertion."""
    mag = LD(mag)
    ddev = float(abs(LD(got) - LD(ref)) / mag) if np.isfinite(got) else np.inf
    d64 = float(abs(LD(f64) - LD(ref)) / mag)
    bar = max(16.0 * d64, floor_u * U)
    for who, d in (("device", ddev), ("float64", d64)):
        SEEN[who][what] = max(SEEN[who].get(what, 0.0), d)
    print("%s %s: device %.3g u, float64 %.3g u, bar %.3g u | so far device %.3g u float64 %.3g u"
          % (label, what, ddev / U, d64 / U, bar / U, SEEN["device"][what] / U, SEEN["float64"][what] / U))
    assert ddev <= bar, (label, what, ddev / U, bar / U)
    return bar


# ---------------------------------------------------------------------------------------------------------------- 1
SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 300)       # around one, two and several 64-row tiles
DS = (1, 3, 4, 31, 32)
# 45 of the 405 shapes: every S five times, every T five times (the offset 1 + i // 9 moves T against S), every D nine times
EDGE_SHAPES = tuple((SIZES[i % 9], SIZES[(i + 1 + i // 9) % 9], DS[i % 5]) for i in range(45))
assert {c[0] for c in EDGE_SHAPES} == set(SIZES) and {c[1] for c in EDGE_SHAPES} == set(SIZES) and {c[2] for c in EDGE_SHAPES} == set(DS)
assert len(set(EDGE_SHAPES)) == 45


def edge_inputs(S, T, D, seed):
    """Seeded draws and scores: X around 0 with unequal scales per coordinate, Y shifted and wider, scores of a few units."""
    rs = np.random.RandomState(1000 + seed)
    scale = 0.5 + rs.rand(D)
    X = rs.randn(S, D) * scale
    Y = 0.3 + 1.5 * rs.randn(T, D) * scale
    return X, Y, 3.0 * rs.randn(S, D), 2.0 * rs.randn(T, D) - 0.5


@pytest.mark.parametrize("case", range(45))
def test_edges_against_the_long_double_referee(bc, pair_stat, case):
    S, T, D = EDGE_SHAPES[case]
    X, Y, GX, GY = edge_inputs(S, T, D, case)
    c = 0.7 + 0.1 * (case % 7)
    label = "S %d T %d D %d" % (S, T, D)
    ref, f64 = {}, {}
    for dtype, into in ((LD, ref), (np.float64, f64)):
        into["d_xy"] = restate.distance_sum(X, Y, dtype)
        into["d_xx"] = restate.distance_sum(X, X, dtype)
        into["s_xy"] = restate.stein_sum(X, GX, Y, GY, c, dtype)
        into["s_xx"] = restate.stein_sum(X, GX, X, GX, c, dtype)
        into["e"] = restate.energy_distance(X, Y, dtype)
        into["k"] = restate.stein_discrepancy(X, GX, c, dtype)
    tiny = LD(np.finfo(np.float64).tiny)
    for splits in SPLITS:
        lab = "%s splits %d" % (label, splits)
        total, diag = pair_stat(0, X, None, Y, None, splits=splits)
        _held(lab, "distances", total, ref["d_xy"][0], f64["d_xy"][0], ref["d_xy"][1], FLOOR(T, D))
        assert diag == 0.0
        total, diag = pair_stat(0, X, splits=splits)
        _held(lab + " sym", "distances", total, ref["d_xx"][0], f64["d_xx"][0], max(ref["d_xx"][1], tiny), FLOOR(S, D))
        assert diag == 0.0
        total, diag = pair_stat(1, X, GX, Y, GY, c=c, splits=splits)
        _held(lab, "Stein terms", total, ref["s_xy"][0], f64["s_xy"][0], ref["s_xy"][1], FLOOR(T, D))
        assert diag == 0.0
        total, diag = pair_stat(1, X, GX, c=c, splits=splits)
        _held(lab + " sym", "Stein terms", total, ref["s_xx"][0], f64["s_xx"][0], ref["s_xx"][1], FLOOR(S, D))
        _held(lab + " sym", "Stein diagonal", diag, ref["s_xx"][2], f64["s_xx"][2], ref["s_xx"][2], FLOOR(S, D))
        # the public functions on the same input
        e = bc.energy_distance(X, Y, _dev_splits=splits)
        assert (e.n_x, e.n_y) == (S, T) and e.distance == math.sqrt(max(e.value, 0.0))
        scale = ref["e"][1] + ref["e"][2] + ref["e"][3]
        for name, i, n in (("mean_xy", 1, T), ("mean_xx", 2, S), ("mean_yy", 3, T)):
            _held(lab, name, getattr(e, name), ref["e"][i], f64["e"][i], max(ref["e"][i], tiny), FLOOR(n, D))
        _held(lab, "energy^2", e.value, ref["e"][0], f64["e"][0], scale, 2 * FLOOR(max(S, T), D) + 3)
        k = bc.stein_discrepancy(X, GX, c=c, _dev_splits=splits)
        assert k.n_draws == S and k.ksd == math.sqrt(max(k.value, 0.0))
        _held(lab, "ksd^2", k.value, ref["k"][0], f64["k"][0], ref["k"][2], FLOOR(S, D))


# ---------------------------------------------------------------------------------------------------------------- 2
def duplicated(S, D, seed):
    """A third of the rows repeat the row before exactly, a third differ from it by 1e-9 relative (what rejected and barely moved
    proposals leave in a chain); centred far from the origin, where |x|^2 + |y|^2 - 2 x.y would lose the distance."""
    rs = np.random.RandomState(seed)
    X = 40.0 + rs.randn(S, D)
    for i in range(1, S):
        if i % 3 == 1:
            X[i] = X[i - 1]
        elif i % 3 == 2:
            X[i] = X[i - 1] * (1.0 + 1e-9 * rs.randn(D))
    return X


@pytest.mark.parametrize("splits", SPLITS)
def test_duplicates_and_near_duplicates(bc, pair_stat, splits):
    S, D = 200, 5
    X = duplicated(S, D, 7)
    ref, f64 = restate.energy_distance(X, X, LD), restate.energy_distance(X, X, np.float64)
    scale = ref[1] + ref[2] + ref[3]
    for label, other in (("same buffer", X), ("a copy", X.copy())):
        e = bc.energy_distance(X, other, _dev_splits=splits)
        bar = _held("duplicates, %s, splits %d" % (label, splits), "energy^2", e.value, ref[0], f64[0], scale, 2 * FLOOR(S, D) + 3)
        assert abs(e.value) <= bar * float(scale)                               # (the referee's value is 0 to its own rounding)
        mean_bar = _held("duplicates, %s, splits %d" % (label, splits), "mean_xx", e.mean_xx, ref[2], f64[2], ref[2], FLOOR(S, D))
        _held("duplicates, %s, splits %d" % (label, splits), "mean_xy", e.mean_xy, ref[1], f64[1], ref[1], FLOOR(S, D))
        # the symmetric path (tiles j >= i, doubled) and the general path see the same pairs
        assert abs(e.mean_xx - e.mean_xy) <= mean_bar * float(ref[2])
    # exact duplicates alone: every distance is 0 or the distance of two distinct rows -- a sample of one repeated row is at 0
    one = np.repeat(X[:1], 70, axis=0)
    assert pair_stat(0, one, splits=splits) == (0.0, 0.0) and pair_stat(0, one, None, one.copy(), None, splits=splits) == (0.0, 0.0)


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("splits", SPLITS)
def test_large_scores_that_cancel(bc, pair_stat, splits):
    """Scores of size 1e6 (full-data gradients at N = 10^6 away from the mode) with random signs: g_x . g_y of size 1e12 D cancels
    over the pairs to a sum far below the sum of its absolute terms, which is what the error is relative to."""
    rs = np.random.RandomState(13)
    S, T, D = 129, 70, 4
    X, Y = rs.randn(S, D), 0.2 + rs.randn(T, D)
    GX, GY = 1e6 * rs.randn(S, D), 1e6 * rs.randn(T, D)
    ref, f64 = restate.stein_sum(X, GX, X, GX, 1.0, LD), restate.stein_sum(X, GX, X, GX, 1.0, np.float64)
    total, diag = pair_stat(1, X, GX, splits=splits)
    _held("large scores sym splits %d" % splits, "Stein terms", total, ref[0], f64[0], ref[1], FLOOR(S, D))
    _held("large scores sym splits %d" % splits, "Stein diagonal", diag, ref[2], f64[2], ref[2], FLOOR(S, D))
    ref2, f642 = restate.stein_sum(X, GX, Y, GY, 1.0, LD), restate.stein_sum(X, GX, Y, GY, 1.0, np.float64)
    assert abs(ref2[0]) < 0.2 * ref2[1]                                         # (it does cancel)
    total, _ = pair_stat(1, X, GX, Y, GY, splits=splits)
    _held("large scores splits %d" % splits, "Stein terms", total, ref2[0], f642[0], ref2[1], FLOOR(T, D))
    k = bc.stein_discrepancy(X, GX, _dev_splits=splits)
    want = restate.stein_discrepancy(X, GX, 1.0, LD)
    _held("large scores splits %d" % splits, "ksd^2", k.value, want[0], restate.stein_discrepancy(X, GX, 1.0, np.float64)[0], want[2], FLOOR(S, D))


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("S,D", ((2, 3), (65, 1), (130, 32)))
def test_u_statistic(bc, S, D):
    """(total - diagonal) / (S (S - 1)): two sums, each within its bar of the sum of the absolute terms, so twice the bar."""
    rs = np.random.RandomState(17 + S)
    X, G = rs.randn(S, D), 2.0 * rs.randn(S, D)
    ref, f64 = restate.stein_discrepancy(X, G, 1.2, LD), restate.stein_discrepancy(X, G, 1.2, np.float64)
    mag = ref[2] * S / (S - 1)
    for splits in (0, 3):
        k = bc.stein_discrepancy(X, G, c=1.2, _dev_splits=splits)
        d64 = float(abs(LD(f64[1]) - ref[1]) / mag)
        ddev = float(abs(LD(k.u_statistic) - ref[1]) / mag)
        print("u_statistic S %d D %d: device %.3g u, float64 %.3g u" % (S, D, ddev / U, d64 / U))
        assert ddev <= 2 * max(16 * d64, FLOOR(S, D) * U)
        assert k.u_statistic < k.value                                          # (the diagonal terms D / c^3 + |g|^2 / c are positive)


def test_u_statistic_of_one_draw_is_nan(bc):
    k = bc.stein_discrepancy(np.array([[0.3, -0.2]]), np.array([[1.0, 2.0]]), c=2.0)
    assert math.isnan(k.u_statistic) and k.n_draws == 1
    assert k.value == pytest.approx(2 / 8.0 + 5.0 / 2.0, rel=1e-15)             # (k_p(x, x) = D / c^3 + |g|^2 / c)
    e = bc.energy_distance(np.array([[0.3, -0.2]]), np.array([[0.3, 0.2]]))
    assert e.value == pytest.approx(0.8, rel=1e-15) and e.mean_xx == 0.0 and e.mean_yy == 0.0


# ---------------------------------------------------------------------------------------------------------------- 5, 6
@pytest.mark.parametrize("splits", (0, 3))
def test_input_forms_give_the_same_bits(bc, splits):
    import torch
    rs = np.random.RandomState(21)
    chains, draws, D, T = 4, 33, 5, 77
    X3, G3, Y = rs.randn(chains, draws, D), rs.randn(chains, draws, D), 0.1 + rs.randn(T, D)
    X, G = X3.reshape(-1, D), G3.reshape(-1, D)

    def same(e, k, e0, k0):
        assert (e.value, e.mean_xy, e.mean_xx, e.mean_yy, e.n_x, e.n_y) == (e0.value, e0.mean_xy, e0.mean_xx, e0.mean_yy, e0.n_x, e0.n_y)
        assert (k.value, k.u_statistic, k.ksd, k.n_draws) == (k0.value, k0.u_statistic, k0.ksd, k0.n_draws)

    e0, k0 = bc.energy_distance(X, Y, _dev_splits=splits), bc.stein_discrepancy(X, G, c=0.9, _dev_splits=splits)
    assert all(isinstance(v, float) for v in (e0.value, e0.distance, e0.mean_xy, e0.mean_xx, e0.mean_yy, k0.value, k0.ksd, k0.u_statistic))
    same(bc.energy_distance(X, Y, _dev_splits=splits), bc.stein_discrepancy(X, G, c=0.9, _dev_splits=splits), e0, k0)   # (two calls)
    same(bc.energy_distance(X3, Y, _dev_splits=splits), bc.stein_discrepancy(X3, G3, c=0.9, _dev_splits=splits), e0, k0)
    # every other column of a wider device tensor
    wide_x = torch.full((chains * draws, 2 * D), float("nan"), dtype=torch.float64, device="cuda")
    wide_g = torch.full((chains * draws, 2 * D), float("nan"), dtype=torch.float64, device="cuda")
    wide_x[:, ::2], wide_g[:, ::2] = torch.from_numpy(X).cuda(), torch.from_numpy(G).cuda()
    vx, vg = wide_x[:, ::2], wide_g[:, ::2]
    assert vx.stride() == (2 * D, 2)
    same(bc.energy_distance(vx, torch.from_numpy(Y).cuda(), _dev_splits=splits), bc.stein_discrepancy(vx, vg, c=0.9, _dev_splits=splits), e0, k0)
    # rows of a wider device tensor: unit column stride, read in place
    pad_x = torch.full((chains * draws, D + 5), float("nan"), dtype=torch.float64, device="cuda")
    pad_g = torch.full((chains * draws, D + 3), float("nan"), dtype=torch.float64, device="cuda")
    pad_x[:, 2:2 + D], pad_g[:, 1:1 + D] = torch.from_numpy(X).cuda(), torch.from_numpy(G).cuda()
    px, pg = pad_x[:, 2:2 + D], pad_g[:, 1:1 + D]
    assert px.stride() == (D + 5, 1) and not px.is_contiguous()
    same(bc.energy_distance(px, Y, _dev_splits=splits), bc.stein_discrepancy(px, pg, c=0.9, _dev_splits=splits), e0, k0)
    same(bc.energy_distance(torch.from_numpy(X3).cuda(), torch.from_numpy(Y).cuda(), _dev_splits=splits),
         bc.stein_discrepancy(torch.from_numpy(X3).cuda(), G3, c=0.9, _dev_splits=splits), e0, k0)
    # max_draws = K: rows floor(i S / K) of the flattened draws, each side
    K, n = 50, chains * draws
    rows_x, rows_y = (np.arange(K) * n) // K, (np.arange(K) * T) // K
    e1 = bc.energy_distance(X[rows_x], Y[rows_y], _dev_splits=splits)
    k1 = bc.stein_discrepancy(X[rows_x], G[rows_x], c=0.9, _dev_splits=splits)
    same(bc.energy_distance(X3, Y, max_draws=K, _dev_splits=splits), bc.stein_discrepancy(X3, G3, c=0.9, max_draws=K, _dev_splits=splits), e1, k1)
    same(bc.energy_distance(px, torch.from_numpy(Y).cuda(), max_draws=K, _dev_splits=splits),
         bc.stein_discrepancy(px, pg, c=0.9, max_draws=K, _dev_splits=splits), e1, k1)
    assert e1.n_x == e1.n_y == k1.n_draws == K
    same(bc.energy_distance(X, Y, max_draws=10 ** 6, _dev_splits=splits), bc.stein_discrepancy(X, G, c=0.9, max_draws=n, _dev_splits=splits), e0, k0)


# ---------------------------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("what", ("nan", "inf", "two infs"))
@pytest.mark.parametrize("where", ("first", "middle", "last"))
def test_non_finite_input_gives_a_non_finite_value(bc, what, where):
    rs = np.random.RandomState(31)
    S, T, D = 130, 67, 3                                                        # (the last row sits alone in a third tile)
    X, Y, G = rs.randn(S, D), rs.randn(T, D), rs.randn(S, D)
    assert np.isfinite(bc.energy_distance(X, Y).value) and np.isfinite(bc.stein_discrepancy(X, G).value)

    def spoil(A):
        A = A.copy()
        n = A.shape[0]
        row = {"first": 0, "middle": n // 2, "last": n - 1}[where]
        A[row, 1] = np.nan if what == "nan" else np.inf
        if what == "two infs":
            A[(row + n // 3) % n, 1] = np.inf
        return A

    for splits in (0, 3):
        for e in (bc.energy_distance(spoil(X), Y, _dev_splits=splits), bc.energy_distance(X, spoil(Y), _dev_splits=splits)):
            assert not np.isfinite(e.value) and not np.isfinite(e.distance)
        for k in (bc.stein_discrepancy(spoil(X), G, _dev_splits=splits), bc.stein_discrepancy(X, spoil(G), _dev_splits=splits)):
            assert not np.isfinite(k.value) and not np.isfinite(k.ksd) and not np.isfinite(k.u_statistic)


# ---------------------------------------------------------------------------------------------------------------- 8
@pytest.mark.parametrize("D", (3, 32))
def test_transform(bc, D):
    """theta = mu + W^T xi: the functions given theta, the score in theta, W and mu against themselves given xi = W^-T (theta - mu)
    and W score formed on the host.  The referee forms xi in long double; the float64 restatement takes the host's float64 xi, so
    its deviation carries what forming xi in float64 costs, and 16 x that is the bar."""
    rs = np.random.RandomState(41 + D)
    S, T = 129, 80
    W = np.eye(D) * 0.05 + 0.01 * rs.randn(D, D) / np.sqrt(D)                   # (a posterior of width 0.05, mildly correlated)
    mu = rs.randn(D)
    xi, xi_y = rs.randn(S, D), 0.2 + rs.randn(T, D)
    theta, theta_y = mu + xi.dot(W), mu + xi_y.dot(W)
    g_theta = -np.linalg.solve(W, xi.T).T                                       # (the score of N(mu, W^T W) in theta)
    Winv_ld = np.linalg.inv(W).astype(LD)
    ref_xi, ref_y, ref_g = (theta.astype(LD) - mu.astype(LD)).dot(Winv_ld), (theta_y.astype(LD) - mu.astype(LD)).dot(Winv_ld), g_theta.astype(LD).dot(W.T.astype(LD))
    host_xi, host_y, host_g = (theta - mu).dot(np.linalg.inv(W)), (theta_y - mu).dot(np.linalg.inv(W)), g_theta.dot(W.T)
    ref_k, f64_k = restate.stein_discrepancy(ref_xi, ref_g, 1.0, LD), restate.stein_discrepancy(host_xi, host_g, 1.0, np.float64)
    ref_e, f64_e = restate.energy_distance(ref_xi, ref_y, LD), restate.energy_distance(host_xi, host_y, np.float64)
    scale = ref_e[1] + ref_e[2] + ref_e[3]
    for label, k, e in (("transform", bc.stein_discrepancy(theta, g_theta, transform=W, center=mu), bc.energy_distance(theta, theta_y, transform=W, center=mu)),
                        ("host xi", bc.stein_discrepancy(host_xi, host_g), bc.energy_distance(host_xi, host_y))):
        _held("%s D %d" % (label, D), "ksd^2", k.value, ref_k[0], f64_k[0], ref_k[2], FLOOR(S, D))
        _held("%s D %d" % (label, D), "energy^2", e.value, ref_e[0], f64_e[0], scale, 2 * FLOOR(S, D) + 3)
    # and it matters: the metric is the frame's, not theta's: distances in theta are 0.05 of those in xi
    assert bc.energy_distance(theta, theta_y).value < 0.2 * bc.energy_distance(theta, theta_y, transform=W, center=mu).value


# ---------------------------------------------------------------------------------------------------------------- 9
def test_computed_scores_are_log_joint_grad(bc):
    import torch
    rs = np.random.RandomState(51)
    N, D, chains, draws = 200, 3, 4, 30
    Xd = rs.randn(N, D)
    Z = np.where(rs.rand(N) < 1 / (1 + np.exp(-Xd.dot([1.0, -0.5, 0.3]))), 1.0, -1.0)[:, None] * Xd
    th = 0.3 * rs.randn(chains, draws, D) + [1.0, -0.5, 0.3]
    g = bc.log_joint_grad("logistic", Z, None, th.reshape(-1, D))[1]
    want = bc.stein_discrepancy(th, g.reshape(chains, draws, D), c=0.5)
    got = bc.stein_discrepancy(th, family="logistic", pts=Z, c=0.5)
    assert (got.value, got.u_statistic, got.n_draws) == (want.value, want.u_statistic, want.n_draws)
    got = bc.stein_discrepancy(torch.from_numpy(th).cuda(), family="logistic", pts=torch.from_numpy(Z).cuda(), c=0.5)
    assert (got.value, got.u_statistic) == (want.value, want.u_statistic)
    # weights, thinning before the score, and the frame
    w = rs.rand(N)
    rows = (np.arange(40) * chains * draws) // 40
    gw = bc.log_joint_grad("logistic", Z, w, th.reshape(-1, D)[rows])[1]
    W, mu = np.eye(D) * 0.2, th.reshape(-1, D).mean(axis=0)
    want = bc.stein_discrepancy(th.reshape(-1, D)[rows], gw, transform=W, center=mu)
    got = bc.stein_discrepancy(th, family="logistic", pts=Z, wts=w, max_draws=40, transform=W, center=mu)
    assert (got.value, got.u_statistic, got.n_draws) == (want.value, want.u_statistic, 40)


# ---------------------------------------------------------------------------------------------------------------- 10
def test_limits(bc):
    import torch
    from bayesiancoresets_amd import _native, discrepancy
    rs = np.random.RandomState(61)
    x, g, pts = rs.randn(10, 3), rs.randn(10, 3), rs.randn(20, 3)
    with pytest.raises(ValueError):
        bc.energy_distance(rs.randn(5, 33), rs.randn(4, 33))
    with pytest.raises(ValueError):
        bc.energy_distance(x, rs.randn(4, 4))
    with pytest.raises(ValueError):
        bc.stein_discrepancy(rs.randn(5, 33), rs.randn(5, 33))
    with pytest.raises(ValueError):
        bc.stein_discrepancy(x, rs.randn(10, 4))
    with pytest.raises(ValueError):
        bc.stein_discrepancy(x, family="logistic", pts=rs.randn(20, 4))         # (logistic rows have D columns)
    with pytest.raises(ValueError):
        bc.stein_discrepancy(x, g, family="logistic", pts=pts)
    with pytest.raises(ValueError):
        bc.stein_discrepancy(x)
    # the size limit: the argument check alone, nothing of that size is allocated
    lib = _native.load()
    big = discrepancy.MAX_DRAWS
    assert lib.bcx_pair_stat_scratch_bytes(big, big, 32, 1) == (big // 64) * 16
    assert lib.bcx_pair_stat_scratch_bytes(big, 0, 32, 0) <= 2 * (big // 64) * 16          # (of order (S / tile) x ranges records)
    for bad in ((big + 1, 5, 3, 0), (5, big + 1, 3, 0), (0, 5, 3, 0), (5, -1, 3, 0), (5, 5, 33, 0), (5, 5, 0, 0), (5, 5, 3, -1), (5, 5, 3, 1025)):
        assert lib.bcx_pair_stat_scratch_bytes(*bad) == -1, bad
    assert lib.bcx_pair_stat_scratch_bytes(130, 0, 3, 2) == 3 * 2 * 16 and lib.bcx_pair_stat_scratch_bytes(130, 65, 3, 7) == 3 * 7 * 16
    huge = np.broadcast_to(np.zeros((1, 3)), (big + 1, 3))
    with pytest.raises(ValueError, match="at most"):
        bc.energy_distance(x, huge)
    with pytest.raises(ValueError, match="at most"):
        bc.stein_discrepancy(huge, huge)

    # the entry point itself
    S, T, D = 10, 6, 3
    A, GA = torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda()
    B, GB = torch.from_numpy(rs.randn(T, D)).cuda(), torch.from_numpy(rs.randn(T, D)).cuda()
    out = torch.zeros(2, dtype=torch.float64, device="cuda")
    need = int(lib.bcx_pair_stat_scratch_bytes(S, T, D, 2))
    work = torch.empty(need // 8, dtype=torch.float64, device="cuda")
    stream = int(torch.cuda.current_stream().cuda_stream)

    def call(kind=1, a=A.data_ptr(), lda=D, ga=GA.data_ptr(), b=B.data_ptr(), nb=T, ldb=D, gb=GB.data_ptr(), c=1.0, splits=2, work_bytes=need, o=out.data_ptr()):
        return lib.bcx_pair_stat(stream, kind, a, S, lda, ga, D, b, nb, ldb, gb, D, D, c, splits, o, work.data_ptr(), work_bytes)

    for kw in (dict(kind=2), dict(a=None), dict(lda=D - 1), dict(ldb=D - 1), dict(ga=None), dict(gb=None), dict(c=0.0), dict(c=-1.0),
               dict(c=float("inf")), dict(c=float("nan")), dict(splits=-1), dict(splits=1025), dict(work_bytes=need - 8), dict(nb=0), dict(o=None)):
        assert call(**kw) == _native.ERR_ARG, kw
        assert b"bcx_pair_stat" in lib.bcx_project_last_error()
    assert call() == _native.OK
    torch.cuda.synchronize()
    assert tuple(out.cpu().tolist()) == discrepancy._pair_stat(1, A, GA, B, GB, c=1.0, splits=2)
    assert call(kind=0, ga=None, gb=None, c=0.0) == _native.OK                  # (distances read neither scores nor c)
    torch.cuda.synchronize()
    assert tuple(out.cpu().tolist()) == discrepancy._pair_stat(0, A, None, B, None, splits=2)
