"""CPU only: the long-double referee of the linear-regression posterior (tests/linreg_post_referee.py) and the cases
(tests/linreg_post_cases.py) before tests/test_gpu_linreg_post.py holds the device to them.

(1) the referee against mpmath at 50 digits on the cases with D <= 40: P, L_R, L_R^-1 and mu_R, each measured in the metric of the
    50-digit factor, within 2^-8 of what the reference's algorithm itself reaches in float64 on that case (long double carries 11
    more bits than double through the same loops; 2^-8 leaves the factor 8 by which two orders of one algorithm differ) -- the
    referee's own error then moves a device ratio of 64 by less than half a percent;
(2) what the cases presume, from the reference's algorithm and the referee alone: cond(P) <= 1e10; the reference's algorithm in
    float64, in LAPACK's order (tests/models.py linreg_weighted_post) and by plain loops (the referee's loops at float64), reaches
    e_cov <= 1e-6 and e_mean <= 1e-3; the two lie within a factor 8 of each other once the storage floor is taken into account
    (the spread the device bound's margin of 64 rests on); the cases meant for the rank-k kernels have k <= 4 + 2 ceil(D / 32).
    Both at the case's weights and at the second step's weights of the enqueued-loop tests."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import linreg_post_cases as cases  # noqa: E402
import linreg_post_referee as referee  # noqa: E402

LD = np.longdouble
SMALL = tuple(cid for cid in cases.IDS if cases.case(cid).D <= 40)


def test_long_double_is_wider_than_double():
    assert np.finfo(LD).eps <= 2.0 ** -63, "np.longdouble is no wider than float64 here: the referee cannot referee"


def test_the_cases_are_the_issue_table():
    assert cases.IDS == ("R1", "R2", "R3", "R4", "R5", "F1", "F2", "F3", "F4", "F5")
    shapes = {cid: (cases.case(cid).D, cases.case(cid).k) for cid in cases.IDS}
    assert shapes == {"R1": (7, 3), "R2": (24, 6), "R3": (24, 6), "R4": (33, 8), "R5": (301, 24), "F1": (40, 130), "F2": (96, 300),
                      "F3": (31, 40), "F4": (33, 12), "F5": (70, 33)}
    for cid in cases.IDS:
        c = cases.case(cid)
        assert c.pts.shape == (c.k, c.D + 1) and c.w.shape == (c.k,)
        assert c.w[1] == 0.0 or c.k <= 2
        assert (c.w < 0).any() == (cid == cases.NEGATIVE_WEIGHT)
        assert cases.case(cid) is c                                     # built once, read-only
        assert not c.pts.flags.writeable and not c.w.flags.writeable


# ---- (1) the referee against mpmath ---------------------------------------------------------------------------------------------------
def _to_mp(mp, v):
    """A long double (or a double) as an mpf, exactly."""
    v = LD(v)
    hi = np.float64(v)
    return mp.mpf(float(hi)) + mp.mpf(float(np.float64(v - LD(hi))))


def _mp_mat(mp, A):
    return [[_to_mp(mp, x) for x in row] for row in np.asarray(A)]


def _mp_chol(mp, A):
    n = len(A)
    L = [[mp.mpf(0)] * n for _ in range(n)]
    for j in range(n):
        L[j][j] = mp.sqrt(A[j][j] - mp.fsum(L[j][u] * L[j][u] for u in range(j)))
        for i in range(j + 1, n):
            L[i][j] = (A[i][j] - mp.fsum(L[i][u] * L[j][u] for u in range(j))) / L[j][j]
    return L


def _mp_lower_inverse(mp, L):
    n = len(L)
    X = [[mp.mpf(0)] * n for _ in range(n)]
    for c in range(n):
        for i in range(c, n):
            X[i][c] = ((1 if i == c else 0) - mp.fsum(L[i][u] * X[u][c] for u in range(c, i))) / L[i][i]
    return X


def _mp_mul(mp, A, B):
    Bt = list(zip(*B))
    return [[mp.fdot(ra, cb) for cb in Bt] for ra in A]


def _mp_T(A):
    return [list(r) for r in zip(*A)]


def _mp_dev_from_identity(mp, G):
    return float(max(abs(G[i][j] - (1 if i == j else 0)) for i in range(len(G)) for j in range(len(G))))


@pytest.mark.parametrize("cid", SMALL)
def test_referee_against_mpmath(cid):
    mp = pytest.importorskip("mpmath")
    c = cases.case(cid)
    b = cases.bars(cid)
    ref = b.ref
    with mp.workdps(50):
        D, k = c.D, c.k
        S0i = _mp_lower_inverse(mp, _mp_chol(mp, _mp_mat(mp, c.Sig0)))
        S0i = _mp_mul(mp, _mp_T(S0i), S0i)
        X = _mp_mat(mp, c.pts[:, :-1])
        y = [_to_mp(mp, v) for v in c.pts[:, -1]]
        w = [max(_to_mp(mp, v), mp.mpf(0)) for v in c.w]
        sig = _to_mp(mp, c.sigsq)
        P = [[S0i[i][j] + mp.fsum(w[n] * X[n][i] * X[n][j] for n in range(k)) / sig for j in range(D)] for i in range(D)]
        mu0 = [_to_mp(mp, v) for v in c.mu0]
        rhs = [mp.fdot(S0i[i], mu0) + mp.fsum(w[n] * y[n] * X[n][i] for n in range(k)) / sig for i in range(D)]
        L = _mp_chol(mp, P)
        Li = _mp_lower_inverse(mp, L)
        LiT = _mp_T(Li)
        mu = [mp.fdot(LiT[i], [mp.fdot(Li[j], rhs) for j in range(D)]) for i in range(D)]
        # the referee's four outputs in the 50-digit factor's metric
        in_metric = lambda A: _mp_mul(mp, _mp_mul(mp, Li, A), LiT)                 # L^-1 A L^-T: the identity for A = P
        e_P = _mp_dev_from_identity(mp, in_metric(_mp_mat(mp, ref.P)))
        LR = _mp_mat(mp, ref.L)
        e_L = _mp_dev_from_identity(mp, in_metric(_mp_mul(mp, LR, _mp_T(LR))))
        M = _mp_mul(mp, _mp_mat(mp, ref.Linv), L)                                  # L_R^-1 L
        e_Li = _mp_dev_from_identity(mp, _mp_mul(mp, _mp_T(M), M))                 # L^T (L_R^-T L_R^-1) L
        d = [_to_mp(mp, v) - m for v, m in zip(ref.mu, mu)]
        e_mu = float(mp.sqrt(mp.fsum(mp.fdot(col, d) ** 2 for col in _mp_T(L))))   # ||L^T d||
    own_cov = max(b.lapack[0], b.loop[0])              # (without the floor: the raw-factor test holds U to this alone)
    print("%s: referee against 50 digits: P %.3g  L %.3g  L^-1 %.3g (float64 reference %.3g)   mu %.3g (float64 reference %.3g, floor %.3g)"
          % (cid, e_P, e_L, e_Li, own_cov, e_mu, max(b.lapack[1], b.loop[1]), b.floor))
    assert max(e_P, e_L, e_Li) <= 2.0 ** -8 * own_cov
    assert e_mu <= 2.0 ** -8 * b.base_mean


# ---- (2) what the cases presume ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", (0, 1))
@pytest.mark.parametrize("cid", cases.IDS)
def test_case_preconditions(cid, step):
    c = cases.case(cid)
    b = cases.bars(cid, step)
    cond = b.ref.cond()
    print("%s step %d: D %d k %d cond(P) %.3g floor %.3g | e_cov lapack %.3g loop %.3g | e_mean lapack %.3g loop %.3g"
          % (cid, step, c.D, c.k, cond, b.floor, b.lapack[0], b.loop[0], b.lapack[1], b.loop[1]))
    assert cond <= 1e10
    for e_cov, e_mean in (b.lapack, b.loop):
        assert e_cov <= 1e-6 and e_mean <= 1e-3
    for fl, a, bb in ((2.0 * b.floor, b.lapack[0], b.loop[0]), (b.floor, b.lapack[1], b.loop[1])):
        hi, lo = max(a, bb, fl), max(min(a, bb), fl)
        assert hi <= 8.0 * lo, (hi, lo)
    if c.low_rank:
        assert c.k <= 4 + 2 * ((c.D + 31) // 32)
    else:
        assert c.k > 4 + 2 * ((c.D + 31) // 32)


def test_float64_loops_are_the_lapack_order_on_a_benign_case():
    """The loops at float64 against LAPACK where both are exact to rounding (R1): a slip in the loops would show here, not as a
    wide bar on the device."""
    c = cases.case("R1")
    S0inv = np.linalg.inv(c.Sig0)
    mu, U = referee.reference_loop(c.mu0, S0inv, c.sigsq, c.pts, c.w, np.float64)
    P = S0inv + (c.w[:, None] * c.pts[:, :-1]).T.dot(c.pts[:, :-1]) / c.sigsq
    np.testing.assert_allclose(U.dot(U.T), np.linalg.inv(P), rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(mu, np.linalg.solve(P, S0inv.dot(c.mu0) + (c.w * c.pts[:, -1]).dot(c.pts[:, :-1]) / c.sigsq), rtol=1e-10)
    assert np.all(np.triu(U, 0) == U)
