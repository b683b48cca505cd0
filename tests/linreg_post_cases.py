"""The cases tests/test_gpu_linreg_post.py holds LinregPosteriorSampler's three device paths to (csrc/svi.hip lrs_draw_kernel and
lrs_apply_kernel, csrc/lrpost.hip), built from fixed seeds; tests/test_linreg_post_referee_host.py checks what they presume.

    prior    dense: A0 A0^T / D + I, iso: 2.5 I; mu0 random
    points   randn; rbf: exp(-(t_i - c_j)^2 / (2 0.3^2)), t sorted uniform on [0, 1], c an even grid of D centres (the collinear
             design of the linear-regression experiment); scaled: randn times 10^U(-2, 2) per column
    y        5 + 3 randn
    weights  scale |randn|, or 10^U(-6, 5); w[1] = 0 where k > 2 (a point that has just entered); F3 has a negative weight, which
             the kernels clamp at zero

``low_rank`` is the form the sampler's call path must take (k <= 4 + 2 ceil(D / 32): the rank-k kernels); the R cases are also
what the enqueued loop's rank-k kernel (plan.fast) is held to, the F cases the D x D form (plan.factored)."""
import collections

import numpy as np

Case = collections.namedtuple("Case", "id D k prior points weights sigsq low_rank seed mu0 Sig0 pts w")

#        id    D    k   prior    points    weights          sigsq  low_rank  seed
_SPEC = (("R1", 7, 3, "dense", "randn", ("abs", 30.0), 0.4, True, 101),
         ("R2", 24, 6, "dense", "randn", ("abs", 1e5), 0.01, True, 102),
         ("R3", 24, 6, "iso", "rbf", ("abs", 1e5), 0.01, True, 308),
         ("R4", 33, 8, "dense", "randn", ("log", -6.0, 5.0), 0.1, True, 104),
         ("R5", 301, 24, "iso", "rbf", ("abs", 2.6e4), 1.0, True, 105),
         ("F1", 40, 130, "dense", "randn", ("abs", 1e4), 0.01, False, 201),
         ("F2", 96, 300, "iso", "rbf", ("abs", 2e3), 0.05, False, 212),
         ("F3", 31, 40, "dense", "scaled", ("abs", 100.0), 0.1, False, 203),
         ("F4", 33, 12, "dense", "randn", ("log", -6.0, 5.0), 0.1, False, 204),
         ("F5", 70, 33, "iso", "rbf", ("abs", 1e4), 0.05, False, 205))
IDS = tuple(s[0] for s in _SPEC)
RANK_K = tuple(s[0] for s in _SPEC if s[7])
FACTORED = tuple(s[0] for s in _SPEC if not s[7])
MOVING = ("R2", "R3", "R4")          # the D x D form at small k (enqueue_plan_moving): the same posteriors as the rank-k kernels'
NEGATIVE_WEIGHT = "F3"
_cache = {}


def rbf_rows(t, D):
    c = np.linspace(0.0, 1.0, D)
    return np.exp(-(t[:, None] - c[None, :]) ** 2 / (2.0 * 0.3 ** 2))


def case(cid):
    if cid in _cache:
        return _cache[cid]
    _, D, k, prior, points, weights, sigsq, low_rank, seed = _SPEC[IDS.index(cid)]
    rs = np.random.RandomState(seed)
    mu0 = rs.randn(D)
    A0 = rs.randn(D, D)                                    # (drawn for either prior: one stream per case)
    Sig0 = A0.dot(A0.T) / D + np.eye(D) if prior == "dense" else 2.5 * np.eye(D)
    if points == "rbf":
        X = rbf_rows(np.sort(rs.rand(k)), D)
    else:
        X = rs.randn(k, D)
        if points == "scaled":
            X = X * 10.0 ** rs.uniform(-2.0, 2.0, D)[None, :]
    y = 5.0 + 3.0 * rs.randn(k)
    w = weights[1] * np.abs(rs.randn(k)) if weights[0] == "abs" else 10.0 ** rs.uniform(weights[1], weights[2], k)
    if k > 2:
        w[1] = 0.0
    if cid == NEGATIVE_WEIGHT:
        w[2] = -3.0
    for a in (mu0, Sig0, w):
        a.setflags(write=False)
    pts = np.hstack((X, y[:, None]))
    pts.setflags(write=False)
    c = _cache[cid] = Case(cid, D, k, prior, points, weights, sigsq, low_rank, seed, mu0, Sig0, pts, w)
    return c


def second_weights(w):
    """The second step's weights of the enqueued-loop tests."""
    return 0.5 * np.asarray(w) + 1.0


MARGIN = 64.0
Bars = collections.namedtuple("Bars", "ref floor lapack loop bar_cov bar_mean base_cov base_mean")
_bars = {}


def bars(cid, step=0):
    """The referee of case ``cid`` at its weights (step 0) or at ``second_weights`` (step 1), the errors (e_cov, e_mean) of the
    reference's algorithm in float64 in LAPACK's order and by plain loops, and the bars of the device:

        e_device <= 64 max(e_lapack, e_loop, floor)      (2 floor for e_cov, where U is a difference of two stored draws)

    -- nothing in them comes from the device.  Computed once per (case, step) and shared."""
    key = (cid, step)
    if key not in _bars:
        import linreg_post_referee as referee
        from models import linreg_weighted_post
        c = case(cid)
        w = np.asarray(c.w) if step == 0 else second_weights(c.w)
        ref = referee.Referee(c.mu0, c.Sig0, c.sigsq, c.pts, w)
        S0inv = np.linalg.inv(c.Sig0)
        mu_a, U_a = linreg_weighted_post(c.mu0, S0inv, c.sigsq, c.pts, np.maximum(w, 0.0))
        mu_b, U_b = referee.reference_loop(c.mu0, S0inv, c.sigsq, c.pts, w, np.float64)
        lapack = (ref.e_cov(U_a), ref.e_mean(mu_a))
        loop = (ref.e_cov(U_b), ref.e_mean(mu_b))
        base_cov = max(lapack[0], loop[0], 2.0 * ref.floor)
        base_mean = max(lapack[1], loop[1], ref.floor)
        _bars[key] = Bars(ref, ref.floor, lapack, loop, MARGIN * base_cov, MARGIN * base_mean, base_cov, base_mean)
    return _bars[key]
