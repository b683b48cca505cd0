"""A helper, not a test: the inputs tests/test_gpu_lik_point.py gives the device, built here so that
tests/test_lik_point_referee_host.py can check on the CPU, with the long-double referee (tests/lik_point_referee.py), what each of
them presumes before a GPU sees it.

* ``host_grid`` / ``device_predictors``: the predictors the point terms are compared at.
* ``h_probe``: two points in D = 1 from which ONE Newton step of the Laplace samplers (warm start 1, max_iter 1) shows
  h(s0) in the covariance factor W = (1 - sum_j w_j h_j x_j^2)^(-1/2).  The first point has x = s0 (its predictor at the start
  is s0 exactly); the second makes the gradient at the start vanish, so that the accepted step -- whatever fraction of it the
  step halving takes -- leaves the iterate where it was.
  A second point with h = 0 exactly cannot do that everywhere: theta . grad(log-likelihood) = sum_j w_j g_j s_j has to equal
  |theta|^2 > 0, and g_j s_j <= 0 wherever a point's h vanishes (Poisson s < -746 or y = 0, s >> 0; logistic -s >= 100), so
  no such point balances a first point with g(s0) s0 <= 0 -- every Poisson predictor of the band -745 .. -355 among them.
  The second point therefore sits at a predictor s' next to 0 (g(s') > 0, sign of s' as needed), so close that its own
  curvature w' |h'| s'^2 is at most 2^-10: it enters the expected W through the referee and the bound with its own term.
  The weight of the first point is 1 / (|h| x^2) (then w |h| x^2 = 1) where |h| > 1e-30, else 1, and at most what keeps
  |w g x| <= 2^20: the two addends of the gradient cancel to 2^-53 of their size, and that remainder must not move the iterate.
* ``end_to_end_case``: six Poisson points in D = 2 and a warm start that puts three predictors into the band."""
import numpy as np

import lik_point_referee as ref

LD = np.longdouble
Y_VALUES = (0.0, 1.0, 3.0, 50.0, 1e3, 1e6)
BRANCH_POINTS = (-100 - 1e-3, -100 + 1e-3, 0.0, -0.0, -355.0, -372.5, -745.2)
LOGISTIC_ONLY = (800.0, -800.0)
STEP_MARGIN = 2.0 ** -30          # the referee's Newton step of an h probe is at most this
GRAD_CAP = 2.0 ** 20              # (the band's largest |g x| at weight 1 is 1000 x 745: below it)


def host_grid(family):
    """4001 points on [-745, 700], 4000 uniform in [-60, 60], the branch points."""
    rs = np.random.RandomState(2024)
    g = np.concatenate((np.linspace(-745.0, 700.0, 4001), rs.uniform(-60.0, 60.0, 4000), BRANCH_POINTS))
    return np.concatenate((g, LOGISTIC_ONLY)) if family == "logistic" else g


def _sides(v):
    return [np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)]


def device_predictors(family):
    """About 400 of the host grid: every 12th of the 4001, 50 of the uniform ones, the branch points, and both neighbours of
    every predictor at which csrc/lik_point.h changes branch (-100; 0; -300, below which the Poisson g and h take their small-rate forms)."""
    g = host_grid(family)
    extra = _sides(-100.0) + _sides(-300.0) + _sides(0.0) + [-700.0, -372.0, -373.0, -374.5, -371.5, 37.0, -37.5, 100.0]
    return np.concatenate((g[:4001:12], g[4001:8001:80], g[8001:], extra))


def _one(family, s, y):
    ll, g, h = ref.point_terms(family, np.array([s], dtype=np.float64), np.array([y], dtype=np.float64))
    return ll[0], g[0], h[0]


def h_probe(family, s0, y=0.0):
    """dict(Z, w, t0): see the module's text.  s0 != 0."""
    assert s0 != 0.0 and np.isfinite(s0)
    t0 = 1.0
    _, g, h = _one(family, s0, y)
    x2 = LD(s0) * LD(s0)
    w = 1.0 if abs(h) <= 1e-30 else float(1 / (abs(h) * x2))
    if abs(w * g * s0) > GRAD_CAP:
        w = float(GRAD_CAP / abs(g * s0))
    r = LD(t0) * t0 - LD(w) * g * s0                     # what the second point's w' g' s' has to supply
    yc = 1.0                                             # (Poisson: g(0) = 0.5 / log 2 - 0.5 > 0 at y = 1)
    delta = 2.0 ** -10 * min(1.0, abs(s0))
    for _ in range(2):                                   # its curvature is linear in delta next to 0: one correction settles it
        sc = float(np.copysign(delta, float(r)))
        _, gc, hc = _one(family, sc, yc)
        wc = r / (gc * sc)
        curv = float(wc * abs(hc) * sc * sc)
        if curv <= 2.0 ** -10:
            break
        delta *= 2.0 ** np.floor(np.log2(2.0 ** -10 / curv))
    Z = np.array([[s0, y], [sc, yc]]) if family == "poisson" else np.array([[s0], [sc]])
    return dict(family=family, Z=Z, w=np.array([w, float(wc)]), t0=t0, s0=s0, y=y)


def h_probe_start(case):
    """(Newton matrix, step) of the referee at the probe's start."""
    _, H, step = ref.newton_step(case["family"], case["Z"], case["w"], np.array([case["t0"]]))
    return H[0, 0], step[0]


def h_probe_expected(case, theta1):
    """(W, lowest, highest admissible W) at the iterate theta1 the DEVICE landed on (a float64): the referee's
    (1 - sum_j w_j h_j x_j^2)^(-1/2) at the predictors the device forms there (one float64 product each), the matrix entry
    moved either way by 16 U sum_j scale_h_j w_j x_j^2."""
    fam, Z, w = case["family"], case["Z"], case["w"].astype(LD)
    x = Z[:, 0]
    s1 = x * np.float64(theta1)
    yv = Z[:, 1] if fam == "poisson" else np.zeros(2)
    h = ref.point_terms(fam, s1, yv)[2]
    sh = ref.scales(fam, s1, yv)[2]
    xl = x.astype(LD)
    H = 1 - (w * h * xl * xl).sum()
    dH = 16 * ref.U * (w * sh * xl * xl).sum()
    with np.errstate(all="ignore"):
        return 1 / np.sqrt(H), 1 / np.sqrt(H + dH), (1 / np.sqrt(H - dH) if H - dH > 0 else LD(np.inf))


def h_probe_cases(family):
    """(s0, y) of every probe: a spread over the whole range, both sides of the branch points, and -- Poisson -- 48 predictors of
    the band -745 < s0 < -355 (18 of them in (-372.5, -355)) at y = 0, 3, 1000, where the weight is 1."""
    spread = [-700.0, -500.0, -300.001, -299.999, -200.0, -100.001, -99.999, -60.0, -37.5, -20.0, -8.0, -3.0, -1.0, -0.25,
              0.25, 1.0, 3.0, 8.0, 20.0, 37.0, 60.0, 99.999, 100.001, 300.0, 700.0]
    if family == "logistic":
        return [(s, 0.0) for s in spread + [-800.0, 800.0]]
    out = [(s, y) for s in spread for y in Y_VALUES]
    band = np.concatenate((np.linspace(-744.5, -373.0, 30), np.linspace(-372.4, -355.1, 18)))
    return out + [(float(s), y) for s in band for y in (0.0, 3.0, 1e3)]


def end_to_end_case():
    """(Z (6 x 3), w (6), warm start (2)): Poisson, D = 2.  At the warm start the predictors of the first two points lie in
    (-745, -373) and that of the third in (-372, -356)."""
    X = np.array([[9.5, 1.0], [11.0, -0.5], [9.1, 0.3], [0.5, 1.0], [-0.3, 0.8], [0.2, -1.0]])
    y = np.array([0.0, 1.0, 0.0, 2.0, 1.0, 3.0])
    w = np.array([1.5, 0.7, 2.0, 3.0, 1.0, 2.5])
    th0 = np.array([-40.0, 1.0])
    s = X.dot(th0)
    assert -745 < s[0] < -373 and -745 < s[1] < -373 and -372 < s[2] < -356
    return np.hstack((X, y[:, None])), w, th0
