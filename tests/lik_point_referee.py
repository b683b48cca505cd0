"""A helper, not a test: the per-point log-likelihood of the logistic / Poisson regression models in its linear predictor s,
with its first two derivatives (what csrc/lik_point.h::lap_point computes), and the sums the kernels build from them, in
np.longdouble -- the referee of tests/test_gpu_lik_point.py and tests/test_gpu_log_joint_shapes.py.

Written from the models' definitions so that no subtraction of nearly equal numbers is left in it; it shares no code and no
branch points with the library or with tests/hmc_restatement.py (tests/test_lik_point_referee_host.py holds it to 60 digits).

    logistic, q = e^-|s|:   ll = min(s, 0) - log1p(q)      g = [s < 0 ? 1 : q] / (1 + q)      h = -q / (1 + q)^2
    Poisson, u = e^s, L = log1p(u) (the rate), m = L - u:
        ll = y log L - L       g = u (y - L) / ((1 + u) L)       h = -u / (1 + u)^2 (1 + y (-m) / L^2)
      m is the only place where the definition cancels (L -> u as s -> -inf, h -> -(1 + y/2) e^s): below u = 4 the ratio
      -m / L^2 is summed from z = u / (2 + u), log1p(u) = 2 atanh z (_curvature_ratio).

The scales the tests' bounds are stated in (what one rounding of the formula's intermediate results costs a term):
    Poisson   scale_ll = y (1 + |log rate|) + rate      scale_g = scale_h = 1 + y
    logistic  scale_ll = |ll|, at least the smallest normal double      scale_g = scale_h = 1"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53                    # the unit roundoff of the device's arithmetic
FAMILIES = ("logistic", "poisson")
_SERIES_TERMS = 64                # z <= 2/3 below u = 4: (4/9)^64 < 2^-74


def _ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD) if not (isinstance(a, np.ndarray) and a.dtype == LD) else a


def _curvature_ratio(u, L):
    """(u - log1p(u)) / log1p(u)^2 >= 0 without the cancellation (u >= 0, L = log1p(u)): below u = 4 from z = u / (2 + u), in
    which u = 2 z / (1 - z) and L = 2 atanh z = 2 z S, S = 1 + z^2 A, A = sum_{k>=1} z^(2k-2) / (2k+1); then
    u - L = 2 z^2 (1 / (1 - z) - z A) and the ratio is (1 / (1 - z) - z A) / (2 S^2) -- z^2 has dropped out."""
    small = u < 4
    z = np.where(small, u / (2 + u), 0)
    z2 = z * z
    A = np.zeros_like(z)
    for k in range(_SERIES_TERMS, 0, -1):                 # Horner in z^2 from the far end
        A = A * z2 + LD(1) / (2 * k + 1)
    S = 1 + z2 * A
    return np.where(small, (1 / (1 - z) - z * A) / (2 * S * S), (u - L) / (L * L))


def point_terms(family, s, y=None, with_h=True):
    """(ll, g, h) of every point in long double; s and y broadcast.  NaN in, NaN out in all three.  ``with_h=False``: h is None
    (the sums of the log joint do not read it)."""
    s = _ld(s)
    with np.errstate(all="ignore"):
        if family == "logistic":
            q = np.exp(-np.abs(s))
            ll = np.minimum(s, 0) - np.log1p(q)
            g = np.where(s < 0, 1 + 0 * q, q) / (1 + q)
            return ll, g, (-q / ((1 + q) * (1 + q)) if with_h else None)
        if family != "poisson":
            raise ValueError(family)
        y = _ld(y)
        u = np.exp(s)
        L = np.log1p(u)
        one = 1 + u
        ll = y * np.log(L) - L
        sig = u / one
        g = sig * (y - L) / L
        if not with_h:
            return ll, g, None
        dsig = sig / one
        return ll, g, -dsig * (1 + y * _curvature_ratio(u, L))


def scales(family, s, y=None):
    """(scale_ll, scale_g, scale_h) of every point, long double."""
    s = _ld(s)
    with np.errstate(all="ignore"):
        if family == "logistic":
            ll = point_terms(family, s, with_h=False)[0]
            one = np.ones_like(s)
            return np.maximum(np.abs(ll), LD(np.finfo(np.float64).tiny)), one, one
        y = _ld(y)
        L = np.log1p(np.exp(s))
        sg = 1 + y + 0 * s
        return y * (1 + np.abs(np.log(L))) + L, sg, sg


def log_factorial(y):
    """log y! in long double for counts y: the sum of the logs up to 64 (exactly 0 at y = 0 and 1), Stirling's series of
    lgamma(y + 1) above (its ninth term is below 2^-90 of the sum there)."""
    y64 = np.asarray(y, dtype=np.float64)
    assert np.all(y64 >= 0) and np.all(y64 == np.round(y64)), "counts"
    table = np.concatenate((np.zeros(2, dtype=LD), np.cumsum(np.log(np.arange(2, 65, dtype=LD)))))      # table[k] = log k!
    low = y64 <= 64
    x = np.where(low, 65, y64).astype(LD) + 1
    r2 = 1 / (x * x)
    coef = (LD(1) / 12, LD(-1) / 360, LD(1) / 1260, LD(-1) / 1680, LD(1) / 1188, LD(-691) / 360360, LD(1) / 156, LD(-3617) / 122400)
    acc = np.zeros_like(x)
    for c in coef[::-1]:
        acc = acc * r2 + c
    half_log_2pi = LD("0.918938533204672741780329736405617639861")
    stirling = (x - LD(0.5)) * np.log(x) - x + half_log_2pi + acc / x
    return np.where(low, table[np.where(low, y64, 0).astype(np.int64)], stirling)


LOG_2PI = LD("1.837877066409345483560659472811235279723")


def _split(family, Z, D):
    Z = np.atleast_2d(np.asarray(Z, dtype=np.float64))
    X = Z[:, :D].astype(LD)
    y = Z[:, D].astype(LD) if family == "poisson" else np.zeros(Z.shape[0], dtype=LD)
    return X, y


def point_table(family, Z, Th):
    """What the sums below read of the N points at the C rows of Th, for callers that sum it under several weightings."""
    Th = np.atleast_2d(np.asarray(Th, dtype=np.float64)).astype(LD)
    X, y = _split(family, Z, Th.shape[1])
    s = X.dot(Th.T)                                        # N x C
    ll, g, _ = point_terms(family, s, y[:, None], with_h=False)
    lf = log_factorial(y)[:, None] if family == "poisson" else np.zeros((X.shape[0], 1), dtype=LD)
    return dict(family=family, Th=Th, X=X, y=y, s=s, ll=ll, g=g, lf=lf)


def log_joint_grad(family, Z, w, Th, with_bounds=False, table=None):
    """The weighted log joint  sum_j w_j log p(z_j | theta) - |theta|^2 / 2 - D/2 log 2 pi  (the Poisson -log y! kept) and its
    theta-gradient at the C rows of Th: (values (C), gradients (C x D)), long double.  Z: rows y x (logistic) or [x, y]
    (Poisson); w None: ones.  ``table``: point_table(family, Z, Th), where it is at hand.

    with_bounds: also (bv (C), bg (C x D)), the rounding allowance of a float64 evaluation that adds its n = N + D + 1 terms in
    any order from point terms good to 16 U in their scales:
        16 U sum_j |w_j| scale_j (|x_jd|)  +  4 n U (sum of the absolute addends)."""
    tb = point_table(family, Z, Th) if table is None else table
    Th, X, ll, g, lf = tb["Th"], tb["X"], tb["ll"], tb["g"], tb["lf"]
    N, D = X.shape
    w = np.ones(N, dtype=LD) if w is None else _ld(w)
    prior = (Th * Th).sum(axis=1) / 2 + D * LOG_2PI / 2
    val = (w[:, None] * (ll - lf)).sum(axis=0) - prior
    grad = (w[:, None] * g).T.dot(X) - Th
    if not with_bounds:
        return val, grad
    if "sl" not in tb:
        tb["sl"], tb["sg"], _ = scales(family, tb["s"], tb["y"][:, None])
    aw, aX, n = np.abs(w)[:, None], np.abs(X), N + D + 1
    bv = 16 * U * (aw * tb["sl"]).sum(axis=0) + 4 * n * U * ((aw * (np.abs(ll) + np.abs(lf))).sum(axis=0) + prior)
    bg = 16 * U * (aw * tb["sg"]).T.dot(aX) + 4 * n * U * ((aw * np.abs(g)).T.dot(aX) + np.abs(Th))
    return val, grad, bv, bg


def newton_matrix(family, Z, w, th):
    """I - sum_j w_j h_j x_j x_j^T at th (D x D, long double): the matrix csrc/laplace.hip factors."""
    th = _ld(th)
    X, y = _split(family, Z, th.shape[0])
    h = point_terms(family, X.dot(th), y)[2]
    return np.eye(th.shape[0], dtype=LD) - (X * (_ld(w) * h)[:, None]).T.dot(X)


def _solve(A, b):
    """A^-1 b by Gaussian elimination with partial pivoting in long double (LAPACK has no long double)."""
    A, b = A.copy(), b.copy()
    n = b.shape[0]
    for i in range(n):
        p = i + int(np.argmax(np.abs(A[i:, i])))
        if p != i:
            A[[i, p]], b[[i, p]] = A[[p, i]], b[[p, i]]
        for r in range(i + 1, n):
            f = A[r, i] / A[i, i]
            A[r, i:] -= f * A[i, i:]
            b[r] -= f * b[i]
    x = np.zeros(n, dtype=LD)
    for i in range(n - 1, -1, -1):
        x[i] = (b[i] - A[i, i + 1:].dot(x[i + 1:])) / A[i, i]
    return x


def inverse(A):
    n = A.shape[0]
    return np.stack([_solve(A, np.eye(n, dtype=LD)[i]) for i in range(n)], axis=1)


def objective(family, Z, w, th):
    """sum_j w_j ll_j - |th|^2 / 2: the log joint without its constants in th, as the Newton iteration compares it."""
    th = _ld(th)
    X, y = _split(family, Z, th.shape[0])
    return (_ld(w) * point_terms(family, X.dot(th), y, with_h=False)[0]).sum() - th.dot(th) / 2


def newton_step(family, Z, w, th):
    """(gradient, Newton matrix, full step) at th."""
    th = _ld(th)
    X, y = _split(family, Z, th.shape[0])
    _, g, h = point_terms(family, X.dot(th), y)
    w = _ld(w)
    grad = (w * g).dot(X) - th
    H = np.eye(th.shape[0], dtype=LD) - (X * (w * h)[:, None]).T.dot(X)
    return grad, H, _solve(H, grad)


def laplace_fit(family, Z, w, th0, tol=1e-10, max_iter=200):
    """Damped Newton from th0 as csrc/laplace.hip states it -- the full step, halved while the objective decreases (to 1e-10 of
    the step at the most), until |step| < tol -- in long double.  Weights below zero count as zero.  Returns (mode, Newton
    matrix at the mode, Newton steps taken, converged)."""
    w = np.maximum(_ld(w), 0)
    th = _ld(th0).copy()
    f = objective(family, Z, w, th)
    for it in range(1, max_iter + 1):
        _, _, step = newton_step(family, Z, w, th)
        t = LD(1)
        while True:
            cand = th + t * step
            fc = objective(family, Z, w, cand)
            if fc >= f or t < 1e-10:
                break
            t = t / 2
        th, f = cand, fc
        if np.abs(step).max() * t < tol:
            return th, newton_matrix(family, Z, w, th), it, True
    return th, newton_matrix(family, Z, w, th), max_iter, False
