"""A NumPy statement of the windowed metric adaptation of bc.DeviceHMC(kernel="nuts", adapt_metric=...) (csrc/nuts_adapt.h,
DESIGN.md 4.17), for the tests, on top of the recursive transition of tests/nuts_restatement.py.  It works in the dtype it is
given (float64, or np.longdouble as the more precise referee) and has its own Cholesky loop (np.linalg has no long double).

    W0: the frame passed; xi0: the chain's coordinate in it; L: lower triangular, I at the start; eta: the coordinate the chain
    moves in, xi0 = L eta, theta = mu + (L^T W0)^T eta -- a metric M^-1 = L L^T in xi0 is a unit metric in eta.
    schedule(n_warmup): none below 20; init, term, base = 75, 50, 25, or floor(.15 n), floor(.1 n), the rest when those exceed n;
      windows from s = init of length w = base: e = s + w, or n - term if e + 2 w > n - term; s = e, w = 2 w while s < n - term.
    after every transition t of a window [s, e): x = L eta joins Welford's mean and sum of outer products
      (d = x - mean; mean += d / n; M2 += d (x - mean)^T).
    after transition e - 1, n = e - s: S = M2 / (n - 1) (its diagonal alone: "diag"); Sigma = n / (n + 5) S + 1e-3 * 5 / (n + 5) I;
      L = chol(Sigma); eta = L^-1 x; the frame L^T W0; the target evaluated at the state; the accumulators cleared; the dual
      averaging restarted: counter 0, Hbar = log eps-bar = 0, eps0 = the step the ended segment averaged to.
    the dual averaging runs in segments that end where a window ends and at n_warmup; the last transition of each hands on
      exp(log eps-bar)."""
import numpy as np

import nuts_restatement as nr

REG, REG_N = 1e-3, 5


def schedule(n_warmup):
    n = int(n_warmup)
    if n < 20:
        return []
    init, term, base = 75, 50, 25
    if init + term + base > n:
        init, term = (15 * n) // 100, n // 10
        base = n - init - term
    out, s, w = [], init, base
    while s < n - term:
        e = s + w
        if e + 2 * w > n - term:
            e = n - term
        out.append((s, e))
        s, w = e, 2 * w
    return out


def scaled_logistic_case():
    """The badly scaled target of DESIGN.md 4.17: logistic, k = 60, D = 3, feature columns scaled by (1, 6, 30).  Returns the
    rows y x, the weights and the generator (for what a test draws next)."""
    rng = np.random.default_rng(5)
    X = rng.standard_normal((60, 3)) * np.array([1.0, 6.0, 30.0])
    theta = np.array([0.5, -0.1, 0.02])
    y = np.where(rng.random(60) < 1 / (1 + np.exp(-X.dot(theta))), 1.0, -1.0)
    w = rng.random(60) * 3 + 0.5
    return y[:, None] * X, w, rng


def segments(n_warmup):
    """The dual-averaging segments [start, end) of the warm-up."""
    ends = [e for _, e in schedule(n_warmup)]
    if not ends or ends[-1] < n_warmup:
        ends.append(n_warmup)
    return list(zip([0] + ends[:-1], ends))


def cholesky(A, dt):
    """Lower triangular L with L L^T = A by the row loop, in dt; None when a pivot is not positive and finite."""
    D = A.shape[0]
    L = np.zeros((D, D), dtype=dt)
    for i in range(D):
        for j in range(i + 1):
            v = A[i, j] - L[i, :j].dot(L[j, :j])
            if i == j:
                if not (v > 0 and np.isfinite(v)):
                    return None
                L[i, i] = np.sqrt(v)
            else:
                L[i, j] = v / L[j, j]
    return L


def solve_lower(L, b):
    x = np.zeros_like(b)
    for i in range(len(b)):
        x[i] = (b[i] - L[i, :i].dot(x[:i])) / L[i, i]
    return x


class Welford(object):
    def __init__(self, D, dt):
        self.n, self.mean, self.M2, self.dt = 0, np.zeros(D, dtype=dt), np.zeros((D, D), dtype=dt), dt

    def add(self, x):
        self.n += 1
        d = x - self.mean
        self.mean = self.mean + d / self.dt(self.n)
        self.M2 = self.M2 + np.outer(d, x - self.mean)

    def factor(self, metric):
        """chol of the regularised sample covariance of the draws so far (its diagonal alone: "diag"); None: keep the frame."""
        dt, n, D = self.dt, self.dt(self.n), len(self.mean)
        S = np.tril(self.M2) / (n - 1)
        S = S + np.tril(S, -1).T
        if metric == "diag":
            S = np.diag(np.diag(S))
        Sigma = n / (n + REG_N) * S + dt(REG) * (REG_N / (n + REG_N)) * np.eye(D, dtype=dt)
        return cholesky(Sigma, dt)


def window_end(draws, metric, dt):
    """From a window's draws in xi0 (n x D): (the new L or None, eta of the last draw in it)."""
    draws = np.asarray(draws).astype(dt)
    acc = Welford(draws.shape[1], dt)
    for x in draws:
        acc.add(x)
    L = acc.factor(metric)
    return L, (None if L is None else solve_lower(L, draws[-1]))


def framed_target(family, pts, wts, D, mu, W0, L, dt):
    """The target in eta: the frame L^T W0, formed in dt."""
    W0 = np.eye(D, dtype=dt) if W0 is None else np.asarray(W0).astype(dt)
    return nr.Target(family, pts, wts, D, mu, np.asarray(L).astype(dt).T.dot(W0), dt)


def run_chain(family, pts, wts, D, mu, W0, noise, n_warmup, J, eps0, metric=None, dtype=np.float64):
    """All transitions of one chain from eta = 0 with the metric learned in the windows (metric None: none is, the chain of
    nuts_restatement.run_chain).  A dict of per-transition arrays (theta, eta in the frame current at the transition, depth,
    n_leapfrog, alpha, divergent, margin, base: the step the transition ran with, start: the state it started from, window: the
    windows that had ended before it), `frames` (L after each window), `metric` (the final L) and `step`."""
    dt, T = dtype, noise.shape[0]
    L = np.eye(D, dtype=dt)
    tg = framed_target(family, pts, wts, D, mu, W0, L, dt)
    eta = np.zeros(D, dtype=dt)
    carried = tg.eval(eta)
    wins = schedule(n_warmup) if metric else []
    segs = segments(n_warmup) if metric else [(0, n_warmup)]
    wi = si = 0
    acc = Welford(D, dt)
    base, seg_eps = dt(eps0), dt(eps0)
    hbar = lebar = dt(0)
    out = dict(theta=np.zeros((T, D)), eta=np.zeros((T, D), dtype=dt), depth=np.zeros(T, dtype=int), n_leapfrog=np.zeros(T, dtype=int),
               alpha=np.zeros(T, dtype=dt), divergent=np.zeros(T, dtype=bool), margin=np.zeros(T), base=np.zeros(T, dtype=dt), frames=[],
               start=np.zeros((T, D), dtype=dt), window=np.zeros(T, dtype=int))
    for t in range(T):
        out["start"][t], out["window"][t] = eta, wi
        r = nr.transition_recursive(tg, eta, noise[t], base, J, carried)
        out["base"][t] = base
        eta, carried = r["state"], (r["logp"], r["grad"])
        out["theta"][t], out["eta"][t] = tg.theta(eta), eta
        for q in ("depth", "n_leapfrog", "alpha", "divergent", "margin"):
            out[q][t] = r[q]
        if t < n_warmup:
            s0, s1 = segs[si]
            base, hbar, lebar = nr.dual_average_alpha(t - s0 + 1, r["alpha"], hbar, lebar, seg_eps, t + 1 == s1, dt)
        if wi < len(wins) and t >= wins[wi][0]:
            x = L.dot(eta)
            acc.add(x)
            if t + 1 == wins[wi][1]:
                Ln = acc.factor(metric)
                if Ln is not None:
                    L, eta = Ln, solve_lower(Ln, x)
                    tg = framed_target(family, pts, wts, D, mu, W0, L, dt)
                    carried = tg.eval(eta)
                out["frames"].append(L.copy())
                acc = Welford(D, dt)
                hbar = lebar = dt(0)
                seg_eps = base
                wi, si = wi + 1, si + 1
    out["metric"], out["step"] = L, float(base)
    return out
