"""A NumPy statement of the HMC transition of csrc/hmc.hip, for the tests: the whitened target, the leapfrog integrator with
the jittered step, the Exp(1) accept threshold and the dual averaging of the warm-up.  It takes its normal numbers as an
array and works in the dtype it is given (float64, or np.longdouble as the more precise referee).

    theta = mu + W^T xi;   log target(xi) = sum_j w_j log p(z_j | theta) - |theta|^2 / 2   (constants dropped)
    transition t reads z (D + 3): p = z[:D];  e = (z[D]^2 + z[D+1]^2) / 2;  eps_t = eps exp(0.1 z[D+2])
    p += eps_t/2 g;  L times: xi += eps_t p, g = grad(xi), p += eps_t g (eps_t/2 the last time);  accept iff dH <= e
    warm-up iteration m (Hoffman & Gelman 2014, Alg. 5; delta .8, gamma .05, t0 10, kappa .75, mu = log(10 eps0)):
      Hbar = (1 - 1/(m+t0)) Hbar + (delta - alpha)/(m+t0);  log eps = mu - sqrt(m)/gamma Hbar;
      log epsbar = m^-kappa log eps + (1 - m^-kappa) log epsbar;  the last warm-up iteration hands epsbar to the sampling."""
import numpy as np

DELTA, GAMMA, T0, KAPPA = 0.8, 0.05, 10.0, 0.75


def point_terms(family, s, y):
    """(log-likelihood, its derivative in s) of every point, in the dtype of s (the branches of csrc/lik_point.h)."""
    if family == "logistic":
        arg = -s
        small = np.logical_not(arg >= 100)                     # (NaN goes through exp)
        e = np.exp(np.where(small, arg, 0))
        return np.where(small, -np.log1p(e), -arg), np.where(small, e / (1 + e), 1)
    e = np.exp(-np.abs(s))
    rate = np.maximum(s, 0) + np.log1p(e)
    pos = rate > 0
    safe = np.where(pos, rate, 1)
    lr = np.where(s > -100, np.log(safe), s)
    sig = np.where(s >= 0, 1, e) / (1 + e)
    return y * lr - rate, y * np.where(pos & np.logical_not(s < -300), sig / safe, 1) - sig


class Target(object):
    def __init__(self, family, pts, wts, D, center=None, transform=None, dtype=np.float64):
        self.family, self.D, self.dt = family, D, dtype
        pts = np.zeros((0, D + (family == "poisson"))) if pts is None else np.atleast_2d(np.asarray(pts))
        self.X = pts[:, :D].astype(dtype)
        self.y = pts[:, D].astype(dtype) if family == "poisson" else np.zeros(pts.shape[0], dtype=dtype)
        self.w = np.ones(pts.shape[0], dtype=dtype) if wts is None else np.asarray(wts).astype(dtype)
        self.mu = np.zeros(D, dtype=dtype) if center is None else np.asarray(center).astype(dtype)
        self.W = np.eye(D, dtype=dtype) if transform is None else np.asarray(transform).astype(dtype)

    def theta(self, xi):
        return self.mu + self.W.T.dot(xi)

    def eval(self, xi):
        """(log target, its gradient in xi) at xi."""
        th = self.theta(xi)
        ll, g = point_terms(self.family, self.X.dot(th), self.y)
        logp = (self.w * ll).sum() - th.dot(th) / 2
        return logp, self.W.dot((self.w * g).dot(self.X) - th)


def transition(target, xi, z, eps_base, L):
    """One transition from xi with the normals z and the base step eps_base: a dict with the proposal (xi), dH, the
    threshold e, the jittered step eps_t, accepted, and the new state."""
    dt, D = target.dt, target.D
    xi, z = np.asarray(xi).astype(dt), np.asarray(z).astype(dt)
    eps_t = dt(eps_base) * np.exp(z[D + 2] / 10)
    e = (z[D] * z[D] + z[D + 1] * z[D + 1]) / 2
    logp, g = target.eval(xi)
    p = z[:D].copy()
    H0 = p.dot(p) / 2 - logp
    p = p + eps_t / 2 * g
    x = xi + eps_t * p
    for l in range(1, L + 1):
        lp, g = target.eval(x)
        if l < L:
            p = p + eps_t * g
            x = x + eps_t * p
        else:
            p = p + eps_t / 2 * g
    H1 = p.dot(p) / 2 - lp
    dH = H1 - H0
    fin = bool(np.isfinite(dH))
    acc = fin and bool(dH <= e)
    return dict(proposal=x, dH=dH, H0=H0, H1=H1, e=e, eps_t=eps_t, accepted=acc, finite=fin, state=x if acc else xi)


def dual_average(m, dH, hbar, lebar, eps0, last, dtype=np.float64):
    """Warm-up iteration m (1-based) after a transition with energy error dH: (next base step, Hbar, log epsbar)."""
    dt = dtype
    m, dH, hbar, lebar = dt(m), dt(dH), dt(hbar), dt(lebar)
    alpha = min(dt(1), np.exp(-dH)) if np.isfinite(dH) else dt(0)
    eta = 1 / (m + dt(T0))
    hbar = (1 - eta) * hbar + eta * (dt(DELTA) - alpha)
    loge = np.log(10 * dt(eps0)) - np.sqrt(m) / dt(GAMMA) * hbar
    mk = m ** dt(-KAPPA)
    lebar = mk * loge + (1 - mk) * lebar
    return (np.exp(lebar) if last else np.exp(loge)), hbar, lebar


def run_chain(target, noise, n_warmup, L, eps0, fixed_eps=None):
    """All transitions of one chain from xi = 0: (theta after every transition (T x D), dH (T), accepted (T), final step)."""
    T, D = noise.shape[0], target.D
    xi = np.zeros(D, dtype=target.dt)
    base = target.dt(eps0 if fixed_eps is None else fixed_eps)
    hbar = lebar = target.dt(0)
    thetas, dHs, accs = np.zeros((T, D)), np.zeros(T), np.zeros(T, dtype=bool)
    for t in range(T):
        r = transition(target, xi, noise[t], base, L)
        xi = r["state"]
        thetas[t], dHs[t], accs[t] = target.theta(xi), r["dH"], r["accepted"]
        if fixed_eps is None and t < n_warmup:
            base, hbar, lebar = dual_average(t + 1, r["dH"], hbar, lebar, eps0, t + 1 == n_warmup, target.dt)
    return thetas, dHs, accs, float(base)
