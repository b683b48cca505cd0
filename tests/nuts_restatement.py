"""Two NumPy statements of the NUTS transition of csrc/nuts.hip, for the tests: a recursive one in the shape of
Hoffman & Gelman 2014, Alg. 6 (a depth-j tree is two depth-(j-1) trees, the turn test at each level) and an iterative one with
the kernel's checkpoint scheme (the endpoint of even leaf i at slot popcount(i)).  Both take their normal numbers as an array and
work in the dtype of the target (float64, or np.longdouble as the more precise referee).

    theta = mu + W^T xi, unit mass matrix, log target as tests/hmc_restatement.py; J = max_depth
    transition t reads z (D + 3 J + 2 (2^J - 1)):  p0 = z[:D];  doubling j: direction z[D+3j] (>= 0 forward), threshold
    e_j = (z[D+3j+1]^2 + z[D+3j+2]^2) / 2;  leaf i of doubling j, slot s = 2^j - 1 + i: e_leaf = (z[D+3J+2s]^2 + z[D+3J+2s+1]^2) / 2
    H0 = |p0|^2 / 2 - logp(xi);  doubling j: 2^j leapfrog steps of v eps from the right (v = +1) or left (v = -1) endpoint
    leaf: delta = H0 - H_leaf;  alpha sum += min(1, exp delta) (0: not finite);  not (finite and delta > -1000): divergent, stop;
          logS = logaddexp(logS, delta);  the leaf is the subtree's proposal iff logS - delta <= e_leaf (the first always);
          every balanced span a .. b that closes at the leaf: d = v (xi_b - xi_a), a turn iff d.p_a < 0 or d.p_b < 0: stop
    a completed doubling: its proposal replaces the tree's iff logW - logS <= e_j;  logW = logaddexp(logW, logS);
          the tree stops (keeping the proposal) iff (xi_right - xi_left).p_left < 0 or (xi_right - xi_left).p_right < 0
    warm-up: the dual averaging of tests/hmc_restatement.py with alpha = alpha sum / leaves.

The recursive statement reports the smallest margin over every decision it made (the direction |z|, both dot products of every
turn test, |(logS - delta) - e_leaf|, |(logW - logS) - e_j|, |delta + 1000|): a transition whose margin is tiny may legitimately
come out differently in another arithmetic."""
import numpy as np

from hmc_restatement import DELTA, GAMMA, KAPPA, T0, Target, point_terms  # noqa: F401  (re-exported for the tests)

DIVERGENT = -1000.0


def noise_columns(D, J):
    return D + 3 * J + 2 * ((1 << J) - 1)


def dual_average_alpha(m, alpha, hbar, lebar, eps0, last, dtype=np.float64):
    """Warm-up iteration m (1-based) after a transition with accept statistic alpha: (next base step, Hbar, log epsbar)."""
    dt = dtype
    m, alpha, hbar, lebar = dt(m), dt(alpha), dt(hbar), dt(lebar)
    eta = 1 / (m + dt(T0))
    hbar = (1 - eta) * hbar + eta * (dt(DELTA) - alpha)
    loge = np.log(10 * dt(eps0)) - np.sqrt(m) / dt(GAMMA) * hbar
    mk = m ** dt(-KAPPA)
    lebar = mk * loge + (1 - mk) * lebar
    return (np.exp(lebar) if last else np.exp(loge)), hbar, lebar


def _logaddexp(a, b):
    return max(a, b) + np.log1p(np.exp(-abs(a - b)))


def _threshold(z, at):
    return (z[at] * z[at] + z[at + 1] * z[at + 1]) / 2


def _result(prop, H0, depth, asum, n, divergent, nonfinite, margin, xi):
    x, logp, g, H = prop
    return dict(state=x, logp=logp, grad=g, depth=depth, n_leapfrog=n, alpha=asum / n, divergent=divergent, finite=not nonfinite,
                dsel=H - H0, H0=H0, margin=margin, moved=bool(np.any(x != xi)))


# --------------------------------------------------------------------------------------------------------------- recursive
class _Walk(object):
    """What the leaves of one transition share: the accumulators, in leaf order."""

    def __init__(self, target, z, eps, H0, J):
        self.tg, self.z, self.eps, self.H0, self.J, self.D = target, z, eps, H0, J, target.D
        self.asum, self.n, self.divergent, self.nonfinite, self.margin = target.dt(0), 0, False, False, np.inf

    def note(self, *vals):
        for v in vals:
            v = abs(float(v))
            if v == v:
                self.margin = min(self.margin, v)

    def start(self, j, v):
        self.j, self.v, self.i, self.logS, self.prop = j, v, 0, None, None

    def leaf(self, x, p, g):
        """One leapfrog step of v eps from (x, p, g): (ok, the new point)."""
        dt, v = self.tg.dt, self.v
        half = v * (self.eps / 2)
        ph = p + half * g
        xn = x + (v * self.eps) * ph
        logp, gn = self.tg.eval(xn)
        pn = ph + half * gn
        H = pn.dot(pn) / 2 - logp
        delta = self.H0 - H
        fin = bool(np.isfinite(delta))
        with np.errstate(over="ignore"):
            self.asum = self.asum + (min(dt(1), np.exp(delta)) if fin else dt(0))
        self.n += 1
        i, self.i = self.i, self.i + 1
        if fin:
            self.note(delta - dt(DIVERGENT))
        if not (fin and delta > DIVERGENT):
            self.divergent, self.nonfinite = True, self.nonfinite or not fin
            return False, None
        if i == 0:
            self.logS, take = delta, True
        else:
            self.logS = _logaddexp(self.logS, delta)
            e = _threshold(self.z, self.D + 3 * self.J + 2 * ((1 << self.j) - 1 + i))
            take = bool(self.logS - delta <= e)
            self.note((self.logS - delta) - e)
        if take:
            self.prop = (xn, logp, gn, H)
        return True, (xn, pn, gn)

    def tree(self, start, depth):
        """2^depth leaves onward from `start`: (ok, first leaf, last leaf)."""
        if depth == 0:
            ok, pt = self.leaf(*start)
            return ok, pt, pt
        ok, a_first, a_last = self.tree(start, depth - 1)
        if not ok:
            return False, None, None
        ok, _, b_last = self.tree(a_last, depth - 1)
        if not ok:
            return False, None, None
        d = self.v * (b_last[0] - a_first[0])
        da, db = d.dot(a_first[1]), d.dot(b_last[1])
        self.note(da, db)
        if da < 0 or db < 0:
            return False, None, None
        return True, a_first, b_last


def transition_recursive(target, xi, z, eps, J, carried=None):
    """One transition from xi with the normals z and the step eps.  `carried`: (logp, gradient) at xi."""
    dt, D = target.dt, target.D
    xi, z, eps = np.asarray(xi).astype(dt), np.asarray(z).astype(dt), dt(eps)
    logp, g = target.eval(xi) if carried is None else carried
    p0 = z[:D].copy()
    H0 = p0.dot(p0) / 2 - logp
    wk = _Walk(target, z, eps, H0, J)
    left = right = (xi, p0, g)
    prop, logW, depth = (xi, logp, g, H0), dt(0), 0
    for j in range(J):
        zj = z[D + 3 * j]
        v = 1 if zj >= 0 else -1
        wk.note(zj)
        e = _threshold(z, D + 3 * j + 1)
        wk.start(j, v)
        ok, _, last = wk.tree(right if v > 0 else left, j)
        if not ok:
            break
        wk.note((logW - wk.logS) - e)
        if logW - wk.logS <= e:
            prop = wk.prop
        logW = _logaddexp(logW, wk.logS)
        if v > 0:
            right = last
        else:
            left = last
        depth = j + 1
        d = right[0] - left[0]
        da, db = d.dot(left[1]), d.dot(right[1])
        wk.note(da, db)
        if da < 0 or db < 0:
            break
    return _result(prop, H0, depth, wk.asum, wk.n, wk.divergent, wk.nonfinite, wk.margin, xi)


# --------------------------------------------------------------------------------------------------------------- iterative
def transition_iterative(target, xi, z, eps, J, carried=None):
    """The same transition as one loop over the leaves, with the checkpoints of the kernel."""
    dt, D = target.dt, target.D
    xi, z, eps = np.asarray(xi).astype(dt), np.asarray(z).astype(dt), dt(eps)
    logp, g = target.eval(xi) if carried is None else carried
    p0 = z[:D].copy()
    H0 = p0.dot(p0) / 2 - logp
    xl, pl, gl = xi, p0, g
    xr, pr, gr = xi, p0, g
    prop, logW, depth = (xi, logp, g, H0), dt(0), 0
    asum, n, divergent, nonfinite = dt(0), 0, False, False
    ckx, ckp = [None] * max(J, 1), [None] * max(J, 1)
    for j in range(J):
        v = 1 if z[D + 3 * j] >= 0 else -1
        e_j = _threshold(z, D + 3 * j + 1)
        x, p, gm = (xr, pr, gr) if v > 0 else (xl, pl, gl)
        half = v * (eps / 2)
        ok, logS, sub = True, None, None
        for i in range(1 << j):
            ph = p + half * gm
            x = x + (v * eps) * ph
            lp, gm = target.eval(x)
            p = ph + half * gm
            H = p.dot(p) / 2 - lp
            delta = H0 - H
            fin = bool(np.isfinite(delta))
            with np.errstate(over="ignore"):
                asum = asum + (min(dt(1), np.exp(delta)) if fin else dt(0))
            n += 1
            if not (fin and delta > DIVERGENT):
                divergent, nonfinite, ok = True, nonfinite or not fin, False
                break
            if i == 0:
                logS, take = delta, True
            else:
                logS = _logaddexp(logS, delta)
                take = bool(logS - delta <= _threshold(z, D + 3 * J + 2 * ((1 << j) - 1 + i)))
            if take:
                sub = (x, lp, gm, H)
            if i & 1:
                m = 1
                while (i >> (m - 1)) & 1:                       # one span per trailing one bit of i
                    slot = bin(i - (1 << m) + 1).count("1")
                    d = v * (x - ckx[slot])
                    if d.dot(ckp[slot]) < 0 or d.dot(p) < 0:
                        ok = False
                        break
                    m += 1
                if not ok:
                    break
            else:
                slot = bin(i).count("1")
                ckx[slot], ckp[slot] = x, p
        if not ok:
            break
        if logW - logS <= e_j:
            prop = sub
        logW = _logaddexp(logW, logS)
        if v > 0:
            xr, pr, gr = x, p, gm
        else:
            xl, pl, gl = x, p, gm
        depth = j + 1
        d = xr - xl
        if d.dot(pl) < 0 or d.dot(pr) < 0:
            break
    return _result(prop, H0, depth, asum, n, divergent, nonfinite, np.nan, xi)


def run_chain(target, noise, n_warmup, J, eps0, fixed_eps=None, step=transition_recursive):
    """All transitions of one chain from xi = 0: a dict of per-transition arrays (theta, xi, depth, n_leapfrog, alpha, divergent,
    margin, base: the step each transition ran with) and the final step."""
    T, D, dt = noise.shape[0], target.D, target.dt
    xi = np.zeros(D, dtype=dt)
    carried = target.eval(xi)
    base = dt(eps0 if fixed_eps is None else fixed_eps)
    hbar = lebar = dt(0)
    out = dict(theta=np.zeros((T, D)), xi=np.zeros((T, D), dtype=dt), depth=np.zeros(T, dtype=int), n_leapfrog=np.zeros(T, dtype=int),
               alpha=np.zeros(T, dtype=dt), divergent=np.zeros(T, dtype=bool), margin=np.zeros(T), base=np.zeros(T, dtype=dt))
    for t in range(T):
        r = step(target, xi, noise[t], base, J, carried)
        out["base"][t] = base
        xi, carried = r["state"], (r["logp"], r["grad"])
        out["theta"][t], out["xi"][t] = target.theta(xi), xi
        for q in ("depth", "n_leapfrog", "alpha", "divergent", "margin"):
            out[q][t] = r[q]
        if fixed_eps is None and t < n_warmup:
            base, hbar, lebar = dual_average_alpha(t + 1, r["alpha"], hbar, lebar, eps0, t + 1 == n_warmup, dt)
    out["step"] = float(base)
    return out
