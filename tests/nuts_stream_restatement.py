"""The NUTS transition of tests/nuts_restatement.py in RESUMABLE form: the statement the consume phase of
csrc/nuts_stream.hip is written from.  The streamed kernel cannot run a transition as a loop around the target:
one pass over the rows evaluates ONE leaf of every chain, so a chain is a record that is moved one evaluation forward at a time.

    chain = Chain(target, noise, n_warmup, J, eps0, fixed_eps)
    theta = chain.begin()                      # the start state xi = 0
    while theta is not None:
        theta = chain.consume(*evaluate(target, theta))     # (sum_j w_j log p_j, sum_j w_j g_j x_j) at theta: what a pass leaves

The record is exactly the kernel's: xi, the moving end's xi (xp) and momentum p, the carried log p, xi-gradient and theta; the
tree (both endpoints with momentum and gradient, the moving end's gradient, the doubling's proposal with gradient and theta, the
checkpoints); the integers t, j, i, nleaf, depth (and the phase, the divergence flag); the scalars H0, logW, logS, asum, dsel,
the base step, Hbar, log eps-bar, the accept sum (and the proposal's log p and energy).  `consume` finishes the leaf whose theta
it handed out -- second half kick, energy, accept statistic, divergence, leaf selection, checkpoint or span tests; where the leaf
closes a doubling the tree-level selection, the endpoint replacement and the tree's turn test; where that ends the transition
the outputs (appended to `chain.out`), the dual averaging and the set-up of the next transition -- and then takes the first half
kick and drift of the next leaf.  Works in the dtype of the target, with the operations of transition_iterative in its order:
tests/test_nuts_stream_host.py holds the two to the same bits."""
import numpy as np

import nuts_restatement as nr
from hmc_restatement import point_terms


def evaluate(target, theta):
    """What one pass leaves for a chain at theta: (sum_j w_j log p_j, sum_j w_j g_j x_j)."""
    ll, g = point_terms(target.family, target.X.dot(theta), target.y)
    return (target.w * ll).sum(), (target.w * g).dot(target.X)


class Chain(object):
    def __init__(self, target, noise, n_warmup, J, eps0, fixed_eps=None):
        dt, D = target.dt, target.D
        self.tg, self.noise, self.nwarm, self.J, self.eps0, self.adapt = target, np.asarray(noise).astype(dt), n_warmup, J, eps0, fixed_eps is None
        self.T = self.noise.shape[0]
        z = np.zeros(D, dtype=dt)
        self.xi, self.xp, self.p, self.gcur, self.thcur, self.th = z, z, z, z, z, z
        self.xl = self.pl = self.gl = self.xr = self.pr = self.gr = self.gm = self.xs = self.gs = self.ths = z
        self.ckx, self.ckp = [None] * max(J, 1), [None] * max(J, 1)
        self.ph = self.t = self.j = self.i = self.nleaf = self.depth = 0
        self.divergent = False
        self.logp_cur = self.H0 = self.logW = self.logS = self.asum = self.dsel = self.hbar = self.lebar = self.acc_sum = dt(0)
        self.logp_s = self.h_s = dt(0)
        self.base = dt(eps0 if fixed_eps is None else fixed_eps)
        self.out, self.rounds, self.nonfinite, self.accept_rate = [], 0, False, None

    def begin(self):
        self.th = self.tg.theta(self.xp)
        return self.th

    def _direction(self):
        z, D = self.noise[self.t], self.tg.D
        return z, (1 if z[D + 3 * self.j] >= 0 else -1)

    def consume(self, value, wgx):
        """One evaluation at the theta handed out last: the chain moves one leaf on.  Returns the next theta, or None after the
        last transition."""
        tg, dt, D, J = self.tg, self.tg.dt, self.tg.D, self.J
        self.rounds += 1
        logp = value - self.th.dot(self.th) / 2               # the prior
        gx = tg.W.dot(wgx - self.th)                           # g_xi = W g_theta
        start = False
        if self.ph == 0:
            self.gcur, self.thcur, self.logp_cur = gx, self.th, logp
            self.ph, start = 1, True
        else:
            z, v = self._direction()
            eps = self.base
            half = v * (eps / 2)
            self.gm = gx
            self.p = self.p + half * gx
            H = self.p.dot(self.p) / 2 - logp
            delta = self.H0 - H
            fin = bool(np.isfinite(delta))
            with np.errstate(over="ignore"):
                self.asum = self.asum + (min(dt(1), np.exp(delta)) if fin else dt(0))
            self.nleaf += 1
            ok, i, j = True, self.i, self.j
            if not (fin and delta > nr.DIVERGENT):
                self.divergent, self.nonfinite, ok = True, self.nonfinite or not fin, False
            else:
                if i == 0:
                    self.logS, take = delta, True
                else:
                    self.logS = nr._logaddexp(self.logS, delta)
                    take = bool(self.logS - delta <= nr._threshold(z, D + 3 * J + 2 * ((1 << j) - 1 + i)))
                if take:
                    self.xs, self.gs, self.ths, self.logp_s, self.h_s = self.xp, self.gm, self.th, logp, H
                if i & 1:
                    m = 1
                    while m <= j and (i >> (m - 1)) & 1:       # one span per trailing one bit of i
                        slot = bin(i - (1 << m) + 1).count("1")
                        d = v * (self.xp - self.ckx[slot])
                        if d.dot(self.ckp[slot]) < 0 or d.dot(self.p) < 0:
                            ok = False
                            break
                        m += 1
                else:
                    slot = bin(i).count("1")
                    self.ckx[slot], self.ckp[slot] = self.xp, self.p
            done = not ok
            if ok:
                if i + 1 < (1 << j):
                    self.i += 1
                else:
                    if self.logW - self.logS <= nr._threshold(z, D + 3 * j + 1):
                        self.xi, self.gcur, self.thcur, self.logp_cur = self.xs, self.gs, self.ths, self.logp_s
                        self.dsel = self.h_s - self.H0
                    self.logW = nr._logaddexp(self.logW, self.logS)
                    if v > 0:
                        self.xr, self.pr, self.gr = self.xp, self.p, self.gm
                    else:
                        self.xl, self.pl, self.gl = self.xp, self.p, self.gm
                    self.depth = j + 1
                    d = self.xr - self.xl
                    if d.dot(self.pl) < 0 or d.dot(self.pr) < 0 or j + 1 >= J:
                        done = True
                    else:
                        self.j, self.i, self.logS, self.logp_s, self.h_s = j + 1, 0, dt(0), dt(0), dt(0)
            if done:
                t = self.t
                alpha = self.asum / self.nleaf
                if self.adapt and t < self.nwarm:
                    self.base, self.hbar, self.lebar = nr.dual_average_alpha(t + 1, alpha, self.hbar, self.lebar, self.eps0, t + 1 == self.nwarm, dt)
                if t >= self.nwarm or self.nwarm >= self.T:
                    self.acc_sum = self.acc_sum + alpha
                self.out.append(dict(state=self.xi, theta=self.thcur, logp=self.logp_cur, grad=self.gcur, depth=self.depth, n_leapfrog=self.nleaf,
                                     alpha=alpha, divergent=self.divergent, dsel=self.dsel, base=self.base, hbar=self.hbar, lebar=self.lebar))
                self.t = t + 1
                start = self.t < self.T
                if not start:
                    self.ph = 2
                    self.accept_rate = self.acc_sum / (self.T if self.nwarm >= self.T else self.T - self.nwarm)
        if start:
            z = self.noise[self.t]
            p0 = z[:D].copy()
            self.H0 = p0.dot(p0) / 2 - self.logp_cur
            self.xl, self.pl, self.gl = self.xi, p0, self.gcur
            self.xr, self.pr, self.gr = self.xi, p0, self.gcur
            self.logW = self.asum = self.dsel = self.logS = self.logp_s = self.h_s = dt(0)
            self.nleaf = self.depth = self.j = self.i = 0
            self.divergent = False
        if self.ph != 1:
            return None
        z, v = self._direction()
        if self.i == 0:
            self.xp, self.p, self.gm = (self.xr, self.pr, self.gr) if v > 0 else (self.xl, self.pl, self.gl)
        half = v * (self.base / 2)
        ph = self.p + half * self.gm
        self.p = ph
        self.xp = self.xp + (v * self.base) * ph
        self.th = tg.theta(self.xp)
        return self.th


def run_chain(target, noise, n_warmup, J, eps0, fixed_eps=None):
    """The chain to its end: (the per-transition records, the evaluations it took = the rounds of a launch it would end)."""
    chain = Chain(target, noise, n_warmup, J, eps0, fixed_eps)
    theta = chain.begin()
    while theta is not None:
        theta = chain.consume(*evaluate(target, theta))
    return chain
