"""Device-resident sampler of the weighted posterior of the Gaussian-mean model -- the ``sampler`` argument of
``DeviceProjector("gaussian", ...)`` for the reference's Gaussian experiment (examples/gaussian/main.py:107-112 with
examples/common/model_gaussian.py:23-30: prior theta ~ N(mu0, Sig0), observations x ~ N(theta, Sig), rows z = x):

    Sigma_w^-1 = Sig0^-1 + (sum w) Sig^-1,      mu_w = Sigma_w (Sig0^-1 mu0 + Sig^-1 sum_i w_i p_i)

The precision depends on the weights only through their sum.  With Sig^-1 = L L^T and L^-1 Sig0^-1 L^-T = V diag(lam) V^T, both
formed here once, Sigma_w = W diag(1 / (lam + sum w)) W^T with W = L^-T V: a call is two reductions over the points and a
few D x D products on the device (csrc/gauss.hip), theta = mu_w + (R * (lam + sum w)^-1/2) W^T -- no factorisation per call.
(Any factor of Sigma_w serves; this one is not the reference's triangular one, so the same normal numbers give other draws of
the same distribution.)

* ``sampler(n, wts, pts)``: the reference's sampler signature -- uploads the k weights and points, returns the draws as a device
  tensor (``DeviceProjector`` uses them in place); ``sampler.mean`` is then the mean of the draws (a device vector);
* ``sampler.enqueue_plan(n, pts, steps)``: for ``SparseVICoreset``'s device-resident weight optimisation -- the plan's
  ``draw(w_dev, i)`` takes the weights FROM the device and enqueues the kernels: no host synchronisation per ADAM step.

A precision that is not positive (weights summing to -min(lam) or less, NaN weights) raises ``EngineError``: at once from the
call form, from ``check()`` after an enqueued loop.  There is no CPU fallback."""
import numpy as np

from .linreg_sampler import _DeviceNormals, _MovingPoints


class GaussianPosteriorSampler(_DeviceNormals):
    DMAX = 1024    # coordinates (csrc/gauss.hip GPS_MAX_DIM)
    KMAX = 4096    # weighted points
    SMAX = 4096    # draws per call (DeviceProjector's own limit on the projection dimension)
    NOISE_BUDGET = 2 << 30      # bytes of pre-drawn normal numbers an enqueue plan may hold

    def __init__(self, mu0, Sig0inv, Siginv, device="cuda", seed=None):
        import torch
        from . import _native
        self._torch, self._nat = torch, _native
        self._lib = _native.load()
        if not torch.cuda.is_available():
            raise RuntimeError("GaussianPosteriorSampler needs a GPU (there is no CPU fallback)")
        self.device = torch.device(device)
        self.mu0 = np.ascontiguousarray(mu0, dtype=np.float64)
        self.Sig0inv = np.ascontiguousarray(Sig0inv, dtype=np.float64)
        self.Siginv = np.ascontiguousarray(Siginv, dtype=np.float64)
        D = self.D = self.mu0.shape[0]
        if D < 1 or D > self.DMAX:
            raise ValueError("GaussianPosteriorSampler: 1 <= D <= %d" % self.DMAX)
        if self.Sig0inv.shape != (D, D) or self.Siginv.shape != (D, D):
            raise ValueError("Sig0inv and Siginv must be %d x %d" % (D, D))
        self.ld = D + (D % 2)                               # rows of the draws start on 16-byte boundaries
        L = np.linalg.cholesky(self.Siginv)
        Li = np.linalg.solve(L, np.eye(D))
        A = Li.dot(self.Sig0inv).dot(Li.T)
        self.lam, V = np.linalg.eigh(0.5 * (A + A.T))
        self.W = Li.T.dot(V)                                # Sigma_w = W diag(1 / (lam + sum w)) W^T
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(self.device)
        self._W, self._WT, self._lam = up(self.W), up(self.W.T), up(self.lam)
        self._c0 = up(self.Sig0inv.dot(self.mu0))
        self._Sig = None if np.array_equal(self.Siginv, np.eye(D)) else up(self.Siginv)
        self._seed, self._offset = (0 if seed is None else int(seed)) & 0xFFFFFFFFFFFFFFFF, 0
        self._theta, self._tbar = {}, torch.empty(D, dtype=torch.float64, device=self.device)
        self._state = torch.empty(2 * D, dtype=torch.float64, device=self.device)
        self._status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.mean = self._tbar

    def supports(self, n, k):
        return 0 <= k <= self.KMAX and 1 <= n <= self.SMAX

    def _theta_buf(self, n):
        t = self._theta.get(n)
        if t is None:
            t = self._theta[n] = self._torch.zeros(n, self.ld, dtype=self._torch.float64, device=self.device)
        return t

    def _points(self, pts):
        pts = np.atleast_2d(np.asarray(pts, dtype=np.float64))
        if pts.shape[1] != self.D:
            raise ValueError("points have %d columns, the model has %d coordinates" % (pts.shape[1], self.D))
        return self._torch.from_numpy(np.ascontiguousarray(pts)).to(self.device)

    def _args(self, k, w_dev, p_dev, theta):
        """Argument list of bcx_gaussian_posterior_draw; slots 11 / 12 take the normal numbers and their column means."""
        return [self._nat.stream_ptr(self.device), k, self.D, w_dev.data_ptr() if k else None, p_dev.data_ptr() if k else None, p_dev.stride(0) if k else 0,
                self._c0.data_ptr(), None if self._Sig is None else self._Sig.data_ptr(), self._W.data_ptr(), self._WT.data_ptr(),
                self._lam.data_ptr(), 0, 0, theta.shape[0], self.ld, theta.data_ptr(), self._tbar.data_ptr(), self._state.data_ptr(),
                self._status.data_ptr()]

    def _run(self, a):
        self._nat.check(self._lib.bcx_gaussian_posterior_draw(*a))

    def clear_status(self):
        self._status.zero_()

    def status(self):
        """Synchronises; raises if any call since ``clear_status`` met a precision lam + sum w that was not positive."""
        if int(self._status.item()) != 0:
            self.clear_status()
            raise self._nat.EngineError(self._nat.ERR_STATE, "GaussianPosteriorSampler: the weighted posterior's precision is not "
                                        "positive definite (weights summing to -min(lam) or less, or weights that are not finite)")

    # -- the reference's sampler signature --------------------------------------------------------------------------------------
    def __call__(self, n, wts, pts):
        torch = self._torch
        k = 0 if wts is None or pts is None else len(wts)
        if k and np.asarray(pts).size == 0:
            k = 0
        if not self.supports(n, k):
            raise ValueError("GaussianPosteriorSampler: %d draws for %d weighted points (at most %d and %d)" % (n, k, self.SMAX, self.KMAX))
        w_dev = p_dev = None
        if k:
            p_dev = self._points(pts)
            if p_dev.shape[0] != k:
                raise ValueError("%d weights for %d points" % (k, p_dev.shape[0]))
            w_dev = torch.from_numpy(np.ascontiguousarray(wts, dtype=np.float64)).to(self.device)
        theta = self._theta_buf(n)
        R = self._noise(n)
        a = self._args(k, w_dev, p_dev, theta)
        rbar = self._column_means(R)
        a[11], a[12] = R.data_ptr(), rbar.data_ptr()
        self.clear_status()
        self._run(a)
        self.status()
        self.mean = self._tbar
        return theta[:, :self.D]

    # -- SparseVI's device-resident weight optimisation ------------------------------------------------------------------------
    def enqueue_plan(self, n, pts, steps):
        """None when this sampler cannot serve the loop from the device (too many points / draws)."""
        pts = np.atleast_2d(np.asarray(pts, dtype=np.float64))
        if pts.shape[0] < 1 or not self.supports(n, pts.shape[0]):
            return None
        if steps * (n + 1) * self.ld * 8 > self.NOISE_BUDGET:
            return None                                     # (the caller's host loop draws step by step)
        return _Plan(self, n, self._points(pts), self._noise_block(steps, n))

    def enqueue_plan_moving(self, n, k, d, steps):
        """A plan for ``steps`` draws at k points that live on the device and are REWRITTEN IN PLACE between the draws
        (``BatchPSVICoreset``'s enqueued loop; ``plan.points``: the k x d view to write them to); None when it cannot be served."""
        if d != self.D or k < 1 or not self.supports(n, k) or steps * (n + 1) * self.ld * 8 > self.NOISE_BUDGET:
            return None
        return _MovingPlan(self, n, k, self._noise_block(steps, n))


class _Plan(object):
    """The draws of ``steps`` consecutive sampler calls at the same points, from weights that live on the device; the normal
    numbers of all steps are drawn up front."""

    def __init__(self, sampler, n, p_dev, noise):
        self.s, self.n, self.p_dev = sampler, n, p_dev
        self.theta = sampler._theta_buf(n)
        sampler.clear_status()                              # (check() then covers every step of this plan)
        self.set_noise(noise)

    def set_noise(self, noise):
        self.noise, self._a = noise, None
        self.rbar = self.s._column_means(noise)             # steps x ld

    def buffers(self):
        """(draws S x D, their mean): the same two device buffers at every step, rewritten in stream order."""
        return self.theta[:, :self.s.D], self.s._tbar

    def draw(self, w_dev, i):
        a = self._a
        if a is None or self._w_ptr != w_dev.data_ptr():
            a = self._a = self.s._args(self.p_dev.shape[0], w_dev, self.p_dev, self.theta)
            self._w_ptr = w_dev.data_ptr()
            self._r0, self._rstep = self.noise.data_ptr(), self.noise.stride(0) * 8
            self._b0, self._bstep = self.rbar.data_ptr(), self.rbar.stride(0) * 8
        a[11], a[12] = self._r0 + i * self._rstep, self._b0 + i * self._bstep
        self.s._run(a)
        return self.buffers()

    def check(self):
        """After the loop's read-back: was the precision positive definite at every step?  Raises ``EngineError`` otherwise."""
        self.s.status()


class _MovingPlan(_MovingPoints, _Plan):
    """``_Plan`` over a point buffer of its own that others rewrite (the draw kernel reads the points at every call)."""

    def __init__(self, sampler, n, k, noise):
        self._alloc_points(sampler._torch, sampler.device, k, sampler.D)
        _Plan.__init__(self, sampler, n, self.points, noise)
