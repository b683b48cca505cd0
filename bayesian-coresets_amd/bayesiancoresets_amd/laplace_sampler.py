"""Device-resident sampler of the Laplace approximation of a WEIGHTED logistic / Poisson regression posterior -- the
``sampler`` argument of ``DeviceProjector("logistic" | "poisson", ...)`` for the reference's logistic / Poisson regression
experiment (examples/logistic_poisson_regression/main.py:15-41 ``get_laplace``, :155-162 ``sampler_w``: standard-normal
prior, mode of the weighted log joint, covariance = inverse negative Hessian there).

As ``bc.LinregPosteriorSampler`` it serves two callers:

* ``sampler(n, wts, pts)``: the reference's sampler signature -- uploads the k weights, returns the draws as a device tensor;
* ``sampler.enqueue_plan(n, pts, steps)``: for ``SparseVICoreset``'s device-resident weight optimisation -- ``draw(w_dev, i)``
  takes the weights FROM the device: no host synchronisation (no SciPy minimisation, no upload) per ADAM step.

One launch of one workgroup per call (csrc/laplace.hip: damped Newton on the points in LDS, the D x D Newton systems by an
in-register Cholesky, then the draws mu + R L^-1); the normal numbers come from the library's counter-based generator.  The
reference finds the mode with SciPy's BFGS to gtol 1e-5; this is Newton to |step| < 1e-10 on the same objective (the
iteration of examples/common/model_lr.py / model_poiss.py ``laplace_fit``, which the tests pin to the reference's outputs).
Limits: D <= 32 parameters, the points within 96 KiB of LDS (``supports``); beyond them ``enqueue_plan`` declines (the host
loop then runs) and the call form raises.  There is no CPU fallback.

``stream=True`` lifts the limit on the points: beyond it the fit is one persistent launch of up to a workgroup per CU that
streams the points from device memory (csrc/laplace_stream.hip: per pass one record of partial sums per workgroup, added in
workgroup order behind a grid barrier; the same iteration, status word and outputs), any k.  ``posterior`` and the call form
then also take the points as a DEVICE tensor (``wts=None``: ones) and read them where they are -- the resident full data set
is fitted without a copy."""
import numpy as np

from .linreg_sampler import _DeviceNormals, _MovingPoints

FAMILIES = {"logistic": 0, "poisson": 1}


class LaplacePosteriorSampler(_DeviceNormals):
    SMAX = 4096        # draws per call (DeviceProjector's own limit on the projection dimension)
    NOISE_BUDGET = 2 << 30

    KMAX_STREAM = (1 << 31) - 1     # rows the streamed form takes (a 32-bit count in the ABI)

    def __init__(self, family, D, device="cuda", seed=None, tol=1e-10, max_iter=100, *, stream=False):
        import torch
        from . import _native
        if family not in FAMILIES:
            raise ValueError("family must be 'logistic' or 'poisson'")
        self._torch, self._nat = torch, _native
        self._lib = _native.load()
        if not torch.cuda.is_available():
            raise RuntimeError("LaplacePosteriorSampler needs a GPU (there is no CPU fallback)")
        self.family, self._fam = family, FAMILIES[family]
        self.device = torch.device(device)
        self.D = int(D)
        self.ld = self.D + (self.D % 2)                     # rows of the draws start on 16-byte boundaries
        self.cols = self.D + (1 if family == "poisson" else 0)      # columns of a point: [x, y] for Poisson, y x for logistic
        self.tol, self.max_iter = float(tol), int(max_iter)
        self._seed, self._offset = (0 if seed is None else int(seed)) & 0xFFFFFFFFFFFFFFFF, 0
        self._mu = torch.zeros(self.D, dtype=torch.float64, device=self.device)       # the last mode (seeds a plan's next step)
        self._tbar = torch.zeros(self.D, dtype=torch.float64, device=self.device)
        self._status = torch.zeros(3, dtype=torch.int32, device=self.device)     # [fit, Newton steps, worst fit since zeroed]
        self._none = torch.zeros(2, dtype=torch.float64, device=self.device)
        self._theta = {}
        self._pts_key, self._pts_dev = None, None
        self.stream = bool(stream)
        self._dev_force_stream = False                      # tests: the streamed form where the LDS form applies too
        self._work = None

    def supports(self, n, k):
        if self.stream:
            return 1 <= n <= self.SMAX and 0 <= int(k) <= self.KMAX_STREAM and 1 <= self.D <= 32
        return 1 <= n <= self.SMAX and bool(self._lib.bcx_laplace_sampler_ok(int(k), self.D))

    def _streams(self, k):
        """Whether k points go through csrc/laplace_stream.hip (only a ``stream=True`` sampler ever does)."""
        return self.stream and (bool(self._dev_force_stream) or not self._lib.bcx_laplace_sampler_ok(int(k), self.D))

    def _stream_work(self, k):
        """A scratch buffer of the streamed form for k points (partial records + the barrier's counter)."""
        need = int(self._lib.bcx_laplace_stream_scratch_bytes(int(k), self.D))
        if need < 0:
            raise ValueError("LaplacePosteriorSampler: no streamed fit for %d points of %d parameters" % (k, self.D))
        return self._torch.zeros((need + 7) // 8, dtype=self._torch.float64, device=self.device)

    def _theta_buf(self, n):
        t = self._theta.get(n)
        if t is None:
            t = self._theta[n] = self._torch.zeros(n, self.ld, dtype=self._torch.float64, device=self.device)
        return t

    def _points(self, pts):
        pts = np.atleast_2d(np.asarray(pts, dtype=np.float64))
        if pts.shape[1] != self.cols:
            raise ValueError("points have %d columns, the %s model takes %d" % (pts.shape[1], self.family, self.cols))
        if self._pts_key is None or self._pts_key.shape != pts.shape or not np.array_equal(self._pts_key, pts):
            self._pts_key = pts.copy()
            self._pts_dev = self._torch.from_numpy(np.ascontiguousarray(pts)).to(self.device)
        return self._pts_dev

    def _device_points(self, pts):
        """A device tensor of points as the kernels read it: fp64 rows of ``cols`` values with unit column stride, used in place
        (its row stride may exceed ``cols``: a view of wider rows)."""
        torch = self._torch
        if pts.dim() != 2 or pts.shape[1] != self.cols:
            raise ValueError("points are %s, the %s model takes rows of %d columns" % (tuple(pts.shape), self.family, self.cols))
        if pts.dtype != torch.float64 or pts.device != self._mu.device or (pts.shape[0] > 1 and pts.stride(0) < self.cols) or \
                (pts.shape[1] > 1 and pts.stride(1) != 1):
            pts = pts.to(device=self.device, dtype=torch.float64).contiguous()
        return pts

    def _args(self, k, w_dev, pts_dev, warm, R, rbar, theta, work=None):
        """Argument list of bcx_laplace_sampler, or -- with a scratch buffer -- of bcx_laplace_sampler_stream (``_fn``)."""
        a = [self._nat.stream_ptr(self.device), self._fam, k, self.D, w_dev.data_ptr() if k else None, pts_dev.data_ptr() if k else None, self.cols,
             self._mu.data_ptr(), int(warm), self.tol, self.max_iter, R.data_ptr(), rbar.data_ptr(), theta.shape[0], self.ld,
             theta.data_ptr(), self._tbar.data_ptr(), self._status.data_ptr()]
        if k:
            a[6] = max(a[6], pts_dev.stride(0))             # (the row stride: the points may be a view of padded rows)
        if work is not None:
            a += [work.data_ptr(), work.numel() * 8]
        return a

    def _fn(self, work):
        return self._lib.bcx_laplace_sampler if work is None else self._lib.bcx_laplace_sampler_stream

    def check(self, worst=False):
        """Synchronises; raises if the last fit (``worst``: any fit since the word was zeroed -- a plan zeroes it when it starts)
        did not converge or met no positive definite Newton matrix (NaN weights included: where the reference would go on with
        NaN draws, this is an error)."""
        st = self._status.cpu().numpy()
        v = st[2] if worst else st[0]
        if v != 0:
            if v == 3:
                raise self._nat.EngineError(self._nat.ERR_TIMEOUT, "Laplace fit on the device: a wait between the workgroups of the "
                                            "streamed fit expired%s" % (" at a step of the loop" if worst else ""))
            raise self._nat.EngineError(self._nat.ERR_STATE, "Laplace fit on the device: %s%s"
                                        % ("iteration limit" if v == 1 else "no positive definite Newton matrix",
                                           " at a step of the loop" if worst else " after %d Newton steps" % int(st[1])))
        return int(st[1])

    # -- the reference's sampler signature --------------------------------------------------------------------------------------
    def __call__(self, n, wts, pts):
        torch = self._torch
        on_device = isinstance(pts, torch.Tensor)           # the points where they are (wts None: ones); never brought to the host
        if on_device:
            k = int(pts.shape[0]) if pts.dim() == 2 and pts.numel() else 0
        else:
            k = 0 if wts is None or pts is None else len(wts)
            if k and np.asarray(pts).size == 0:
                k = 0
        if not self.supports(n, k):
            raise ValueError("LaplacePosteriorSampler: %d draws for %d weighted points of %d parameters (D <= 32, the points within "
                             "96 KiB of LDS unless stream=True, at most %d draws)" % (n, k, self.D, self.SMAX))
        pts_dev, w_dev = None, self._none
        if k:
            pts_dev = self._device_points(pts) if on_device else self._points(pts)
            if wts is None:
                w_dev = torch.ones(k, dtype=torch.float64, device=self.device)
            elif isinstance(wts, torch.Tensor):
                w_dev = wts.to(device=self.device, dtype=torch.float64).contiguous()
            else:
                w_dev = torch.from_numpy(np.ascontiguousarray(wts, dtype=np.float64)).to(self.device)
            if w_dev.shape != (k,):
                raise ValueError("LaplacePosteriorSampler: %d weights for %d points" % (w_dev.numel(), k))
        theta = self._theta_buf(n)
        R = self._noise(n)
        work = None
        if self._streams(k):
            if self._work is None or self._work.numel() * 8 < int(self._lib.bcx_laplace_stream_scratch_bytes(k, self.D)):
                self._work = self._stream_work(k)
            work = self._work
        self._nat.check(self._fn(work)(*self._args(k, w_dev, pts_dev, False, R, self._column_means(R), theta, work)))
        self.newton_steps = self.check()
        self.mean = self._tbar
        return theta[:, :self.D]

    def posterior(self, wts, pts):
        """(mode, covariance factor W with Sigma = W^T W) as ndarrays: the rows of W come out as the draws of unit noise.
        ``pts``: an array, or a device tensor that is read in place (then ``wts`` None: ones, or a tensor / array of k weights)."""
        torch = self._torch
        keep = self._noise
        try:
            eye = torch.zeros(self.D + 1, self.ld, dtype=torch.float64, device=self.device)
            eye[:self.D, :self.D] = torch.eye(self.D, dtype=torch.float64, device=self.device)
            self._noise = lambda n: eye
            th = self(self.D + 1, wts, pts).cpu().numpy()
        finally:
            self._noise = keep
        mu = th[self.D]
        return mu, th[:self.D] - mu

    # -- SparseVI's device-resident weight optimisation ------------------------------------------------------------------------
    def enqueue_plan(self, n, pts, steps):
        """None when this sampler cannot serve the loop from the device (too many points / parameters / draws)."""
        pts = np.atleast_2d(np.asarray(pts, dtype=np.float64))
        if pts.shape[0] < 1 or not self.supports(n, pts.shape[0]) or 2 * steps * (n + 1) * self.ld * 8 > self.NOISE_BUDGET:
            return None
        return _LaplacePlan(self, n, self._points(pts), self._noise_block(steps, n))

    def enqueue_plan_moving(self, n, k, d, steps):
        """A plan for ``steps`` draws at k points that live on the device and are REWRITTEN IN PLACE between the draws
        (``BatchPSVICoreset``'s enqueued loop; ``plan.points``: the k x d view to write them to); None when it cannot be served."""
        if d != self.cols or k < 1 or not self.supports(n, k) or 2 * steps * (n + 1) * self.ld * 8 > self.NOISE_BUDGET:
            return None
        return _MovingLaplacePlan(self, n, k, self._noise_block(steps, n))


class _LaplacePlan(object):
    """The draws of ``steps`` consecutive sampler calls at the same points, from weights that live on the device; every step
    after the first starts its Newton iteration at the mode of the step before."""

    def __init__(self, sampler, n, pts_dev, noise):
        self.s, self.n, self.pts_dev = sampler, n, pts_dev
        self.theta = sampler._theta_buf(n)
        # (the streamed form's scratch is the plan's own: its steps are enqueued behind one another on one stream)
        self.work = sampler._stream_work(pts_dev.shape[0]) if sampler._streams(pts_dev.shape[0]) else None
        sampler._status[2].zero_()                          # (check() then covers every fit of this plan)
        self.set_noise(noise)

    def set_noise(self, noise):
        self.noise, self._a = noise, None
        self.rbar = self.s._column_means(noise)

    def buffers(self):
        return self.theta[:, :self.s.D], self.s._tbar

    def draw(self, w_dev, i):
        s = self.s
        a = self._a
        if a is None or self._w_ptr != w_dev.data_ptr():
            a = self._a = s._args(self.pts_dev.shape[0], w_dev, self.pts_dev, False, self.noise, self.rbar, self.theta, self.work)
            self._w_ptr = w_dev.data_ptr()
            self._r0, self._rstep = self.noise.data_ptr(), self.noise.stride(0) * 8
            self._b0, self._bstep = self.rbar.data_ptr(), self.rbar.stride(0) * 8
        a[8] = 1 if i > 0 else 0                            # (warm: the mode of the previous ADAM step)
        a[11], a[12] = self._r0 + i * self._rstep, self._b0 + i * self._bstep
        s._nat.check(s._fn(self.work)(*a))
        return self.buffers()

    def check(self):
        """After the loop's read-back: raises ``EngineError`` if ANY fit of the plan failed (a fit that failed leaves NaNs or
        stale draws behind; a later warm-started fit may still converge)."""
        self.s.check(worst=True)


class _MovingLaplacePlan(_MovingPoints, _LaplacePlan):
    """``_LaplacePlan`` over a point buffer of its own that others rewrite (the kernel stages the points at every call); every
    step after the first still starts at the mode of the step before."""

    def __init__(self, sampler, n, k, noise):
        self._alloc_points(sampler._torch, sampler.device, k, sampler.cols)
        _LaplacePlan.__init__(self, sampler, n, self.points, noise)
