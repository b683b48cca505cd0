"""MCMC on the weighted points: what a Bayesian coreset is built for.  The reference's logistic / Poisson regression
experiment scores every coreset by running Stan on it with ``'w': wts`` (examples/logistic_poisson_regression/main.py:107-127,
205-232; examples/common/mcmc.py:60-70); here the sampler is Hamiltonian Monte Carlo on the device (csrc/hmc.hip, csrc/nuts.hip):

* ``DeviceHMC(family, D, chains, leapfrog, seed).sample(pts, wts, n_samples, ...)``: ``chains`` chains in the whitened variable
  xi (theta = center + transform^T xi, by default the Laplace mode and covariance factor of the same weighted posterior), a fixed
  number of leapfrog steps, the step adapted per chain by dual averaging during the warm-up.  k points that fit the LDS of one
  workgroup run as ONE launch with a workgroup per chain; more (the resident full data set) run as one log-joint pass over the
  rows per leapfrog step for all chains, enqueued without host synchronisation.  The normal numbers come from the library's
  counter-based generator (``_DeviceNormals``): a seed fixes the run.
* ``DeviceHMC(..., kernel="nuts", max_depth=8)``: the same chains with the No-U-Turn transition (csrc/nuts.hip) in
  place of the fixed leapfrog count -- trees of up to ``max_depth`` doublings, no step jitter, dual averaging on the tree's mean
  accept statistic -- for points that fit the LDS of one workgroup, as ONE launch.  ``stream=True`` adds the rows that do not
  (csrc/nuts_stream.hip): one persistent launch of co-resident workgroups, one pass over the rows per leaf for
  all chains still running, at most 256 chains.
* ``DeviceHMC(..., kernel="nuts", adapt_metric="diag" | "dense")``: the LDS-resident NUTS learns a metric per chain in Stan's
  windowed warm-up (csrc/nuts_adapt.h) -- for a frame that is not the Laplace fit of the posterior (``transform=
  np.eye(D)``, features that were not standardised).  The metric is a frame: M^-1 = L L^T in the coordinates of ``transform`` is
  a unit metric in eta with theta = center + (L^T transform)^T eta, re-expressed at the end of every window.
* ``DeviceHMC(..., kernel="nuts").sample_many(problems, n_samples, ...)``: many weighted posteriors of one family and D -- the
  coresets of a size schedule, of several algorithms or trials -- in ONE launch of problems x chains workgroups (csrc/nuts.hip
  nuts_batch_kernel), with or without ``adapt_metric``; every result is bit for bit what ``sample`` returns for
  that problem.  LDS-resident NUTS only: no fixed-length HMC, no streamed rows, one D / depth / transition count per call.
* ``log_joint_grad(family, pts, wts, thetas)``: the weighted log joint and its gradient for many parameter vectors at once
  (model_lr.py:34-39, 59-64; model_poiss.py:40-46, 69-74) -- what the experiment's ``Fs`` metric is made of.

Fixed-length HMC is the default; without ``stream=True`` NUTS runs only on the LDS-resident path (more points than one
workgroup holds raise, use ``kernel="hmc"`` or ``stream=True``), with up to 10 doublings and a noise tensor of chains x transitions x
(D + 3 max_depth + 2 (2^max_depth - 1)) doubles of at most 2 GiB.  Both use a unit mass matrix in xi; only the LDS-resident NUTS
learns one (``adapt_metric``), the streamed NUTS and the fixed-length HMC do not;
logistic and Poisson only (the linreg / Gaussian posteriors are closed-form and sampled exactly by their own samplers), D <= 32,
one device.  There is no CPU fallback."""
import importlib.util
import os
import time

import numpy as np

from .laplace_sampler import FAMILIES, LaplacePosteriorSampler
from .linreg_sampler import _DeviceNormals

DMAX = 32
STREAM_CHAINS_MAX = 256
DIAG = 6
NUTS_DIAG = 8
NUTS_DEPTH_MAX = 10
NUTS_NOISE_BYTES_MAX = 2 << 30
NUTS_METRICS = {"diag": 1, "dense": 2}
NUTS_WINDOWS_MAX = 32


def _example_model(family):
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "common",
                        "model_lr.py" if family == "logistic" else "model_poiss.py")
    if not os.path.exists(path):
        raise ValueError("DeviceHMC: no default center / transform for this many points without the example models (%s); pass "
                         "center= and transform=" % path)
    spec = importlib.util.spec_from_file_location("_bcx_hmc_" + os.path.basename(path)[:-3], path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def split_rhat(x):
    """Split-R-hat per coordinate of x (chains x draws x D): every chain cut into halves (Gelman et al., BDA3 section 11.4)."""
    x = np.asarray(x, dtype=np.float64)
    C, T, D = x.shape
    h = T // 2
    if h < 2:
        return np.full(D, np.nan)
    y = np.concatenate((x[:, :h], x[:, T - h:]), axis=0)
    W = y.var(axis=1, ddof=1).mean(axis=0)
    B = h * y.mean(axis=1).var(axis=0, ddof=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.sqrt(((h - 1.0) / h * W + B / h) / W)


class HMCResult(object):
    """``samples`` (chains, n_samples, D); ``accept_rate`` / ``step_size`` (chains); ``delta_h`` / ``accepted`` (chains,
    n_samples); ``rhat`` (D); ``seconds_per_iteration`` (wall time of the run over warm-up + sampling transitions); ``streamed``
    (the path taken); ``center`` / ``transform``; ``trace`` (``keep_trace=True``: every transition, warm-up included).
    ``kernel="nuts"`` adds ``tree_depth`` / ``n_leapfrog`` / ``divergent`` / ``accept_stat`` (chains, n_samples) and
    ``leapfrog_total`` (chains: the leapfrog steps of all transitions, warm-up included); there
    ``accept_rate`` is the per-chain mean of the accept statistic, ``delta_h`` the selected state's energy minus the start's and
    ``accepted`` whether the state moved.  ``adapt_metric`` ("diag" / "dense") adds ``metric`` (chains, D, D: the final lower
    triangular L, M^-1 = L L^T in the coordinates of ``transform``) and ``metric_windows`` (the warm-up windows, rows start, end);
    ``transform`` stays the frame that was passed, ``step_size`` is the step in the final frame, ``trace["xi"]`` the state in
    the frame current at that transition (``trace["proposal"]`` at a window's last transition: the same state in the new frame)
    and ``trace["frames"]`` (chains, windows, D, D) the L after each window."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _device_rows(torch, device, pts, cols, what):
    if isinstance(pts, torch.Tensor):
        t = pts.to(device=device, dtype=torch.float64)
        if t.dim() != 2 or t.stride(1) != 1:
            t = t.reshape(t.shape[0], -1).contiguous()
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.atleast_2d(np.asarray(pts, dtype=np.float64)))).to(device)
    if t.shape[1] != cols:
        raise ValueError("%s have %d columns, the model takes %d" % (what, t.shape[1], cols))
    return t


def _device_weights(torch, device, wts, n, who):
    """The n weights as a contiguous fp64 device tensor; None (ones) without weights or points."""
    if wts is None or not n:
        return None
    w = wts.to(device=device, dtype=torch.float64).contiguous() if isinstance(wts, torch.Tensor) else \
        torch.from_numpy(np.ascontiguousarray(wts, dtype=np.float64)).to(device)
    if w.shape != (n,):
        raise ValueError("%s: %d weights for %d points" % (who, w.numel(), n))
    return w


def log_joint_grad(family, pts, wts, thetas, device="cuda"):
    """(values (C), gradients (C x D)) of the weighted log joint at the rows of ``thetas`` -- ndarrays, or device tensors when
    ``thetas`` is one.  ``pts``: rows y x (logistic) or [x, y] (Poisson), host array or device tensor; ``wts=None``: ones."""
    import torch
    from . import _native
    if family not in FAMILIES:
        raise ValueError("family must be 'logistic' or 'poisson'")
    if not torch.cuda.is_available():
        raise RuntimeError("log_joint_grad needs a GPU (there is no CPU fallback)")
    lib = _native.load()
    as_tensor = isinstance(thetas, torch.Tensor)
    if isinstance(pts, torch.Tensor) and pts.is_cuda:
        device = pts.device
    device = torch.device(device)
    th = thetas.to(device=device, dtype=torch.float64) if as_tensor else \
        torch.from_numpy(np.ascontiguousarray(np.atleast_2d(np.asarray(thetas, dtype=np.float64)))).to(device)
    th = th.reshape(-1, th.shape[-1]).contiguous()
    C, D = th.shape
    if D < 1 or D > DMAX:
        raise ValueError("log_joint_grad: D = %d parameters (1 <= D <= %d)" % (D, DMAX))
    cols = D + (1 if family == "poisson" else 0)
    N = 0 if pts is None else len(pts)
    Z = _device_rows(torch, device, pts, cols, "points") if N else None
    w = _device_weights(torch, device, wts, N, "log_joint_grad")
    value = torch.empty(C, dtype=torch.float64, device=device)
    grad = torch.empty(C, D, dtype=torch.float64, device=device)
    work = torch.empty(max(int(lib.bcx_log_joint_grad_scratch_bytes(N, D, C)), 8) // 8, dtype=torch.float64, device=device)
    with torch.cuda.device(device):
        _native.check(lib.bcx_log_joint_grad(_native.stream_ptr(device), FAMILIES[family], Z.data_ptr() if N else None, N,
                                             Z.stride(0) if N else cols, D, w.data_ptr() if w is not None else None, th.data_ptr(), C, D,
                                             value.data_ptr(), grad.data_ptr(), work.data_ptr()))
    if as_tensor:
        return value, grad
    return value.cpu().numpy(), grad.cpu().numpy()


class DeviceHMC(_DeviceNormals):
    STEP0 = 0.5        # the step the dual averaging starts from (the whitened target is near N(0, I))

    def __init__(self, family, D, chains=64, leapfrog=8, seed=None, device="cuda", *, device_frame=False, kernel="hmc", max_depth=8,
                 stream=False, adapt_metric=None):
        if family not in FAMILIES:
            raise ValueError("family must be 'logistic' or 'poisson'")
        if not 1 <= int(D) <= DMAX:
            raise ValueError("DeviceHMC: D = %d parameters (1 <= D <= %d)" % (D, DMAX))
        if int(chains) < 1 or int(leapfrog) < 1:
            raise ValueError("DeviceHMC: at least one chain and one leapfrog step")
        if kernel not in ("hmc", "nuts"):
            raise ValueError("DeviceHMC: kernel must be 'hmc' or 'nuts', not %r" % (kernel,))
        if not 1 <= int(max_depth) <= NUTS_DEPTH_MAX:
            raise ValueError("DeviceHMC: max_depth = %d (1 <= max_depth <= %d)" % (max_depth, NUTS_DEPTH_MAX))
        if stream and kernel != "nuts":
            raise ValueError("DeviceHMC: stream=True selects the streamed NUTS (kernel=\"nuts\"); kernel=\"hmc\" streams on its own")
        if adapt_metric is not None:
            if adapt_metric not in NUTS_METRICS:
                raise ValueError("DeviceHMC: adapt_metric must be None, 'diag' or 'dense', not %r" % (adapt_metric,))
            if kernel != "nuts":
                raise ValueError("DeviceHMC: adapt_metric needs kernel=\"nuts\" (the fixed-length HMC learns no metric); drop adapt_metric")
            if stream:
                raise ValueError("DeviceHMC: adapt_metric runs on the LDS-resident NUTS only (the streamed NUTS learns no metric); drop "
                                 "stream=True or adapt_metric")
        import torch
        from . import _native
        self._torch, self._nat = torch, _native
        self._lib = _native.load()
        if not torch.cuda.is_available():
            raise RuntimeError("DeviceHMC needs a GPU (there is no CPU fallback)")
        self.adapt_metric = adapt_metric
        self.family, self._fam = family, FAMILIES[family]
        self.device = torch.device(device)
        self.D, self.chains, self.leapfrog = int(D), int(chains), int(leapfrog)
        self.kernel, self.max_depth = kernel, int(max_depth)
        self.stream = bool(stream)                          # kernel="nuts": rows past one workgroup's LDS take csrc/nuts_stream.hip
        self._scratch = None                                # (its scratch: the sampler's, grown on demand)
        self.ld = self.D + (self.D % 2)
        self.cols = self.D + (1 if family == "poisson" else 0)
        self._seed, self._offset = (0 if seed is None else int(seed)) & 0xFFFFFFFFFFFFFFFF, 0
        self._seed_arg = seed
        self.device_frame = bool(device_frame)              # the default frame by a streamed Laplace fit of the points in place
        self._status = torch.zeros(2, dtype=torch.int32, device=self.device)

    def coreset_path(self, k):
        """Whether k points run on the LDS-resident path (one launch, a workgroup per chain)."""
        return bool(self._lib.bcx_hmc_coreset_ok(int(k), self.D))

    def nuts_path(self, k):
        """Whether k points fit the LDS-resident NUTS kernel (``kernel="nuts"``: the only path it has without ``stream=True``)."""
        return bool(self._lib.bcx_nuts_coreset_ok(int(k), self.D))

    def adapt_path(self, k):
        """Whether k points fit the LDS-resident NUTS kernel that learns a metric (``adapt_metric``: the only path it has)."""
        return bool(self._lib.bcx_nuts_adapt_ok(int(k), self.D))

    @staticmethod
    def metric_windows(n_warmup):
        """The slow windows of a warm-up of ``n_warmup`` transitions, rows start, end (bcx_nuts_adapt_schedule)."""
        import ctypes
        from . import _native
        buf = (ctypes.c_int32 * (2 * NUTS_WINDOWS_MAX))()
        n = int(_native.load().bcx_nuts_adapt_schedule(int(n_warmup), buf, NUTS_WINDOWS_MAX))
        return np.array(buf[:2 * n], dtype=np.int64).reshape(n, 2)

    def _default_frame(self, k, pts, wts, Z=None, w=None):
        if k == 0:
            return np.zeros(self.D), None
        if self.device_frame and Z is not None:
            # csrc/laplace_stream.hip on the device rows (any k): no download of the points, no host Newton iteration
            lap = LaplacePosteriorSampler(self.family, self.D, device=self.device, seed=self._seed_arg, stream=True)
            return lap.posterior(w, Z)
        lap = LaplacePosteriorSampler(self.family, self.D, device=self.device, seed=self._seed_arg)
        host_pts = pts.cpu().numpy() if isinstance(pts, self._torch.Tensor) else np.asarray(pts, dtype=np.float64)
        host_w = None if wts is None else (wts.cpu().numpy() if isinstance(wts, self._torch.Tensor) else np.asarray(wts, dtype=np.float64))
        if lap.supports(self.D + 1, k):
            return lap.posterior(np.ones(k) if host_w is None else host_w, host_pts)
        mod = _example_model(self.family)
        mu, cov = mod.laplace_fit(host_pts, host_w)
        return mu, np.linalg.cholesky(cov).T

    def sample(self, pts, wts, n_samples, n_warmup=None, center=None, transform=None, keep_trace=False, _dev_step_size=None,
               _dev_force_stream=False):
        """``pts``: k rows (host array or device tensor; None / empty: the prior); ``wts``: k weights or None (ones);
        ``n_warmup`` defaults to ``n_samples`` (examples/common/mcmc.py:65).  ``center`` (D) / ``transform`` (D x D, Sigma ~
        transform^T transform) default to the Laplace fit of the same weighted posterior; ``transform=np.eye(D)``: plain HMC."""
        torch, lib, D, C, ld = self._torch, self._lib, self.D, self.chains, self.ld
        n_samples = int(n_samples)
        n_warmup = n_samples if n_warmup is None else int(n_warmup)
        if n_samples < 0 or n_warmup < 0 or n_samples + n_warmup < 1:
            raise ValueError("DeviceHMC.sample: at least one transition")
        T = n_samples + n_warmup
        k = 0 if pts is None else len(pts)
        nuts = self.kernel == "nuts"
        R = D + 3 * self.max_depth + 2 * ((1 << self.max_depth) - 1) if nuts else D + 3
        nuts_streamed = nuts and self.stream and (bool(_dev_force_stream) or not self.nuts_path(k))
        if self.adapt_metric is not None:
            if _dev_step_size is not None:
                raise ValueError("DeviceHMC: a fixed step (_dev_step_size) does not go with adapt_metric; drop one of them")
            if _dev_force_stream or not self.adapt_path(k):
                raise ValueError("DeviceHMC: adapt_metric runs only where the points fit one workgroup's LDS next to the metric's "
                                 "accumulators (%d points of %d parameters do not); drop adapt_metric, or pass fewer points" % (k, D))
        if nuts:
            if not self.stream and (_dev_force_stream or not self.nuts_path(k)):
                raise ValueError("DeviceHMC: NUTS without `stream=True` runs only where the points fit one workgroup's LDS; pass "
                                 "`stream=True` or `kernel=\"hmc\"`")
            if 8 * C * T * R > NUTS_NOISE_BYTES_MAX:
                raise ValueError("DeviceHMC: the NUTS noise (chains x transitions x %d doubles = %d bytes) exceeds 2 GiB; lower max_depth "
                                 "(%d), chains (%d) or the number of transitions (%d)" % (R, 8 * C * T * R, self.max_depth, C, T))
        Z = _device_rows(torch, self.device, pts, self.cols, "points") if k else None
        w = _device_weights(torch, self.device, wts, k, "DeviceHMC.sample")
        if center is None and transform is None:
            center, transform = self._default_frame(k, pts, wts, Z, w)
        mu = np.zeros(D) if center is None else np.ascontiguousarray(center, dtype=np.float64).reshape(D)
        Wm = None if transform is None else np.ascontiguousarray(transform, dtype=np.float64).reshape(D, D)
        mu_dev = torch.from_numpy(mu).to(self.device)
        W_dev = None if Wm is None else torch.from_numpy(Wm).to(self.device)
        streamed = nuts_streamed or (not nuts and (bool(_dev_force_stream) or not self.coreset_path(k)))
        if streamed and C > STREAM_CHAINS_MAX:
            raise ValueError("DeviceHMC: the streamed path takes at most %d chains" % STREAM_CHAINS_MAX)
        noise = self._normal(C, T, R)
        f64 = dict(dtype=torch.float64, device=self.device)
        samples = torch.empty(C, T, ld, **f64)
        xis = torch.empty(C, T, ld, **f64) if keep_trace else None
        props = torch.empty(C, T, ld, **f64) if keep_trace else None
        diag = torch.empty(C, T, NUTS_DIAG if nuts else DIAG, **f64)
        acc, eps = torch.empty(C, **f64), torch.empty(C, **f64)
        ptr = lambda t: None if t is None else t.data_ptr()
        fixed = 0.0 if _dev_step_size is None else float(_dev_step_size)
        windows = self.metric_windows(n_warmup) if self.adapt_metric is not None else None
        frames = None if windows is None else torch.empty(C, max(len(windows), 1), D, D, **f64)
        metric = None if windows is None else torch.empty(C, D, D, **f64)

        def native_args(stream, *scratch):
            # the four entry points' arguments.  Head: stream, family, k, D, weights, rows, row stride.  Tail: frame, counts, steps,
            # noise, outputs, status.  In between what differs: the leapfrog count, or max_depth and (behind the noise) its row length
            # R; the streamed ones end with their scratch and its bytes.
            depth_or_leapfrog, noise_ld = (self.max_depth, [R]) if nuts else (self.leapfrog, [])
            return ([stream, self._fam, k, D, ptr(w), ptr(Z), Z.stride(0) if k else self.cols, ptr(mu_dev), ptr(W_dev), D, C, n_warmup,
                     n_samples, depth_or_leapfrog, self.STEP0, fixed, noise.data_ptr()] + noise_ld +
                    [ld, samples.data_ptr(), ptr(xis), ptr(props), diag.data_ptr(), acc.data_ptr(), eps.data_ptr(), self._status.data_ptr()] +
                    list(scratch))

        with torch.cuda.device(self.device):
            stream = self._nat.stream_ptr(self.device)
            torch.cuda.synchronize(self.device)
            t0 = time.perf_counter()
            if nuts_streamed:
                nbytes = int(lib.bcx_nuts_stream_scratch_bytes(k, D, C, self.max_depth))
                if self._scratch is None or self._scratch.numel() * 8 < nbytes:
                    self._scratch = torch.empty(nbytes // 8 + 1, **f64)
                rc = lib.bcx_nuts_stream(*native_args(stream, self._scratch.data_ptr(), nbytes))
            elif self.adapt_metric is not None:
                rc = lib.bcx_nuts_adapt(*(native_args(stream) + [NUTS_METRICS[self.adapt_metric], frames.data_ptr(), metric.data_ptr()]))
            elif nuts:
                rc = lib.bcx_nuts_coreset(*native_args(stream))
            elif streamed:
                nbytes = int(lib.bcx_hmc_stream_scratch_bytes(k, D, C))
                work = torch.empty(nbytes // 8 + 1, **f64)
                rc = lib.bcx_hmc_stream(*native_args(stream, work.data_ptr(), nbytes))
            else:
                rc = lib.bcx_hmc_coreset(*native_args(stream))
            self._nat.check(rc)
            torch.cuda.synchronize(self.device)
            seconds = time.perf_counter() - t0
        st = self._status.cpu().numpy()
        if st[0] == 3:
            raise self._nat.EngineError(self._nat.ERR_TIMEOUT, "NUTS on the device: a wait between the workgroups of the streamed launch expired")
        if st[0] == 2:
            raise self._nat.EngineError(self._nat.ERR_STATE, "HMC on the device: the log joint at the start is not finite (NaN weights or points)")
        return self._result(n_samples, n_warmup, mu, Wm, seconds, streamed, int(st[0]), noise, samples, xis, props, diag, acc, eps, frames,
                            metric, windows)

    def _result(self, n_samples, n_warmup, mu, Wm, seconds, streamed, status, noise, samples, xis, props, diag, acc, eps, frames, metric,
                windows):
        """The HMCResult of one posterior from its device arrays (``sample``: the launch's; ``sample_many``: one problem's slices);
        ``xis`` / ``props``: None without ``keep_trace``; ``frames`` / ``metric`` / ``windows``: None without ``adapt_metric``."""
        D, C, T = self.D, self.chains, n_samples + n_warmup
        nuts, keep_trace = self.kernel == "nuts", xis is not None
        out = samples[:, n_warmup:, :D].cpu().numpy()
        dg = diag.cpu().numpy()
        if nuts:
            th = samples[:, :, :D].cpu().numpy()
            before = np.concatenate((np.broadcast_to(mu, (C, 1, D)), th[:, :-1]), axis=1)      # (every chain starts at xi = 0: theta = center)
            extra = dict(delta_h=dg[:, n_warmup:, 7], accepted=(th != before).any(axis=2)[:, n_warmup:], accept_stat=dg[:, n_warmup:, 0],
                         tree_depth=dg[:, n_warmup:, 1].astype(np.int64), n_leapfrog=dg[:, n_warmup:, 2].astype(np.int64),
                         divergent=dg[:, n_warmup:, 6] > 0.5, leapfrog_total=dg[:, :, 2].sum(axis=1).astype(np.int64), kernel="nuts",
                         max_depth=self.max_depth, adapt_metric=self.adapt_metric)
            if self.adapt_metric is not None:
                extra.update(metric=metric.cpu().numpy(), metric_windows=windows)
        else:
            extra = dict(delta_h=dg[:, n_warmup:, 0], accepted=dg[:, n_warmup:, 1] > 0.5, kernel="hmc")
        res = HMCResult(samples=out, accept_rate=acc.cpu().numpy(), step_size=eps.cpu().numpy(), rhat=split_rhat(out) if n_samples >= 4 else np.full(D, np.nan),
                        seconds_per_iteration=seconds / T, streamed=streamed, nonfinite_rejected=bool(status == 1),
                        center=mu, transform=np.eye(D) if Wm is None else Wm, n_warmup=n_warmup, trace=None, **extra)
        if keep_trace:
            res.trace = dict(noise=noise.cpu().numpy(), theta=samples[:, :, :D].cpu().numpy(), xi=xis[:, :, :D].cpu().numpy(),
                             proposal=props[:, :, :D].cpu().numpy(), diag=dg, step0=self.STEP0)
            if self.adapt_metric is not None:
                res.trace["frames"] = frames[:, :len(windows)].cpu().numpy()
        return res

    def sample_many(self, problems, n_samples, n_warmup=None, *, seeds=None, keep_trace=False):
        """Many weighted posteriors in ONE launch (``kernel="nuts"``, with or without ``adapt_metric``; bcx_nuts_batch, DESIGN.md
        4.18): a list of HMCResult, the p-th bit for bit what ``sample(pts, wts, n_samples, n_warmup, center, transform,
        keep_trace)`` returns for ``problems[p]`` -- a ``(pts, wts)`` pair or a dict with ``pts``, ``wts``, ``center``,
        ``transform`` (the last three optional; a missing frame is the Laplace fit of that problem, as in ``sample``).
        ``seeds=None``: the noise of problem p is what the p-th of P successive ``sample`` calls on this sampler would draw, and
        the sampler's stream advances as it would.  ``seeds=[s_0, ...]``: problem p reads what a fresh ``DeviceHMC(seed=s_p)``
        reads first, and this sampler's stream does not move.  ``seconds_per_iteration`` is the launch's wall time over the
        transitions, the same for every problem; ``batch_seconds`` that wall time.  A problem whose log joint at the start is not
        finite raises EngineError naming it (and those like it); the workgroups are dispatched by k descending (a heuristic)."""
        import ctypes
        torch, lib, nat, D, C, ld = self._torch, self._lib, self._nat, self.D, self.chains, self.ld
        if self.kernel != "nuts":
            raise ValueError("DeviceHMC.sample_many: kernel=\"nuts\" only (the fixed-length HMC has no batched launch); call sample per problem")
        if self.stream:
            raise ValueError("DeviceHMC.sample_many: the LDS-resident NUTS only (stream=True has no batched launch); drop stream=True")
        problems = list(problems)
        P = len(problems)
        if P == 0:
            raise ValueError("DeviceHMC.sample_many: no problems")
        if seeds is not None:
            seeds = list(seeds)
            if len(seeds) != P:
                raise ValueError("DeviceHMC.sample_many: %d seeds for %d problems" % (len(seeds), P))
        n_samples = int(n_samples)
        n_warmup = n_samples if n_warmup is None else int(n_warmup)
        if n_samples < 0 or n_warmup < 0 or n_samples + n_warmup < 1:
            raise ValueError("DeviceHMC.sample_many: at least one transition")
        T = n_samples + n_warmup
        R = D + 3 * self.max_depth + 2 * ((1 << self.max_depth) - 1)
        adapt = self.adapt_metric is not None
        items = []
        for p, prob in enumerate(problems):
            if isinstance(prob, dict):
                pts, wts, center, transform = prob.get("pts"), prob.get("wts"), prob.get("center"), prob.get("transform")
            else:
                (pts, wts), center, transform = prob, None, None
            k = 0 if pts is None else len(pts)
            if adapt and not self.adapt_path(k):
                raise ValueError("DeviceHMC.sample_many: problem %d: adapt_metric runs only where the points fit one workgroup's LDS next to "
                                 "the metric's accumulators (%d points of %d parameters do not)" % (p, k, D))
            if not self.nuts_path(k):
                raise ValueError("DeviceHMC.sample_many: problem %d: %d points of %d parameters do not fit one workgroup's LDS; sample it on "
                                 "its own with `stream=True` or `kernel=\"hmc\"`" % (p, k, D))
            items.append((pts, wts, center, transform, k))
        if 8 * P * C * T * R > NUTS_NOISE_BYTES_MAX:
            raise ValueError("DeviceHMC.sample_many: the NUTS noise (problems x chains x transitions x %d doubles = %d bytes) exceeds 2 GiB; "
                             "pass fewer problems (%d), or lower max_depth (%d), chains (%d) or the number of transitions (%d)"
                             % (R, 8 * P * C * T * R, P, self.max_depth, C, T))
        records = (nat.NutsProblem * P)()
        frames_host, keep = [], []
        for p, (pts, wts, center, transform, k) in enumerate(items):
            Z = _device_rows(torch, self.device, pts, self.cols, "points") if k else None
            w = _device_weights(torch, self.device, wts, k, "DeviceHMC.sample_many")
            if center is None and transform is None:
                center, transform = self._default_frame(k, pts, wts, Z, w)
            mu = np.zeros(D) if center is None else np.ascontiguousarray(center, dtype=np.float64).reshape(D)
            Wm = None if transform is None else np.ascontiguousarray(transform, dtype=np.float64).reshape(D, D)
            mu_dev = torch.from_numpy(mu).to(self.device)
            W_dev = None if Wm is None else torch.from_numpy(Wm).to(self.device)
            frames_host.append((mu, Wm))
            keep.append((Z, w, mu_dev, W_dev))
            r = records[p]
            r.w_dev, r.pts_dev, r.ldp = (None if w is None else w.data_ptr()), (Z.data_ptr() if k else None), (Z.stride(0) if k else self.cols)
            r.mu_dev, r.W_dev, r.ldw, r.k, r.index = mu_dev.data_ptr(), (None if W_dev is None else W_dev.data_ptr()), D, k, p
        f64 = dict(dtype=torch.float64, device=self.device)
        noise = torch.empty(P, C, T, R, **f64)
        pairs = (C * T * R + 1) // 2
        with torch.cuda.device(self.device):
            stream = nat.stream_ptr(self.device)
            for p in range(P):     # (the _normal(C, T, R) call of the p-th sample, into its slice)
                seed, offset = (self._seed, self._offset + p * pairs) if seeds is None else (int(seeds[p]) & 0xFFFFFFFFFFFFFFFF, 0)
                nat.check(lib.bcx_standard_normal(stream, seed, offset, C * T * R, noise[p].data_ptr()))
            if seeds is None:
                self._offset += P * pairs
            samples = torch.empty(P, C, T, ld, **f64)
            xis = torch.empty(P, C, T, ld, **f64) if keep_trace else None
            props = torch.empty(P, C, T, ld, **f64) if keep_trace else None
            diag = torch.empty(P, C, T, NUTS_DIAG, **f64)
            acc, eps = torch.empty(P, C, **f64), torch.empty(P, C, **f64)
            windows = self.metric_windows(n_warmup) if adapt else None
            frames = torch.empty(P, C, max(len(windows), 1), D, D, **f64) if adapt else None
            metric = torch.empty(P, C, D, D, **f64) if adapt else None
            status = torch.zeros(2 * P, dtype=torch.int32, device=self.device)
            table = torch.empty(int(lib.bcx_nuts_batch_table_bytes(P)), dtype=torch.uint8, device=self.device)
            ptr = lambda t: None if t is None else t.data_ptr()
            torch.cuda.synchronize(self.device)
            t0 = time.perf_counter()
            nat.check(lib.bcx_nuts_batch(stream, self._fam, P, records, table.data_ptr(), D, C, n_warmup, n_samples, self.max_depth, self.STEP0,
                                         noise.data_ptr(), R, ld, samples.data_ptr(), ptr(xis), ptr(props), diag.data_ptr(), acc.data_ptr(),
                                         eps.data_ptr(), status.data_ptr(), NUTS_METRICS[self.adapt_metric] if adapt else 0, ptr(frames),
                                         ptr(metric)))
            torch.cuda.synchronize(self.device)
            seconds = time.perf_counter() - t0
        del keep
        st = status.cpu().numpy().reshape(P, 2)[:, 0]
        bad = [p for p in range(P) if st[p] == 2]
        if bad:
            raise nat.EngineError(nat.ERR_STATE, "NUTS on the device: the log joint at the start is not finite (NaN weights or points) in "
                                  "problem%s %s" % ("" if len(bad) == 1 else "s", ", ".join(str(p) for p in bad)))
        at = lambda t, p: None if t is None else t[p]
        results = []
        for p, (mu, Wm) in enumerate(frames_host):
            res = self._result(n_samples, n_warmup, mu, Wm, seconds, False, int(st[p]), noise[p], samples[p], at(xis, p), at(props, p), diag[p],
                               acc[p], eps[p], at(frames, p), at(metric, p), windows)
            res.batch_seconds = seconds
            results.append(res)
        return results
