"""Quasi-Newton coreset (Naik, Rousseau and Campbell, "Fast Bayesian coresets via subsampling and quasi-Newton refinement",
2022): draw the M points uniformly once, then take ``opt_itrs`` second-order steps on all M weights together.

State: k points (rows of the data set, fixed after the draw) and weights w >= 0.  One step i, with draws theta_1 .. theta_S
from the sampler at (w, pts):

    V      k x S   log-likelihoods of the coreset points at the draws, each row centred over the draws (projector.py:21)
    c      S       scaling x column sums of the centred log-likelihoods of the data (scaling = N / n_sub, 1 without sub-sampling)
    resid  = c - V^T w                                  (sparsevi.py:47 / :72)
    b      = V resid / S                                (minus SparseVI's gradient, sparsevi.py:74)
    G      = V V^T / S
    d      : (G + tau I) d = b                          (tau >= 0, absolute, in squared log-likelihood units)
    w      <- max(w + gamma_i d, 0)                     (NumPy's maximum: a NaN stays a NaN)

``build(sz)`` follows ``BatchPSVICoreset._build`` (bpsvi.py:15-22): ``idcs = np.random.choice(N, size=sz, replace=False)``,
``pts = data[idcs]``, ``wts = N / sz``, then ``opt_itrs`` steps; unlike BatchPSVI the points do not move and ``idcs`` keeps the
drawn rows.  A second ``build`` starts afresh; ``optimize()`` runs ``opt_itrs`` more steps.

The N-sized pieces are SparseVI's (``_residual``, the enqueue plans): the class is built on ``SparseVICoreset``.  Two forms of the
loop, chosen by SparseVI's conditions -- the host loop (any ``Projector``; the step in NumPy float64 with ``np.linalg.cholesky``)
and the enqueued loop (``DeviceProjector`` + a device sampler: per step the sampler's draw at the device-resident weights, the two
projections, ``bcx_quasi_newton_step``, csrc/qn.hip; the weights are read back once)."""
import numpy as np

from .sparsevi import SparseVICoreset
from .. import _native as nat


class QuasiNewtonCoreset(SparseVICoreset):
    def __init__(self, data, ll_projector, opt_itrs=20, n_subsample_opt=None, step_sched=lambda i: 1.0, tau=1e-2, *, subsample="host",
                 **kw):
        if kw.get("group") is not None or kw.get("row_offset", 0):
            raise ValueError("QuasiNewtonCoreset: row-sharded construction (group= / row_offset=) is not provided")
        kw.pop("group", None)
        kw.pop("row_offset", None)
        if not tau >= 0.0:
            raise ValueError("tau must be >= 0")
        if opt_itrs < 0:
            raise ValueError("opt_itrs must be >= 0")
        if getattr(ll_projector, "_world", 1) > 1:
            raise ValueError("QuasiNewtonCoreset: row-sharded construction is not provided (the projector has a group)")
        super().__init__(data, ll_projector, n_subsample_select=None, n_subsample_opt=n_subsample_opt, opt_itrs=opt_itrs,
                         step_sched=step_sched, subsample=subsample, **kw)
        self.tau = float(tau)

    # ---- bpsvi.py:15-22, the points fixed -----------------------------------------------------------------------------------------
    def _build(self, sz):
        n = self.data.shape[0]
        first = np.random.choice(n, size=sz, replace=False)        # every build starts afresh
        rows = self.data[first] if not hasattr(self.data, "detach") else self.data[self.ll_projector._torch.as_tensor(first, device=self.data.device)]
        self.pts = np.array(self._host_row(rows), dtype=np.float64)
        self.wts = n / sz * np.ones(sz)
        self.idcs = first.astype(np.int64)
        self._optimize()

    def _optimize(self):
        if self.wts.shape[0] == 0 or self.opt_itrs == 0:
            return
        plan = self._enqueue_plan()
        if plan is not None:
            self.wts = self._optimize_enqueued(plan)
            return
        plan = self._enqueue_plan_subsampled()
        if plan is not None:
            self.wts = self._optimize_enqueued(plan, n_sub=self.n_subsample_opt)
            return
        w = np.asarray(self.wts, dtype=np.float64)
        for i in range(self.opt_itrs):
            resid, sub, pts, eng, corevecs = self._residual(self.n_subsample_opt, w)
            # (resid = scaling colsum - w corevecs already; the step restated from it)
            S = corevecs.shape[1]
            try:
                L = np.linalg.cholesky(corevecs.dot(corevecs.T) / S + self.tau * np.eye(w.shape[0]))
            except np.linalg.LinAlgError as e:
                raise nat.EngineError(nat.ERR_STATE, "QuasiNewton: step %d: G + tau I has no Cholesky factor (%s)" % (i, e))
            d = np.linalg.solve(L.T, np.linalg.solve(L, corevecs.dot(resid) / S))
            w = np.maximum(w + self.step_sched(i) * d, 0.0)
        self._finite(w)
        self.wts = w

    @staticmethod
    def _finite(w):
        if not np.isfinite(w).all():
            raise nat.EngineError(nat.ERR_STATE, "QuasiNewton: the weight optimisation ended with weights that are not finite")

    def _optimize_enqueued(self, plan, n_sub=None):
        """The loop enqueued: per step the sampler's draw kernel at the current device weights, the two projections (column sums of
        the data or of table row i of a pre-drawn sub-sample; the coreset points, raw), and ``bcx_quasi_newton_step``.  The host
        evaluates the schedule up front, clears the status word before the loop and reads it, with the weights, once after it."""
        prj = self.ll_projector
        torch, lib = prj._torch, prj._lib
        k, S, T = self.wts.shape[0], prj.projection_dimension, self.opt_itrs
        sched = np.array([self.step_sched(i) for i in range(T)], dtype=np.float64)
        # one upload: [weights | status word (an int32 in a double's place, zero: cleared) | schedule]; the head is read back once
        state = torch.from_numpy(np.concatenate((np.asarray(self.wts, dtype=np.float64), np.zeros(1), sched))).to(prj.device)
        w, status, sched_d = state[:k], state[k:k + 1], state[k + 1:]
        theta, mean = plan.buffers()
        scaling = 1.0
        if n_sub is None:
            run, buf, _ = prj.enqueue_step_plan(self.data, self._core_points_device(), True, theta, mean)    # sparsevi.py:35-41
        else:
            table = np.stack([np.random.randint(self.n_global, size=n_sub) for _ in range(T)])           # sparsevi.py:33, T calls
            scaling = self.n_global / n_sub
            run, buf, _ = prj.enqueue_step_plan(self._resident(), self._core_points_device(), False, theta, mean, rows=table)
        need = int(lib.bcx_quasi_newton_scratch_bytes(k, S))
        work = torch.empty(need // 8 + 2, dtype=torch.float64, device=prj.device)
        args = [prj._stream(), k, S, buf.data_ptr(), scaling, buf[S:].data_ptr(), S, 1, w.data_ptr(), sched_d.data_ptr(), 0, self.tau,
                None, None, status.data_ptr(), work.data_ptr(), work.numel() * 8]
        for i in range(T):
            plan.draw(w, i)                                                       # sparsevi.py:25
            run() if n_sub is None else run(i)
            args[10] = i
            prj._check(lib.bcx_quasi_newton_step(*args))
        head = state[:k + 1].cpu().numpy()
        out, failed = head[:k].copy(), int(head[k:].view(np.int32)[0])
        check = getattr(plan, "check", None)
        if check is not None:
            check()                                                               # (a failed factorisation / fit of the sampler raises)
        if failed:
            raise nat.EngineError(nat.ERR_STATE, "QuasiNewton: G + tau I had a pivot that is not positive (or NaN) at some step: "
                                                 "no Cholesky factor; the weights stopped there")
        self._finite(out)
        return out
