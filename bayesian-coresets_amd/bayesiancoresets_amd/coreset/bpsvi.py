"""Batch pseudocoreset variational inference (reference: bayesiancoresets/coreset/bpsvi.py:6-64).

``build(sz)`` starts from ``sz`` distinct data points drawn at random (bpsvi.py:15-22), each with weight N / sz, and then
moves the weights AND the points themselves by ``opt_itrs`` steps of projected ADAM (util/opt.py: only the weights are
kept non-negative).  The objective's gradient at (w, P) needs, after the sampler has drawn S parameters at (w, P):

* the column sums of the projected data (or of a fresh random sub-sample of it, scaled by N / n);
* the projected pseudo-points (k x S) and the gradients of those projections with respect to the points (k x S x dz).

With a ``DeviceProjector`` all of it is one call, ``psvi_gradient``: the data's column sums as SparseVI takes them (fused
projection, or the closed form for the linear-regression family), the points' projection, and the pseudo-point gradient
as two products on the matrix cores (csrc/psvi.hip) -- the k x S x dz tensor is never formed, and one device->host copy
returns (wgrad, ugrad).  The host keeps the ADAM state, the sampler calls and the random draws, in the reference's order:
``choice`` once per build, then per step the sampler (projector.update) and, with ``n_subsample_opt``, one ``randint``.
A NumPy sampler therefore reproduces the reference's trajectory.

With one of the package's device samplers (``enqueue_plan_moving``) and the full data set at every step, the whole loop is
enqueued instead (``_optimize_enqueued``): weights, points and ADAM moments stay on the device, the sampler draws from them there,
``bcx_psvi_adam_step`` takes the step, and the host reads (w, P) back once after ``opt_itrs`` steps.

With ``subsample="device"`` a sub-sampled step projects the drawn rows of the resident data set in place (``rows=``: the gathered
consumers of csrc/proj.hip, the bits of the gathered copy) instead of gathering ``data[sub]``, and the enqueued loop serves
``n_subsample_opt`` too, on an index table drawn up front by the host loop's own ``randint`` calls (``_enqueue_plan_subsampled``).

There is no host path: any other projector raises NotImplementedError.  The Poisson family's gradient has D entries for
points of D + 1 columns, where the reference fails reshaping it (bpsvi.py:56): ``build`` raises ValueError before any
draw."""
import numpy as np

from .coreset import Coreset
from ..util.opt import nn_opt
from ..projector import DeviceProjector
from .. import _native as nat


class BatchPSVICoreset(Coreset):
    def __init__(self, data, ll_projector, opt_itrs, n_subsample_opt=None, step_sched=lambda i: 1.0 / (1.0 + i), *, subsample="host",
                 **kw):
        """``subsample`` (keyword-only): "host" (default) gathers ``data[sub]`` for every sub-sampled step; "device" keeps the data set
        resident on the projector's device and projects the drawn rows in place -- same ``randint`` calls, same results bit for bit
        (``colsum`` "auto" / "mfma").  One rank only."""
        if subsample not in ("host", "device"):
            raise ValueError("subsample must be 'host' or 'device'")
        if subsample == "device" and not isinstance(ll_projector, DeviceProjector):
            raise ValueError("subsample='device' needs a DeviceProjector")
        if subsample == "device" and (getattr(ll_projector, "group", None) is not None or getattr(ll_projector, "_world", 1) > 1):
            raise ValueError("subsample='device' is provided on one rank only (a projector with a group is row-sharded)")
        self.subsample = subsample
        self._data_dev = None
        if not isinstance(ll_projector, DeviceProjector):
            raise NotImplementedError("BatchPSVICoreset runs on the device only: it needs a bc.DeviceProjector (the pseudo-point "
                                      "gradients are csrc/psvi.hip kernels; there is no host fallback)")
        self.data = data
        self.ll_projector = ll_projector
        self.opt_itrs = opt_itrs
        n = data.shape[0]
        self.n_subsample_opt = None if n_subsample_opt is None else min(n, n_subsample_opt)    # bpsvi.py:11
        self.step_sched = step_sched
        super().__init__(**kw)

    def _rows(self, idx):
        """data[idx] as a host array (``data`` may be a device tensor)."""
        rows = self._sub(idx)
        if hasattr(rows, "detach"):
            rows = rows.detach().cpu().numpy()
        return np.array(rows, dtype=np.float64)

    def _resident(self):
        """The data set on the projector's device, made resident once (``subsample="device"``) and kept by this object."""
        if self._data_dev is None:
            self._data_dev = self.ll_projector._dev(self.data)
        return self._data_dev

    def _sub(self, idx):
        """data[idx] where it lives (a device tensor is indexed on its device)."""
        if hasattr(self.data, "detach"):
            import torch
            return self.data[torch.as_tensor(idx, device=self.data.device)]
        return self.data[idx]

    # ---- bpsvi.py:15-22 ----------------------------------------------------------------------------------------------
    def _build(self, sz):
        if self.ll_projector.family == "poisson":
            raise ValueError("BatchPSVICoreset: the Poisson family's pseudo-point gradient has D entries for points of D + 1 "
                             "columns (the reference fails at bpsvi.py:56 reshaping it)")
        n = self.data.shape[0]
        first = np.random.choice(n, size=sz, replace=False)        # every build starts afresh
        self.pts = self._rows(first)
        self.wts = n / sz * np.ones(sz)
        self.idcs = -1 * np.ones(sz)                               # (a float array, as in the reference)
        self._optimize()

    # ---- bpsvi.py:42-60 ----------------------------------------------------------------------------------------------
    def _optimize(self):
        plan = self._enqueue_plan()
        if plan is not None:
            self.wts, self.pts = self._optimize_enqueued(plan)
            return
        plan = self._enqueue_plan_subsampled()
        if plan is not None:
            self.wts, self.pts = self._optimize_enqueued(plan, n_sub=self.n_subsample_opt)
            return
        on_device = self.subsample == "device"
        k, d = self.wts.shape[0], self.pts.shape[1]
        prj, n, nsub = self.ll_projector, self.data.shape[0], self.n_subsample_opt

        def grd(x):
            w, p = x[:k], x[k:].reshape((k, d))
            prj.update(w, p)                                       # bpsvi.py:26
            rows = None
            if nsub is None:
                pts, scaling = self.data, 1.0
            elif on_device:
                pts, scaling, rows = self._resident(), n / nsub, np.random.randint(n, size=nsub)      # bpsvi.py:34-36, rows in place
            else:
                pts, scaling = self._sub(np.random.randint(n, size=nsub)), n / nsub       # bpsvi.py:34-36
            if k == 0:
                return np.zeros(0)
            wgrad, ugrad = prj.psvi_gradient(pts, p, w, scaling, persistent=pts is self.data and rows is None, rows=rows)
            if ugrad.shape[1] != d:
                raise ValueError("pseudo-point gradient has %d entries for points of %d columns" % (ugrad.shape[1], d))
            return np.hstack((wgrad, ugrad.reshape(k * d)))

        x0 = np.hstack((self.wts, self.pts.reshape(k * d)))
        x = nn_opt(x0, grd, nn_idcs=np.arange(k), opt_itrs=self.opt_itrs, step_sched=self.step_sched)
        self.wts, self.pts = x[:k], x[k:].reshape((k, d))

    # ---- the same loop with the weights AND the points resident on the device (csrc/psvi.hip psvi_adam_kernel) ------------------
    ENQUEUE = True      # False: always the host loop above (tests compare the two)

    def _enqueue_plan(self):
        """A moving-points draw plan when the whole ADAM loop can be enqueued: device projector on one rank, the full data set at
        every step (a per-step sub-sample is a host ``randint`` + gather), and a sampler that can draw from weights and points that
        live on the device and move (``enqueue_plan_moving``: the package's three device samplers)."""
        prj = self.ll_projector
        k = self.wts.shape[0]
        if not (self.ENQUEUE and isinstance(prj, DeviceProjector) and prj._world == 1 and self.n_subsample_opt is None
                and self.opt_itrs > 0 and 1 <= k <= 4096 and prj.projection_dimension <= 8192 and prj.family != "poisson"):
            return None
        make = getattr(prj.sampler, "enqueue_plan_moving", None)
        return None if make is None else make(prj.projection_dimension, k, self.pts.shape[1], self.opt_itrs)

    INDEX_BUDGET = 1 << 30      # bytes of pre-drawn row indices (opt_itrs x n_subsample_opt int64) an enqueued loop may hold

    def _enqueue_plan_subsampled(self):
        """The same for ``subsample="device"`` with ``n_subsample_opt``: the conditions of ``_enqueue_plan`` with the per-step
        sub-sample in the place of the full data set, plus the loop's index table fitting INDEX_BUDGET (beyond it the host loop
        serves).  ``_enqueue_plan`` itself keeps returning None with ``n_subsample_opt``."""
        prj = self.ll_projector
        k = self.wts.shape[0]
        if not (self.ENQUEUE and self.subsample == "device" and isinstance(prj, DeviceProjector) and prj._world == 1
                and self.n_subsample_opt is not None and self.opt_itrs > 0 and 1 <= k <= 4096 and prj.projection_dimension <= 8192
                and prj.family != "poisson" and 8 * self.opt_itrs * self.n_subsample_opt <= self.INDEX_BUDGET):
            return None
        make = getattr(prj.sampler, "enqueue_plan_moving", None)
        return None if make is None else make(prj.projection_dimension, k, self.pts.shape[1], self.opt_itrs)

    def _optimize_enqueued(self, plan, b1=0.9, b2=0.999, eps=1e-8, n_sub=None):
        """nn_opt (util/opt.py:4-28) with grd = bpsvi.py:47-55 and nn_idcs = arange(k), enqueued on the projector's stream: per step
        the sampler's draw at the device-resident weights and points, the gradient left on the device
        (``psvi_gradient_enqueue``) and ``bcx_psvi_adam_step`` on x = [w | P].  One upload before the loop (the schedule is
        evaluated on the host up front), one read-back after it.  ``n_sub``: every step takes the column sums of a fresh sub-sample
        of that many rows (scaling N / n_sub): the host draws the loop's indices up front by the host loop's own calls, one
        ``randint(n, size=n_sub)`` per step in step order, uploads them once, and step i projects the rows of table row i in place."""
        prj = self.ll_projector
        torch = prj._torch
        k, d, T = self.wts.shape[0], self.pts.shape[1], self.opt_itrs
        ldp, kq = plan.ldp, k + k % 2
        sched = np.array([(self.step_sched(i), 1.0 - b1 ** (i + 1), 1.0 - b2 ** (i + 1)) for i in range(T)], dtype=np.float64)
        nm = kq + k * ldp
        state = torch.from_numpy(np.concatenate((np.asarray(self.wts, dtype=np.float64), np.zeros(kq - k + 2 * nm), sched.ravel()))).to(prj.device)
        w, m1, m2, sched_d = state[:k], state[kq:kq + nm], state[kq + nm:kq + 2 * nm], state[kq + 2 * nm:]
        plan.set_points(self.pts)
        P = plan.points
        theta, mean = plan.buffers()
        if n_sub is None:
            run, out, dz = prj.psvi_gradient_enqueue(self.data, P, w, 1.0, True, theta, mean)      # bpsvi.py:47-55
        else:
            n = self.data.shape[0]
            table = np.stack([np.random.randint(n, size=n_sub) for _ in range(T)])                # bpsvi.py:34, T calls
            run, out, dz = prj.psvi_gradient_enqueue(self._resident(), P, w, n / n_sub, False, theta, mean, rows=table)
        if dz != d:
            raise ValueError("pseudo-point gradient has %d entries for points of %d columns" % (dz, d))
        mir = plan.mirror
        adam = prj._lib.bcx_psvi_adam_step
        args = [prj._stream(), k, d, out.data_ptr(), prj.projection_dimension, w.data_ptr(), P.data_ptr(), ldp, m1.data_ptr(),
                m2.data_ptr(), sched_d.data_ptr(), 0, b1, b2, eps, None if mir is None else mir[0].data_ptr(),
                0 if mir is None else mir[1], None if mir is None else mir[2].data_ptr(), None]
        for i in range(T):
            plan.draw(w, i)                                                       # bpsvi.py:26
            run() if n_sub is None else run(i)
            args[11] = i
            prj._check(adam(*args))
        res = torch.cat((w, P.reshape(-1))).cpu().numpy()
        plan.check()                                                              # (a failed factorisation / fit at any step raises)
        if not np.isfinite(res).all():
            # the reference's loop ends with NaN weights / points here (np.maximum keeps a NaN, and so does the ADAM kernel): an error
            raise nat.EngineError(nat.ERR_STATE, "BatchPSVI: the optimisation ended with weights or points that are not finite")
        return res[:k].copy(), res[k:].reshape(k, d).copy()

    def error(self):
        return 0.0   # as in the reference (bpsvi.py:62-63: the KL estimate is not implemented)
