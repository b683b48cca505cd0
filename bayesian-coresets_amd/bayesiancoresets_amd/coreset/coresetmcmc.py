"""Coreset MCMC (Chen and Campbell, "Coreset Markov chain Monte Carlo", 2024): the weights of M uniformly drawn points are
learned from K Markov chains that target the coreset posterior itself while they run -- no Laplace stand-in in the loop.

State: M points (rows of the data set, fixed after the draw), weights w >= 0, K chains at positions xi_c in a fixed frame
theta = mu + W^T xi (the Laplace fit of the points at the initial weights N / M), per chain the HMC base step and its
dual-averaging state, the ADAM moments.  Iteration i:

    advance  every chain takes ``thin`` HMC transitions (``leapfrog`` steps, csrc/hmc.hip) on sum_m w_m log p(z_m | theta)
             - |theta|^2 / 2 at the current w; the target at the carried state is evaluated again first (the cached value
             belongs to the previous weights); the transitions of the first ``n_adapt`` iterations adapt the step
    V        M x K   log-likelihoods of the points at the K states (the Poisson -log y! dropped: it cancels below)
    s        K       sum over the rows R_i of the data's log-likelihoods at the K states; R_i = all N rows, or row i of a
                     table of ``n_subsample`` indices, one ``np.random.randint(N, size=n_subsample)`` per iteration
    centre   V <- V - mean over the chains (per point), s <- s - mean(s)
    resid  = (N / n_sub) s - V^T w;   g = -V resid / K
    w      <- max(w - ADAM(g, gamma_i), 0)             (util/opt.py: b1 0.9, b2 0.999, eps 1e-8; a NaN stays a NaN)

The paper divides the gradient by K - 1.  ADAM's step is invariant to that factor except through eps, and the package's 1 / K
is kept so that the weight step is ``bcx_sparsevi_adam_step_ws`` (csrc/svi.hip) as it stands, with S = K.

Per iteration the host enqueues ``bcx_cmc_advance`` (the chains' launch, one workgroup per chain with the points in LDS, and the
one-workgroup launch that centres s) and the ADAM step; nothing is read back inside the loop.  The normal numbers come from the
library's counter-based generator at an offset that depends only on (seed, iteration, chain, transition), so a run is the same
bits however it is split into ``build`` and ``optimize()`` calls.  ``status`` follows ``DeviceHMC``: a log joint that is not
finite at a launch's start (NaN points or weights) raises EngineError after the loop, and so do weights that are not finite; a
transition rejected for a non-finite dH is reported as ``result.nonfinite_rejected``.

Limits: logistic / Poisson, D <= 32, the (M, D) that fit one workgroup's LDS, M <= 4096, at most 8192 chains, one device.
There is no CPU fallback."""
import numpy as np

from .coreset import Coreset
from .. import _native as nat
from ..laplace_sampler import FAMILIES
from ..linreg_sampler import _DeviceNormals
from ..mcmc import DIAG, DMAX, DeviceHMC, HMCResult, _device_rows, split_rhat

CHAINS_MAX = 8192
POINTS_MAX = 4096
NOISE_BYTES_MAX = 2 << 30


def default_step_sched(N, M):
    """gamma_i = 0.05 (N / M) / sqrt(1 + i / 10): steps of a fixed fraction of the initial weight, decaying slowly."""
    scale = 0.05 * N / M
    return lambda i: scale / np.sqrt(1.0 + i / 10.0)


class CoresetMCMC(Coreset, _DeviceNormals):
    def __init__(self, data, family, chains=64, leapfrog=8, thin=1, opt_itrs=500, n_subsample=None, step_sched=None, n_adapt=None,
                 seed=None, device="cuda"):
        if family not in FAMILIES:
            raise ValueError("family must be 'logistic' or 'poisson'")
        if getattr(data, "ndim", None) is None and not hasattr(data, "dim"):
            data = np.asarray(data, dtype=np.float64)
        if len(data.shape) != 2 or data.shape[0] < 1:
            raise ValueError("CoresetMCMC: data must be N x columns with N >= 1")
        D = int(data.shape[1]) - (1 if family == "poisson" else 0)
        if not 1 <= D <= DMAX:
            raise ValueError("CoresetMCMC: D = %d parameters (1 <= D <= %d)" % (D, DMAX))
        if int(chains) < 1 or int(leapfrog) < 1:
            raise ValueError("CoresetMCMC: at least one chain and one leapfrog step")
        if int(chains) > CHAINS_MAX:
            raise ValueError("CoresetMCMC: at most %d chains" % CHAINS_MAX)
        if int(thin) < 1 or int(opt_itrs) < 0:
            raise ValueError("CoresetMCMC: thin >= 1 and opt_itrs >= 0")
        if n_subsample is not None and int(n_subsample) < 1:
            raise ValueError("CoresetMCMC: n_subsample must be at least 1 (or None: all rows)")
        if n_adapt is not None and int(n_adapt) < 0:
            raise ValueError("CoresetMCMC: n_adapt >= 0")
        # (raises RuntimeError without a GPU; the default frame of build() is this sampler's)
        self._hmc = DeviceHMC(family, D, chains=chains, leapfrog=leapfrog, seed=seed, device=device)
        self._torch, self._nat, self._lib, self.device = self._hmc._torch, nat, self._hmc._lib, self._hmc.device
        self.family, self._fam, self.D, self.ld, self.cols = family, FAMILIES[family], D, self._hmc.ld, self._hmc.cols
        self.chains, self.leapfrog, self.thin, self.opt_itrs = int(chains), int(leapfrog), int(thin), int(opt_itrs)
        self.n_subsample = None if n_subsample is None else int(n_subsample)
        self.step_sched = step_sched
        self.n_adapt = self.opt_itrs // 2 if n_adapt is None else int(n_adapt)
        self._seed, self._offset = self._hmc._seed, 0
        self.data = data
        self.n = int(data.shape[0])
        self._Z = _device_rows(self._torch, self.device, data, self.cols, "data")      # the resident data set
        super().__init__()
        self._run_state, self.result, self.trace = None, None, None
        self._keep_trace, self._noise_arg = False, None

    # ---- the public surface ---------------------------------------------------------------------------------------------------------
    def reset(self):
        super().reset()
        self._run_state, self.result = None, None

    def build(self, M, keep_trace=False, _dev_noise=None):
        """Draw M points uniformly, start the chains at xi = 0 and the weights at N / M, run ``opt_itrs`` iterations.  A second
        ``build`` starts afresh.  ``keep_trace`` / ``_dev_noise`` are development arguments: the first keeps, per iteration, the
        weights after the step, V, the centred s, the chains' xi / proposal / diag and the noise in ``self.trace``; the second
        supplies the noise (opt_itrs x chains x thin x (D + 3))."""
        self._keep_trace, self._noise_arg = bool(keep_trace), _dev_noise
        try:
            super().build(M)
        finally:
            self._keep_trace, self._noise_arg = False, None      # (optimize() keeps no trace and draws its own noise)

    def error(self):
        return 0.0   # as for SparseVI: no KL estimate

    def samples(self, burn=None):
        """(chains, kept iterations, D): theta after each iteration's last transition, the first ``burn`` iterations dropped
        (default: ``n_adapt``)."""
        if self._run_state is None:
            return np.zeros((self.chains, 0, self.D))
        burn = self.n_adapt if burn is None else int(burn)
        th = np.concatenate(self._run_state["theta"], axis=0)                  # iterations x chains x D
        return np.ascontiguousarray(th[burn:].transpose(1, 0, 2))

    # ---- Coreset's hooks ------------------------------------------------------------------------------------------------------------
    def _build(self, M):
        torch, lib, D, K = self._torch, self._lib, self.D, self.chains
        M = int(M)
        if M > self.n:
            raise ValueError("CoresetMCMC: %d points of %d rows" % (M, self.n))
        if M > POINTS_MAX or not lib.bcx_cmc_advance_ok(M, D):
            raise ValueError("CoresetMCMC: %d points of %d parameters do not fit one workgroup's LDS (or exceed %d)" % (M, D, POINTS_MAX))
        first = np.random.choice(self.n, size=M, replace=False)        # every build starts afresh
        idx = torch.from_numpy(first.astype(np.int64)).to(self.device)
        pts_dev = self._Z[idx].contiguous()
        self.pts = pts_dev.cpu().numpy()
        self.wts = self.n / M * np.ones(M)
        self.idcs = first.astype(np.int64)
        # the frame: the Laplace fit of the points at the initial weights, as DeviceHMC.sample's default; fixed for the run
        w_dev = torch.from_numpy(self.wts).to(self.device)
        mu, Wm = self._hmc._default_frame(M, self.pts, self.wts, pts_dev, w_dev)
        mu = np.ascontiguousarray(mu, dtype=np.float64).reshape(D)
        Wm = np.eye(D) if Wm is None else np.ascontiguousarray(Wm, dtype=np.float64).reshape(D, D)
        f64 = dict(dtype=torch.float64, device=self.device)
        nstate = int(lib.bcx_cmc_state_bytes(K)) // 8
        self._run_state = dict(
            pts=pts_dev, mu=torch.from_numpy(mu).to(self.device), W=torch.from_numpy(Wm).to(self.device), center=mu, transform=Wm,
            # [weights | status (two int32 in a double's place) | ADAM moments]: the head is read back once per run
            head=torch.cat((w_dev, torch.zeros(1 + 2 * M, **f64))), chains=torch.zeros(nstate, **f64), iteration=0,
            sched=self.step_sched if self.step_sched is not None else default_step_sched(self.n, M),
            theta=[], diag=[], nonfinite=False)
        self.trace = None
        self._optimize()

    def _optimize(self):
        st = self._run_state
        if st is None or self.wts.shape[0] == 0 or self.opt_itrs == 0:
            return
        torch, lib, D, K, ld, thin = self._torch, self._lib, self.D, self.chains, self.ld, self.thin
        M, T, i0 = self.wts.shape[0], self.opt_itrs, st["iteration"]
        if (i0 + T) * thin > 2 ** 31 - 1:
            raise ValueError("CoresetMCMC: more than 2^31 - 1 transitions in a chain's life")
        b1, b2, eps = 0.9, 0.999, 1e-8
        f64 = dict(dtype=torch.float64, device=self.device)
        sched = np.array([(st["sched"](i), 1.0 - b1 ** (i + 1), 1.0 - b2 ** (i + 1)) for i in range(i0, i0 + T)], dtype=np.float64)
        sched_d = torch.from_numpy(sched.ravel()).to(self.device)
        head = st["head"]
        w, status, m1, m2 = head[:M], head[M:M + 1], head[M + 1:2 * M + 1], head[2 * M + 1:]
        status.zero_()
        table, n_sub, scaling = None, 0, 1.0
        if self.n_subsample is not None:
            n_sub = self.n_subsample
            table = torch.from_numpy(np.stack([np.random.randint(self.n, size=n_sub) for _ in range(T)]).astype(np.int64)).to(self.device)
            scaling = self.n / n_sub
        noise = self._iteration_noise(i0, T)
        keep = self._keep_trace
        samples, diag = torch.empty(T, K, thin, ld, **f64), torch.empty(T, K, thin, DIAG, **f64)
        xis = torch.empty(T, K, thin, ld, **f64) if keep else None
        props = torch.empty(T, K, thin, ld, **f64) if keep else None
        V = torch.empty((T if keep else 1), M, K, **f64)
        s = torch.empty((T if keep else 1), K, **f64)
        wtrace = torch.empty(T, M, **f64) if keep else None
        need = int(lib.bcx_sparsevi_adam_scratch_bytes(M, K))
        work = torch.empty(max(need // 8, 1), **f64)
        Z, pts = self._Z, st["pts"]
        ptr = lambda t: None if t is None else t.data_ptr()
        with torch.cuda.device(self.device):
            stream = nat.stream_ptr(self.device)
            for i in range(T):
                Vi, si = (V[i], s[i]) if keep else (V[0], s[0])
                rc = lib.bcx_cmc_advance(stream, self._fam, M, D, w.data_ptr(), pts.data_ptr(), pts.stride(0), st["mu"].data_ptr(),
                                         st["W"].data_ptr(), D, K, thin, self.leapfrog, DeviceHMC.STEP0, (i0 + i) * thin, self.n_adapt * thin,
                                         1 if i0 + i == 0 else 0, noise[i].data_ptr(), st["chains"].data_ptr(), Z.data_ptr(), self.n,
                                         Z.stride(0), None if table is None else table[i].data_ptr(), n_sub, Vi.data_ptr(), K, si.data_ptr(),
                                         ld, samples[i].data_ptr(), None if xis is None else xis[i].data_ptr(),
                                         None if props is None else props[i].data_ptr(), diag[i].data_ptr(), status.data_ptr())
                if rc == 0:
                    rc = lib.bcx_sparsevi_adam_step_ws(stream, M, K, si.data_ptr(), scaling, Vi.data_ptr(), K, w.data_ptr(), m1.data_ptr(),
                                                       m2.data_ptr(), sched_d.data_ptr(), i, b1, b2, eps, ptr(wtrace), 1, work.data_ptr(),
                                                       work.numel() * 8)
                nat.check(rc)
            got = head[:M + 1].cpu().numpy()                                    # the one read-back: weights and status
        out, worst = got[:M].copy(), int(got[M:].view(np.int32)[1])
        st["iteration"] = i0 + T
        self.status = worst
        if worst == 2:
            raise nat.EngineError(nat.ERR_STATE, "CoresetMCMC: the log joint at a launch's start was not finite (NaN weights or points)")
        if not np.isfinite(out).all():
            raise nat.EngineError(nat.ERR_STATE, "CoresetMCMC: the weight optimisation ended with weights that are not finite")
        st["nonfinite"] = st["nonfinite"] or worst == 1
        st["theta"].append(samples[:, :, thin - 1, :D].cpu().numpy())
        st["diag"].append(diag.cpu().numpy())
        if keep:
            tr = dict(weights=wtrace.cpu().numpy(), V=V.cpu().numpy(), s=s.cpu().numpy(), xi=xis[..., :D].cpu().numpy(),
                      proposal=props[..., :D].cpu().numpy(), diag=st["diag"][-1], noise=noise.cpu().numpy(),
                      theta=samples[..., :D].cpu().numpy(), table=None if table is None else table.cpu().numpy(), step0=DeviceHMC.STEP0,
                      sched=sched, first_iteration=i0)
            self.trace = tr
        self.wts = out
        self.result = self._result()

    # ---- pieces ---------------------------------------------------------------------------------------------------------------------
    def _iteration_noise(self, i0, T):
        """The normals of iterations i0 .. i0 + T - 1 as a (T, chains, thin, D + 3) view: iteration i's block starts at the pair
        counter i x ceil(chains thin (D + 3) / 2), whatever call draws it."""
        torch, K, thin, R = self._torch, self.chains, self.thin, self.D + 3
        if self._noise_arg is not None:
            z = self._noise_arg.to(device=self.device, dtype=torch.float64).contiguous()
            if tuple(z.shape) != (T, K, thin, R):
                raise ValueError("CoresetMCMC: _dev_noise must be opt_itrs x chains x thin x (D + 3)")
            return z
        count = K * thin * R
        pairs = (count + 1) // 2
        if 16 * pairs * T > NOISE_BYTES_MAX:
            raise ValueError("CoresetMCMC: the noise of one call (opt_itrs x chains x thin x (D + 3) doubles) exceeds 2 GiB; lower "
                             "opt_itrs and call optimize()")
        self._offset = i0 * pairs
        flat = self._normal(T, 2 * pairs)
        return flat[:, :count].unflatten(1, (K, thin, R))

    def _result(self):
        st = self._run_state
        dg = np.concatenate(st["diag"], axis=0)                                # iterations x chains x thin x 6
        burn = min(self.n_adapt, dg.shape[0])
        kept = dg[burn:] if burn < dg.shape[0] else dg
        flat = lambda a: np.ascontiguousarray(a.transpose(1, 0, 2)).reshape(self.chains, -1)
        out = self.samples()
        return HMCResult(samples=out, accept_rate=kept[..., 1].mean(axis=(0, 2)), step_size=dg[-1, :, -1, 3].copy(),
                         rhat=split_rhat(out) if out.shape[1] >= 4 else np.full(self.D, np.nan), delta_h=flat(dg[burn:, :, :, 0]),
                         accepted=flat(dg[burn:, :, :, 1]) > 0.5, nonfinite_rejected=bool(st["nonfinite"]), center=st["center"],
                         transform=st["transform"], n_adapt=self.n_adapt, kernel="hmc", trace=None)
