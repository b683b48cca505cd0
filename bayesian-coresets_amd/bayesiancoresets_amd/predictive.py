"""Held-out log predictive density on the device: what the draws of a coreset's posterior are worth on rows the coreset never
saw.  For a test row z_n and draws theta_1 .. theta_S

    lppd[n] = log( 1/S sum_s p(z_n | theta_s) ) = logsumexp_s ll(z_n, theta_s) - log S,     mean_ll[n] = 1/S sum_s ll(z_n, theta_s)

with ll the reference's full log-likelihood (examples/common/model_lr.py:25-32; model_poiss.py:25-38, -log y! included).
``log_predictive(family, pts, samples)`` is one pass over the rows (csrc/predict.hip): products on the fp64
matrix pipe, likelihood and an online log-sum-exp over the draws in registers; the N x S table is never stored.  Logistic and
Poisson only, D <= 32, one device, unweighted draws.  There is no CPU fallback."""
import numpy as np

from .laplace_sampler import FAMILIES
from .mcmc import DMAX, _device_rows


class PredictiveResult(object):
    """``lppd`` (N) and ``mean_ll`` (N): ndarrays, or device tensors when ``pts`` was a device tensor; ``elpd`` (the sum of
    ``lppd``, a float); ``n_draws`` (S)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def log_predictive(family, pts, samples, device="cuda", *, _dev_splits=0):
    """The log predictive density of the rows ``pts`` (logistic: y x; Poisson: [x, y]; host array or device tensor, a strided
    device tensor is read in place) under the draws ``samples`` ((S, D) or (chains, draws, D), host array or device tensor --
    ``HMCResult.samples`` as it is).  A non-finite value in a row makes that row's outputs NaN, one in a draw every row's.
    ``_dev_splits`` (a development argument): the number of ranges the draws are cut into, 0 = the library's choice."""
    import torch
    from . import _native
    if family not in FAMILIES:
        raise ValueError("family must be 'logistic' or 'poisson'")
    if not torch.cuda.is_available():
        raise RuntimeError("log_predictive needs a GPU (there is no CPU fallback)")
    lib = _native.load()
    as_tensor = isinstance(pts, torch.Tensor)
    if as_tensor and pts.is_cuda:
        device = pts.device
    elif isinstance(samples, torch.Tensor) and samples.is_cuda:
        device = samples.device
    device = torch.device(device)
    th = samples.to(device=device, dtype=torch.float64) if isinstance(samples, torch.Tensor) else \
        torch.from_numpy(np.ascontiguousarray(np.asarray(samples, dtype=np.float64))).to(device)
    if th.dim() not in (2, 3):
        raise ValueError("log_predictive: samples are (S, D) or (chains, draws, D)")
    D = int(th.shape[-1])
    if D < 1 or D > DMAX:
        raise ValueError("log_predictive: D = %d parameters (1 <= D <= %d)" % (D, DMAX))
    th = th.reshape(-1, D).contiguous()
    S = int(th.shape[0])
    if S < 1:
        raise ValueError("log_predictive: no draws")
    splits = int(_dev_splits)
    cols = D + (1 if family == "poisson" else 0)
    N = 0 if pts is None else len(pts)
    lppd = torch.empty(N, dtype=torch.float64, device=device)
    mean = torch.empty(N, dtype=torch.float64, device=device)
    if N:
        Z = _device_rows(torch, device, pts, cols, "points")
        nbytes = int(lib.bcx_log_predictive_scratch_bytes(N, D, S, splits))
        work = torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device=device)
        with torch.cuda.device(device):
            _native.check(lib.bcx_log_predictive(_native.stream_ptr(device), FAMILIES[family], Z.data_ptr(), N, Z.stride(0), D, th.data_ptr(),
                                                 S, D, splits, lppd.data_ptr(), mean.data_ptr(), work.data_ptr(), work.numel() * 8))
    elif pts is not None and np.ndim(pts) == 2 and np.shape(pts)[1] != cols:
        raise ValueError("points have %d columns, the model takes %d" % (np.shape(pts)[1], cols))
    elpd = float(lppd.sum().item()) if N else 0.0
    if not as_tensor:
        lppd, mean = lppd.cpu().numpy(), mean.cpu().numpy()
    return PredictiveResult(lppd=lppd, mean_ll=mean, elpd=elpd, n_draws=S)
