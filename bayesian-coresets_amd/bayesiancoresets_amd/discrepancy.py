"""How good a set of posterior draws is, without reducing it to a Gaussian: the two discrepancies the quasi-Newton-coreset and
Coreset-MCMC papers report, both sums over ALL pairs of draws on the device (csrc/pairstat.hip), in float64.

    energy_distance(x, y)       energy^2 = 2 m_xy - m_xx - m_yy,   m_ab = mean over all (i, j) of |a_i - b_j|_2   (i = j included)
    stein_discrepancy(x, g)     ksd^2 = 1/S^2 sum_{i,j} k_p(x_i, x_j), the kernel Stein discrepancy of the IMQ base kernel
                                (c^2 + |x - y|^2)^(-1/2) (Gorham and Mackey, 2017) under the scores g_i = grad log p(x_i):
                                r = x - y, q = c^2 + |r|^2,
                                k_p = D q^(-3/2) - 3 |r|^2 q^(-5/2) - ((g_y - g_x) . r) q^(-3/2) + (g_x . g_y) q^(-1/2)

Both are V-statistics; the Stein result carries the U-statistic besides.  The kernel is Euclidean: ``transform=W, center=mu`` (the
convention of ``HMCResult.transform``, theta = mu + W^T xi) computes both in xi -- without it c = 1 means nothing for a posterior
of width 1 / sqrt(N).  D <= 32, at most 2^20 draws a side, one device, unweighted draws.  There is no CPU fallback."""
import math

import numpy as np

from .laplace_sampler import FAMILIES
from .mcmc import DMAX, log_joint_grad

MAX_DRAWS = 1 << 20           # PS_MAX_ROWS of csrc/pairstat.hip


class EnergyResult(object):
    """``value`` (energy^2 as computed: rounding can leave it a hair below 0), ``distance`` (sqrt(max(value, 0))), ``mean_xy`` /
    ``mean_xx`` / ``mean_yy`` (the three mean distances), ``n_x`` / ``n_y`` (the draws that entered)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class SteinResult(object):
    """``value`` (ksd^2, the V-statistic), ``ksd`` (sqrt(max(value, 0))), ``u_statistic`` (the pairs i != j over S (S - 1); NaN for
    one draw), ``n_draws``."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _root(v):
    """sqrt(max(v, 0)) that keeps a NaN a NaN."""
    return v if v != v else math.sqrt(max(v, 0.0))


def _thinned(torch, x, D, n, max_draws):
    """The (n, D) rows of ``x`` (any leading shape), thinned to rows floor(i n / K), i < K, where ``max_draws`` = K < n."""
    if isinstance(x, torch.Tensor):
        x = x.reshape(-1, D)
        if max_draws is not None and max_draws < n:
            x = x.index_select(0, ((torch.arange(max_draws, dtype=torch.int64) * n) // max_draws).to(x.device))
        return x
    x = x.reshape(-1, D)
    if max_draws is not None and max_draws < n:
        x = x[(np.arange(max_draws, dtype=np.int64) * n) // max_draws]
    return x


def _draws(torch, who, what, x, max_draws, D=None):
    """(rows, n): ``x`` ((S, D) or (chains, draws, D), host array or tensor) as (n, D) rows, thinned; still where it was."""
    if not isinstance(x, torch.Tensor):
        x = np.asarray(x, dtype=np.float64)
    if x.ndim not in (2, 3):
        raise ValueError("%s: %s are (S, D) or (chains, draws, D)" % (who, what))
    d = int(x.shape[-1])
    if d < 1 or d > DMAX:
        raise ValueError("%s: D = %d coordinates (1 <= D <= %d)" % (who, d, DMAX))
    if D is not None and d != D:
        raise ValueError("%s: %s have %d coordinates, the draws %d" % (who, what, d, D))
    n = int(np.prod(x.shape[:-1]))
    if n < 1:
        raise ValueError("%s: no %s" % (who, what))
    if max_draws is not None and int(max_draws) < 1:
        raise ValueError("%s: max_draws = %d" % (who, max_draws))
    kept = n if max_draws is None else min(n, int(max_draws))
    if kept > MAX_DRAWS:
        raise ValueError("%s: %d %s (at most %d a side; see max_draws)" % (who, kept, what, MAX_DRAWS))
    return _thinned(torch, x, d, n, None if max_draws is None else int(max_draws)), kept


def _resident(torch, device, x):
    """(n, D) fp64 on ``device`` with unit column stride and a row stride >= D: a device tensor of that form is used in place."""
    t = x.to(device=device, dtype=torch.float64) if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x)).to(device)
    if t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        t = t.contiguous()
    return t


def _frame(torch, transform, center, D, who):
    """(mu, W, W^-1) on the host for theta = mu + W^T xi; None without a transform."""
    if transform is None:
        if center is not None:
            raise ValueError("%s: center goes with transform" % who)
        return None
    W = np.asarray(transform.detach().cpu() if isinstance(transform, torch.Tensor) else transform, dtype=np.float64)
    mu = np.zeros(D) if center is None else np.asarray(center.detach().cpu() if isinstance(center, torch.Tensor) else center, dtype=np.float64)
    if W.shape != (D, D) or mu.shape != (D,):
        raise ValueError("%s: transform is (D, D) and center (D), D = %d" % (who, D))
    return mu, W, np.linalg.inv(W)                # (D <= 32: on the host)


def _to_frame(torch, device, frame, X, G=None):
    """xi = W^-T (theta - mu) and score_xi = W score_theta, row by row: two small torch operations in front of the kernel."""
    if frame is None:
        return X, G
    mu, W, Winv = (torch.from_numpy(np.ascontiguousarray(v)).to(device) for v in frame)
    return (X - mu) @ Winv, None if G is None else G @ W.T


def _pick_device(torch, device, *inputs):
    for x in inputs:
        if isinstance(x, torch.Tensor) and x.is_cuda:
            return x.device
    return torch.device(device)


def _enqueue(torch, lib, kind, A, GA, B, GB, c, splits, out):
    """One bcx_pair_stat on the current stream into ``out`` (2 doubles on the device); B = None: A against itself."""
    from . import _native
    nA, D = int(A.shape[0]), int(A.shape[1])
    nB = 0 if B is None else int(B.shape[0])
    nbytes = int(lib.bcx_pair_stat_scratch_bytes(nA, nB, D, splits))
    if nbytes < 0:
        raise ValueError("pair statistic: %d x %d draws, D = %d, splits = %d out of range" % (nA, nB or nA, D, splits))
    work = torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device=A.device)
    with torch.cuda.device(A.device):
        _native.check(lib.bcx_pair_stat(_native.stream_ptr(A.device), kind, A.data_ptr(), nA, A.stride(0),
                                        GA.data_ptr() if GA is not None else None, GA.stride(0) if GA is not None else D,
                                        B.data_ptr() if B is not None else None, nB, B.stride(0) if B is not None else D,
                                        GB.data_ptr() if GB is not None else None, GB.stride(0) if GB is not None else D,
                                        D, float(c), splits, out.data_ptr(), work.data_ptr(), work.numel() * 8))


def _pair_stat(kind, A, GA=None, B=None, GB=None, c=1.0, splits=0, device="cuda"):
    """(total, diagonal total) of one bcx_pair_stat call as floats -- the entry point as the tests and tools/discrepancy_bench.py
    drive it: kind 0 distances / 1 Stein terms, (n, D) host arrays or device tensors, B = None: A against itself."""
    import torch
    from . import _native
    if not torch.cuda.is_available():
        raise RuntimeError("the pair statistics need a GPU (there is no CPU fallback)")
    lib = _native.load()
    device = _pick_device(torch, device, A, B)
    A, GA, B, GB = (None if v is None else _resident(torch, device, v if isinstance(v, torch.Tensor) else np.asarray(v, dtype=np.float64))
                    for v in (A, GA, B, GB))
    out = torch.empty(2, dtype=torch.float64, device=device)
    _enqueue(torch, lib, kind, A, GA, B, GB, c, int(splits), out)
    total, diag = out.cpu().tolist()
    return total, diag


def energy_distance(x, y, *, transform=None, center=None, max_draws=None, device="cuda", _dev_splits=0):
    """The energy distance between the draws ``x`` and ``y`` ((S, D) or (chains, draws, D), host arrays or device tensors --
    ``HMCResult.samples`` and ``CoresetMCMC.samples()`` as they are; a device tensor with unit column stride is read in place).
    ``max_draws=K`` keeps rows floor(i S / K), i < K, of each side's flattened draws.  ``transform=W, center=mu``: both sides are
    mapped to xi = W^-T (theta - mu) first.  Non-finite input gives a non-finite ``value``, no exception.  ``_dev_splits`` (a
    development argument): the ranges the tiles of the second operand are cut into, 0 = the library's choice."""
    import torch
    from . import _native
    who = "energy_distance"
    x, nx = _draws(torch, who, "x", x, max_draws)
    D = int(x.shape[1])
    y, ny = _draws(torch, who, "y", y, max_draws, D)
    frame = _frame(torch, transform, center, D, who)
    if not torch.cuda.is_available():
        raise RuntimeError("energy_distance needs a GPU (there is no CPU fallback)")
    lib = _native.load()
    device = _pick_device(torch, device, x, y)
    X, Y = _to_frame(torch, device, frame, _resident(torch, device, x))[0], _to_frame(torch, device, frame, _resident(torch, device, y))[0]
    out = torch.empty(3, 2, dtype=torch.float64, device=device)
    _enqueue(torch, lib, 0, X, None, Y, None, 1.0, int(_dev_splits), out[0])
    _enqueue(torch, lib, 0, X, None, None, None, 1.0, int(_dev_splits), out[1])
    _enqueue(torch, lib, 0, Y, None, None, None, 1.0, int(_dev_splits), out[2])
    sums = out[:, 0].cpu().tolist()                                             # (the one synchronise)
    m_xy, m_xx, m_yy = sums[0] / (float(nx) * ny), sums[1] / (float(nx) * nx), sums[2] / (float(ny) * ny)
    value = 2.0 * m_xy - m_xx - m_yy
    return EnergyResult(value=value, distance=_root(value), mean_xy=m_xy, mean_xx=m_xx, mean_yy=m_yy, n_x=nx, n_y=ny)


def stein_discrepancy(samples, scores=None, *, family=None, pts=None, wts=None, c=1.0, transform=None, center=None, max_draws=None,
                      device="cuda", _dev_splits=0):
    """The IMQ kernel Stein discrepancy of the draws ``samples`` (forms as in ``energy_distance``) under the target whose scores
    grad log p at the draws are either given (``scores``: the draws' leading shape, any target) or computed by
    ``log_joint_grad(family, pts, wts, samples)`` (logistic / Poisson; ``wts=None``: the full data).  ``max_draws`` thins the draws
    (and the given scores alike) before any score is computed.  ``transform=W, center=mu``: xi = W^-T (theta - mu) and score_xi = W
    score_theta, so ``c`` is in units of the frame."""
    import torch
    from . import _native
    who = "stein_discrepancy"
    given = scores is not None
    computed = family is not None or pts is not None
    if given and computed:
        raise ValueError("stein_discrepancy: scores, or family / pts to compute them -- not both")
    if not given and not computed:
        raise ValueError("stein_discrepancy: scores, or family / pts to compute them")
    if computed and (family not in FAMILIES or pts is None):
        raise ValueError("stein_discrepancy: family ('logistic' or 'poisson') and pts compute the scores")
    if not (float(c) > 0.0 and float(c) < float("inf")):
        raise ValueError("stein_discrepancy: c = %r (finite, > 0)" % (c,))
    x, n = _draws(torch, who, "samples", samples, max_draws)
    D = int(x.shape[1])
    if given:
        lead = tuple(samples.shape[:-1]) if hasattr(samples, "shape") else np.shape(samples)[:-1]
        if tuple(np.shape(scores)[:-1]) != tuple(lead):
            raise ValueError("stein_discrepancy: scores of shape %s for samples of shape %s" % (tuple(np.shape(scores)), tuple(np.shape(samples))))
        g, _ = _draws(torch, who, "scores", scores, max_draws, D)
    frame = _frame(torch, transform, center, D, who)
    if not torch.cuda.is_available():
        raise RuntimeError("stein_discrepancy needs a GPU (there is no CPU fallback)")
    lib = _native.load()
    device = _pick_device(torch, device, x, scores if given else pts)
    X = _resident(torch, device, x)
    G = _resident(torch, device, g) if given else log_joint_grad(family, pts, wts, X.contiguous(), device=device)[1]
    X, G = _to_frame(torch, device, frame, X, G)
    out = torch.empty(2, dtype=torch.float64, device=device)
    _enqueue(torch, lib, 1, X, G, None, None, float(c), int(_dev_splits), out)
    total, diag = out.cpu().tolist()                                            # (the one synchronise)
    value = total / (float(n) * n)
    u = (total - diag) / (float(n) * (n - 1)) if n > 1 else float("nan")
    return SteinResult(value=value, ksd=_root(value), u_statistic=u, n_draws=n)
