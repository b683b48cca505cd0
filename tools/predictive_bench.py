"""Dev tool: time of bc.log_predictive (csrc/predict.hip) per call and in (row, draw) pairs per second at
N = 100 000 held-out rows and S = 64 000 draws, D = 10 and D = 32, logistic and Poisson, the inputs resident on the device --
beside two baselines that are not the code under test:

* the same quantity by chunked torch fp64 on the same device: `Z @ Theta^T` per chunk of draws, the likelihood elementwise,
  `torch.logsumexp` per chunk and over the chunks' results;
* NumPy on the host (tests/predictive_restatement.py in float64) at a size scaled down to a few seconds.

Every timed window is warmed up by one untimed call of the same shape, ends in a device synchronise and is repeated; the line
carries the median and the extremes of the repeats, the share of the model of DESIGN.md 4.19 -- pairs x OPS_PER_PAIR fp64 VALU
lane-operations on 256 CUs x 4 SIMDs x 16 fp64 lanes per clock at 2.4 GHz, plus the product's 2 x (D padded to 4) flops per pair at
the fp64 MFMA peak, which shares the datapath (csrc/proj_math.h) -- and the largest difference between the kernel's and the torch
baseline's outputs.  One JSON line.

    python tools/predictive_bench.py [--quick]
"""
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "bayesian-coresets_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import predictive_restatement as restate  # noqa: E402

VALU_RATE = 256 * 4 * 16 * 2.4e9          # fp64 lane-operations per second
MFMA_RATE = 78.6e12                       # fp64 MFMA flops per second
OPS_PER_PAIR = {"logistic": 45.5, "poisson": 60.5}   # fp64 VALU instructions per value in the compiled loop


def inputs(family, N, S, D, rs):
    t0 = rs.randn(D) / np.sqrt(D)
    X = np.hstack((rs.randn(N, D - 1), np.ones((N, 1))))
    th = t0 + 0.3 * rs.randn(S, D) / np.sqrt(D)
    if family == "logistic":
        y = np.where(rs.rand(N) < 1 / (1 + np.exp(-X.dot(t0))), 1.0, -1.0)
        return y[:, None] * X, th
    y = rs.poisson(np.log1p(np.exp(X.dot(t0)))).astype(np.float64)
    return np.hstack((X, y[:, None])), th


def torch_chunked(torch, family, Z, th, chunk):
    """lppd and mean_ll by plain torch fp64: the table of one chunk of draws at a time."""
    S = th.shape[0]
    lses, sums = [], []
    if family == "poisson":
        X, y = Z[:, :-1], Z[:, -1:]
        lg = torch.lgamma(y + 1.0)
    for c0 in range(0, S, chunk):
        t = th[c0:c0 + chunk]
        if family == "logistic":
            m = -(Z @ t.T)
            ll = torch.where(m < 100.0, -torch.log1p(torch.exp(m)), -m)
        else:
            s = X @ t.T
            rate = torch.clamp(s, min=0.0) + torch.log1p(torch.exp(-torch.abs(s)))
            ll = y * torch.where(s > -100.0, torch.log(rate), s) - rate - lg
        lses.append(torch.logsumexp(ll, dim=1))
        sums.append(ll.sum(dim=1))
    return torch.logsumexp(torch.stack(lses), dim=0) - math.log(S), torch.stack(sums).sum(dim=0) / S


def timed(torch, fn, reps):
    fn()                                                                        # (first-use costs, this shape)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return dict(median_ms=float(np.median(ts)) * 1e3, min_ms=min(ts) * 1e3, max_ms=max(ts) * 1e3, reps=reps)


def main():
    import torch
    import bayesiancoresets_amd as bc
    if not torch.cuda.is_available():
        raise RuntimeError("predictive_bench needs a GPU")
    quick = "--quick" in sys.argv
    N, S = (20000, 8000) if quick else (100000, 64000)
    chunk = 1000
    rs = np.random.RandomState(0)
    cases = []
    for family in ("logistic", "poisson"):
        for D in (10, 32):
            Zh, thh = inputs(family, N, S, D, rs)
            Z, th = torch.from_numpy(Zh).cuda(), torch.from_numpy(thh).cuda()
            pairs = float(N) * S
            res = bc.log_predictive(family, Z, th)
            ref_lppd, ref_mean = torch_chunked(torch, family, Z, th, chunk)
            diff = float(((res.lppd - ref_lppd).abs() / ref_lppd.abs().clamp(min=1.0)).max())
            diff_mean = float(((res.mean_ll - ref_mean).abs() / ref_mean.abs().clamp(min=1.0)).max())
            kern = timed(torch, lambda: bc.log_predictive(family, Z, th), 10)
            base = timed(torch, lambda: torch_chunked(torch, family, Z, th, chunk), 3)
            model_ms = pairs * (OPS_PER_PAIR[family] / VALU_RATE + 2.0 * ((D + 3) // 4 * 4) / MFMA_RATE) * 1e3
            cases.append(dict(family=family, N=N, S=S, D=D, kernel=kern, pairs_per_second=pairs / (kern["median_ms"] * 1e-3),
                              model_ms=model_ms, fraction_of_model=model_ms / kern["median_ms"],
                              torch_chunked=dict(base, chunk=chunk, pairs_per_second=pairs / (base["median_ms"] * 1e-3)),
                              torch_over_kernel=base["median_ms"] / kern["median_ms"],
                              lppd_max_rel_diff_to_torch=diff, mean_ll_max_rel_diff_to_torch=diff_mean))
            del Z, th, res, ref_lppd, ref_mean
            torch.cuda.empty_cache()
    host = []
    Nh, Sh = (1000, 1000) if quick else (20000, 6400)
    for family in ("logistic", "poisson"):
        Zh, thh = inputs(family, Nh, Sh, 10, rs)
        restate.log_predictive(family, Zh[:100], thh[:100], np.float64)
        t0 = time.perf_counter()
        restate.log_predictive(family, Zh, thh, np.float64)
        dt = time.perf_counter() - t0
        host.append(dict(family=family, N=Nh, S=Sh, D=10, seconds=dt, pairs_per_second=Nh * Sh / dt))
    print(json.dumps(dict(tool="predictive_bench", device=torch.cuda.get_device_name(0), cases=cases, numpy_host=host)), flush=True)


if __name__ == "__main__":
    main()
