"""dev: the quasi-Newton coreset (csrc/qn.hip, bc.QuasiNewtonCoreset), two measurements.

    python tools/qnc_bench.py step  [k ...]                  bcx_quasi_newton_step alone at S = 256 (default k = 32 300 1024 4096)
    python tools/qnc_bench.py build [--rows N] [--reps R]    build(300), opt_itrs = 20, on the c5 workload against SparseVI grown to 300
    python tools/qnc_bench.py build --only svi               one leg alone (a copy of this file in a checkout of the parent commit
                                                             times the parent's SparseVI on the same box)

step: device events around `reps` back-to-back calls, five windows after a warm-up window: median and min - max of the windows.
Beside it a model -- 2 k^2 S + k^3 / 3 flops at the 78.6 TFLOP/s fp64 MFMA peak plus the step's launch count -- and, as an outside
baseline, torch.linalg.cholesky + torch.cholesky_solve on the same G + tau I and b (the factorisation and the solves only: the
baseline is handed the matrix the step has to form first).

build: RBF regression, D = 301, S = 256, closed-form column sums (colsum="moments"), the data resident on the device.  The two
algorithms alternate in one process on one data set, each after a warm-up build; wall clock around build() (it ends with a
read-back, which synchronises); median and min - max.  One JSON line per measurement."""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("BCX_DEV", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "bayesian-coresets_amd"), os.path.join(ROOT, "bayesian-coresets_amd", "examples", "common")):
    sys.path.insert(0, p)
import numpy as np

PEAK = 78.6e12
SINGLE_MAX, NB = 128, 32                  # csrc/qn.hip: QN_SINGLE_MAX, QN_NB


def launches(k):
    """Kernel launches of one step (csrc/qn.hip bcx_quasi_newton_step; the Gram is one launch when its blocks need no slices)."""
    if k <= SINGLE_MAX:
        return 4
    n = 3
    for jj in range(0, (k + NB - 1) // NB * NB, NB):
        n += 1 + (2 if k - jj - NB > 0 else 0)
    return n + 1


def stats(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "n": len(xs)}


def bench_step(ks, S=256, tau=1e-2):
    import torch
    from bayesiancoresets_amd import _native as nat
    lib = nat.load()
    st = int(torch.cuda.current_stream().cuda_stream)
    for k in ks:
        g = torch.Generator(device="cuda")
        g.manual_seed(k)
        core = torch.randn(k, S, dtype=torch.float64, device="cuda", generator=g) - 500.0
        col = 20.0 * torch.randn(S, dtype=torch.float64, device="cuda", generator=g)
        w0 = torch.rand(k, dtype=torch.float64, device="cuda", generator=g) + 0.1
        w, d = w0.clone(), torch.zeros(k, dtype=torch.float64, device="cuda")
        sched = torch.zeros(1, dtype=torch.float64, device="cuda")          # gamma = 0: every call sees the same weights
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        need = int(lib.bcx_quasi_newton_scratch_bytes(k, S))
        work = torch.empty(need // 8 + 2, dtype=torch.float64, device="cuda")
        args = [st, k, S, col.data_ptr(), 1.0, core.data_ptr(), S, 1, w.data_ptr(), sched.data_ptr(), 0, tau, d.data_ptr(), None,
                status.data_ptr(), work.data_ptr(), work.numel() * 8]
        reps = 200 if k <= 1024 else 30

        def window(fn, n):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / n

        def step():
            rc = lib.bcx_quasi_newton_step(*args)
            assert rc == 0, lib.bcx_project_last_error()
        window(step, reps)
        ours = stats([window(step, reps) for _ in range(5)])
        assert int(status.item()) == 0
        # the outside baseline on the same system
        V = core - core.mean(dim=1, keepdim=True)
        A = V @ V.T / S + tau * torch.eye(k, dtype=torch.float64, device="cuda")
        b = (V @ (col - w0 @ V) / S)[:, None]

        def vendor():
            torch.cholesky_solve(b, torch.linalg.cholesky(A))
        window(vendor, reps)
        theirs = stats([window(vendor, reps) for _ in range(5)])
        d_ref = torch.cholesky_solve(b, torch.linalg.cholesky(A))[:, 0]
        err = float((d - d_ref).norm() / d_ref.norm())
        flops = 2.0 * k * k * S + k ** 3 / 3.0
        print(json.dumps({"what": "bcx_quasi_newton_step", "k": k, "S": S, "us_per_step": ours, "launches": launches(k),
                          "model_flops": flops, "model_us_at_fp64_mfma_peak": flops / PEAK * 1e6,
                          "torch_cholesky_plus_cholesky_solve_us": theirs, "reps_per_window": reps,
                          "direction_rel_diff_to_torch": err}), flush=True)


def c5_workload(torch, N, seed=1):
    """bench.py --config c5's data: observations generated on the device from one seeded draw, the RBF design rows resident."""
    import rbf_workload
    nb = 50
    D = 6 * nb + 1
    rs = np.random.RandomState(seed)
    pilot = rbf_workload.synthetic_observations(200_000, rs)
    scales, centres = rbf_workload.basis_layout(pilot, nb, rs)
    std, mean = pilot[:, 2].std(), pilot[:, 2].mean()
    g = torch.Generator(device="cuda")
    g.manual_seed(seed * 1_000_003)
    loc = torch.rand(N, 2, dtype=torch.float64, device="cuda", generator=g)
    eps = torch.randn(N, dtype=torch.float64, device="cuda", generator=g)
    price = 5.3 + 0.35 * torch.sin(3.0 * loc[:, 0]) * torch.cos(2.0 * loc[:, 1]) + 0.25 * loc[:, 0] * loc[:, 1] + 0.15 * eps
    Z = rbf_workload.design_rows_device(torch, torch.cat((loc, price[:, None]), dim=1), scales, centres)
    return Z, mean * np.ones(D), (std ** 2 + mean ** 2) * np.eye(D), float(std ** 2)


def bench_build(a):
    import torch
    from bayesiancoresets_amd import _native as nat
    import bayesiancoresets_amd as bc
    import model_linreg
    S, M = 256, a.size
    Z, mu0, Sig0, sigsq = c5_workload(torch, a.rows)
    legs = {}
    if a.only in (None, "qnc"):
        smp = model_linreg.posterior_sampler(mu0, Sig0, sigsq, device="cuda", seed=8)
        legs["qnc"] = bc.QuasiNewtonCoreset(Z, bc.DeviceProjector("linreg", smp, S, sigsq=sigsq, colsum="moments"), opt_itrs=a.opt_itrs)
    if a.only in (None, "svi"):
        smp = model_linreg.posterior_sampler(mu0, Sig0, sigsq, device="cuda", seed=8)
        legs["svi"] = bc.SparseVICoreset(Z, bc.DeviceProjector("linreg", smp, S, sigsq=sigsq, colsum="moments"), opt_itrs=100)
    np.random.seed(1)

    def one(name):
        alg = legs[name]
        alg.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        alg.build(M)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, int(alg.size())
    times, sizes = {n: [] for n in legs}, {}
    for name in legs:                                  # warm-up: the moments, the code objects, every shape of the loop
        one(name)
    for rep in range(a.reps):
        for name in legs:                              # alternating
            t, sizes[name] = one(name)
            times[name].append(t)
    for name in legs:
        print(json.dumps({"what": "build(%d) wall seconds" % M, "alg": name, "rows": a.rows, "D": Z.shape[1] - 1, "S": S,
                          "opt_itrs": a.opt_itrs if name == "qnc" else 100, "colsum": "moments", "seconds": stats(times[name]),
                          "size": sizes[name], "lib": nat.LIB_PATH}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["step", "build"])
    ap.add_argument("ks", nargs="*", type=int)
    ap.add_argument("--rows", type=int, default=5_000_000)
    ap.add_argument("--size", type=int, default=300)
    ap.add_argument("--opt_itrs", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=["qnc", "svi"], default=None)
    a = ap.parse_args()
    if a.mode == "step":
        bench_step(a.ks or [32, 300, 1024, 4096])
    else:
        bench_build(a)
