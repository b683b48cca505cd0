"""dev: Coreset MCMC (csrc/hmc.hip cmc_advance_kernel, bc.CoresetMCMC) against the two enqueued weight loops it
succeeds, on one synthetic logistic data set resident on the device.

    python tools/cmc_bench.py [--rows N] [--dim D] [--sub n] [--itrs T] [--reps R] [--sizes M ...] [--chains K ...] [--only cmc]

Per (M, K): wall clock around ``optimize()`` of T iterations (it ends with the one read-back, which synchronises) after a
``build`` that warmed every shape up -- iterations / s and us per iteration; device events around back-to-back calls of
``bcx_cmc_advance`` alone (its memset, cmc_advance_kernel, cmc_centre_kernel) and of ``bcx_sparsevi_adam_step_ws`` alone at the
same shapes -- us per call; the launches of one iteration.  The split of the first figure between its two kernels is read from a
kernel trace of this script (``rocprofv3 --kernel-trace --stats -- python tools/cmc_bench.py --only cmc ...``).  Beside them the us
per step of ``QuasiNewtonCoreset``'s and ``SparseVICoreset``'s enqueued loops (``subsample="device"``, bc.LaplacePosteriorSampler)
on the same M points with S = K draws and the same n_sub rows per step.  Median and min - max of the repetitions; one JSON line
per (M, K)."""
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


def stats(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 3), "min": round(xs[0], 3), "max": round(xs[-1], 3), "n": len(xs)}


def data(torch, N, D, seed=1):
    """Rows y x of a logistic model with a unit-scale linear predictor, generated on the device."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    X = torch.randn(N, D, dtype=torch.float64, device="cuda", generator=g)
    X[:, -1] = 1.0
    th = torch.ones(D, dtype=torch.float64, device="cuda") / np.sqrt(D)
    y = torch.where(torch.rand(N, dtype=torch.float64, device="cuda", generator=g) < torch.sigmoid(X @ th), 1.0, -1.0)
    return (y[:, None] * X).contiguous()


def wall(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def window(torch, fn, n):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def bench_cmc(torch, bc, lib, Z, M, K, a):
    N, D = Z.shape
    np.random.seed(1)
    alg = bc.CoresetMCMC(Z, "logistic", chains=K, leapfrog=a.leapfrog, thin=a.thin, opt_itrs=a.itrs, n_subsample=a.sub, seed=1)
    alg.build(M)                                      # the warm-up: the frame's fit, the code objects, the adaptation
    secs = [wall(torch, alg.optimize) for _ in range(a.reps)]
    out = {"iterations_per_s": stats([a.itrs / s for s in secs]), "us_per_iteration": stats([s / a.itrs * 1e6 for s in secs]),
           "accept_rate": round(float(alg.result.accept_rate.mean()), 3), "step_size": round(float(alg.result.step_size.mean()), 4)}
    # the two calls of an iteration alone, at the run's own state
    st = alg._run_state
    f64 = dict(dtype=torch.float64, device="cuda")
    head = st["head"]
    w, status, m1, m2 = head[:M], head[M:M + 1], head[M + 1:2 * M + 1], head[2 * M + 1:]
    noise = torch.randn(K, a.thin, D + 3, **f64)
    table = torch.randint(N, (a.sub,), dtype=torch.int64, device="cuda")
    V, s = torch.empty(M, K, **f64), torch.empty(K, **f64)
    samples, diag = torch.empty(K, a.thin, alg.ld, **f64), torch.empty(K, a.thin, 6, **f64)
    sched = torch.tensor([0.0, 1.0, 1.0], **f64)     # gamma = 0: every call sees the same weights
    work = torch.empty(max(int(lib.bcx_sparsevi_adam_scratch_bytes(M, K)) // 8, 1), **f64)
    stream = int(torch.cuda.current_stream().cuda_stream)
    pts = st["pts"]
    first = st["iteration"] * a.thin

    def advance():
        rc = lib.bcx_cmc_advance(stream, 0, M, D, w.data_ptr(), pts.data_ptr(), pts.stride(0), st["mu"].data_ptr(), st["W"].data_ptr(), D, K,
                                 a.thin, a.leapfrog, 0.5, first, 0, 0, noise.data_ptr(), st["chains"].data_ptr(), Z.data_ptr(), N, Z.stride(0),
                                 table.data_ptr(), a.sub, V.data_ptr(), K, s.data_ptr(), alg.ld, samples.data_ptr(), None, None, diag.data_ptr(),
                                 status.data_ptr())
        assert rc == 0, lib.bcx_project_last_error()

    def adam():
        rc = lib.bcx_sparsevi_adam_step_ws(stream, M, K, s.data_ptr(), N / a.sub, V.data_ptr(), K, w.data_ptr(), m1.data_ptr(), m2.data_ptr(),
                                           sched.data_ptr(), 0, 0.9, 0.999, 1e-8, None, 1, work.data_ptr(), work.numel() * 8)
        assert rc == 0, lib.bcx_project_last_error()
    for name, fn in (("advance_and_centre", advance), ("adam_step", adam)):
        window(torch, fn, 50)
        out["us_per_call_" + name] = stats([window(torch, fn, 200) for _ in range(5)])
    out["launches_per_iteration"] = {"memset": 1, "cmc_advance_kernel": 1, "cmc_centre_kernel": 1, "adam_step_kernels": 1 if M <= 16 else 2}
    out["target_evaluations_per_launch"] = 1 + a.thin * a.leapfrog
    return out, alg


def bench_loops(torch, bc, Z, M, K, a, pts, idcs):
    """us per step of the two enqueued loops on the same points: optimize() of T steps after a warm-up."""
    N, D = Z.shape
    out = {}
    for name in ("qnc", "svi"):
        smp = bc.LaplacePosteriorSampler("logistic", D, seed=1, stream=True)
        prj = bc.DeviceProjector("logistic", smp, K)
        kw = dict(n_subsample_opt=a.sub, opt_itrs=a.itrs, subsample="device")
        alg = bc.QuasiNewtonCoreset(Z, prj, **kw) if name == "qnc" else bc.SparseVICoreset(Z, prj, step_sched=lambda i: 1.0 / (1.0 + i), **kw)
        alg.pts, alg.idcs, alg.wts = pts.copy(), idcs.copy(), N / M * np.ones(M)
        enq = alg._enqueue_plan_subsampled() is not None

        def run():
            alg.wts = N / M * np.ones(M)
            alg._optimize()
        np.random.seed(1)
        run()
        secs = [wall(torch, run) for _ in range(a.reps)]
        out[name + "_us_per_step"] = stats([s / a.itrs * 1e6 for s in secs])
        out[name + "_enqueued"] = bool(enq)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=10)
    ap.add_argument("--sub", type=int, default=1000)
    ap.add_argument("--itrs", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--thin", type=int, default=1)
    ap.add_argument("--leapfrog", type=int, default=8)
    ap.add_argument("--sizes", type=int, nargs="*", default=[32, 256, 1024])
    ap.add_argument("--chains", type=int, nargs="*", default=[64, 256])
    ap.add_argument("--only", choices=["cmc"], default=None)
    a = ap.parse_args()
    import torch
    import bayesiancoresets_amd as bc
    from bayesiancoresets_amd import _native as nat
    lib = nat.load()
    Z = data(torch, a.rows, a.dim)
    for M in a.sizes:
        for K in a.chains:
            rec = {"what": "Coreset MCMC iteration", "M": M, "K": K, "D": a.dim, "rows": a.rows, "n_sub": a.sub, "thin": a.thin,
                   "leapfrog": a.leapfrog, "itrs": a.itrs}
            cmc, alg = bench_cmc(torch, bc, lib, Z, M, K, a)
            rec.update(cmc)
            if a.only is None:
                rec.update(bench_loops(torch, bc, Z, M, K, a, alg.pts, alg.idcs))
            print(json.dumps(rec), flush=True)
