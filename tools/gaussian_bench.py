"""Dev tool: the Gaussian-mean family on the device.  One JSON line per measurement (medians after
warm-up, pieces between device synchronisations), appended to profiles/gaussian_family.jsonl by the caller:

    python tools/gaussian_bench.py [--proj-n 5000000] [--n 1000000] [--reps 5] >> profiles/gaussian_family.jsonl

  * projection kernel time / TFLOP/s (DeviceProjector.profile) of select and column sums, N x 301 (302 for linreg), S = 256: the
    "gaussian" family beside the "linreg" family in the same run, with the run-to-run spread of each;
  * SparseVI on N x 200, S = 100 at k = 8 / 64 / 300: microseconds per ADAM step of the enqueued loop (GaussianPosteriorSampler +
    closed-form column sums), beside one ADAM step of the callback arrangement (BlackBoxProjector's NumPy projection of the whole
    data set + the host sampler's Cholesky factorisation) -- what this model ran as before the family existed;
  * one BatchPSVI gradient at k = 200 on the same data: column sums, points' projection + gradient kernels, read-back."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bayesian-coresets_amd"))
sys.path.insert(1, os.path.join(ROOT, "bayesian-coresets_amd", "examples", "common"))
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")


def emit(**kw):
    print(json.dumps(kw), flush=True)


def med(v):
    return float(np.median(v))


def projection(bc, torch, N, reps):
    D, S = 301, 256
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    Z = torch.empty((N, D + 1), dtype=torch.float64, device="cuda")
    Z.normal_(generator=g)
    th = 0.1 * np.random.RandomState(2).randn(S, D)
    resid = np.random.RandomState(3).randn(S)
    for fam in ("linreg", "gaussian", "linreg", "gaussian"):
        prj = bc.DeviceProjector(fam, lambda n, w, p: th, S, sigsq=1.0, colsum="mfma")
        pts = Z if fam == "linreg" else Z[:, :D]
        for what in ("select", "colsum"):
            call = (lambda: prj.project_select(pts, resid)) if what == "select" else (lambda: prj.project_colsum(pts))
            call()
            ms = []
            for _ in range(reps):
                prj.profile(True)
                call()
                t, n, fl = prj.profile_read()
                prj.profile(False)
                ms.append(t)
            emit(bench="projection", family=fam, consumer=what, N=N, D=D, S=S, kernel_ms_median=med(ms), kernel_ms_min=min(ms),
                 kernel_ms_max=max(ms), tflops=2.0 * N * D * S / (med(ms) * 1e-3) / 1e12, reps=reps)
    del Z
    torch.cuda.empty_cache()


def sparsevi(bc, torch, N, reps):
    import model_gaussian as mg
    D, S, T = 200, 100, 20
    rs = np.random.RandomState(4)
    x = np.ones(D) + rs.randn(N, D)
    mu0, Sig0inv, Siginv = np.zeros(D), np.eye(D), np.eye(D)
    for k in (8, 64, 300):
        smp = bc.GaussianPosteriorSampler(mu0, Sig0inv, Siginv, seed=1)
        prj = bc.DeviceProjector("gaussian", smp, S)
        alg = bc.SparseVICoreset(x, prj, opt_itrs=T)
        idcs = rs.choice(N, k, replace=False)
        alg.idcs, alg.pts, alg.wts = idcs.astype(np.int64), x[idcs].copy(), np.full(k, N / k)
        us = []
        for r in range(reps + 2):
            w0 = alg.wts.copy()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            alg._optimize()
            torch.cuda.synchronize()
            if r >= 2:
                us.append((time.perf_counter() - t0) / T * 1e6)
            alg.wts = w0
        t0 = time.perf_counter()
        alg._select()
        torch.cuda.synchronize()
        sel_ms = (time.perf_counter() - t0) * 1e3
        emit(bench="sparsevi_adam_step", arrangement="device", N=N, D=D, S=S, k=k, opt_itrs=T, us_per_adam_step_median=med(us),
             us_min=min(us), us_max=max(us), select_ms=sel_ms, moments=prj.moments_info)
    # the callback arrangement: one ADAM step = the host sampler + a NumPy projection of the whole data set (+ the coreset's)
    def sampler_w(n, wts, pts):
        mu, U = mg.weighted_posterior(mu0, Sig0inv, Siginv, pts, wts)
        return mu + np.random.randn(n, D).dot(U.T)
    for k in (8, 300):
        idcs = rs.choice(N, k, replace=False)
        bb = bc.BlackBoxProjector(lambda n, w, p: sampler_w(n, np.full(k, N / k), x[idcs]), S, lambda p, t: mg.log_likelihood(p, t, Siginv, 0.0))
        ts = []
        for r in range(2):
            t0 = time.perf_counter()
            bb.update(None, None)
            col = bb.project(x).sum(axis=0)
            core = bb.project(x[idcs])
            ts.append((time.perf_counter() - t0) * 1e6)
        emit(bench="sparsevi_adam_step", arrangement="callback (host projection + host sampler; engine ingest not included)", N=N, D=D,
             S=S, k=k, us_per_adam_step_median=med(ts), reps=2, checksum=float(col[0] + core[0, 0]))
    return x


def bpsvi(bc, torch, x, reps):
    N, D = x.shape
    S, k = 100, 200
    rs = np.random.RandomState(6)
    smp = bc.GaussianPosteriorSampler(np.zeros(D), np.eye(D), np.eye(D), seed=2)
    prj = bc.DeviceProjector("gaussian", smp, S)
    P, w = x[rs.choice(N, k, replace=False)].copy(), np.full(k, N / k)
    upd, grd = [], []
    for r in range(reps + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        prj.update(w, P)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        prj.psvi_gradient(x, P, w, 1.0)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if r >= 2:
            upd.append((t1 - t0) * 1e6)
            grd.append((t2 - t1) * 1e6)
    emit(bench="bpsvi_step", N=N, D=D, S=S, k=k, sampler_us_median=med(upd), gradient_us_median=med(grd), gradient_us_min=min(grd),
         gradient_us_max=max(grd), moments=prj.moments_info)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--proj-n", type=int, default=5000000)
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip", type=str, default="")
    a = ap.parse_args()
    import torch
    import bayesiancoresets_amd as bc
    head = open(os.path.join(ROOT, "bayesian-coresets_amd", "lib", "HEAD.txt")).read().strip() if os.path.exists(
        os.path.join(ROOT, "bayesian-coresets_amd", "lib", "HEAD.txt")) else "n/a"
    emit(bench="header", device=torch.cuda.get_device_name(0), built_from=head)
    if "projection" not in a.skip:
        projection(bc, torch, a.proj_n, a.reps)
    if "sparsevi" not in a.skip:
        x = sparsevi(bc, torch, a.n, a.reps)
        bpsvi(bc, torch, x, a.reps)


if __name__ == "__main__":
    main()
