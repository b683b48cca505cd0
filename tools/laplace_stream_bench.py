#!/usr/bin/env python3
"""dev: time of the streamed Laplace fit (bc.LaplacePosteriorSampler(stream=True), csrc/laplace_stream.hip) against the path the
same call took before it existed, alternating on one device in one process:

  fits     (k = 1000, D = 10) and (k = 4096, D = 32), both families, cold and warm-started, against the NumPy laplace_fit of
           examples/common (what a harness run falls back to when the points exceed one workgroup's LDS);
  resident (N = 1M, D = 10) on the device rows, against the NumPy fit of the downloaded rows and (logistic) the torch
           laplace_fit on the device rows; the time of ONE more Newton iteration (a pass over the rows + the solve) against the
           model of the pass: N (D + 1) 8 bytes at 8 TB/s;
  adam     SparseVI's weight optimisation at k = 1000 points: the enqueued loop against the host loop with the NumPy sampler;
  frame    DeviceHMC's default frame at N = 1M with device_frame=True against the download + NumPy fit.

    python tools/laplace_stream_bench.py [--rows 1000000 --reps 5 --out results/laplace_stream_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "bayesian-coresets_amd"))
sys.path.insert(0, os.path.join(ROOT, "bayesian-coresets_amd", "examples", "common"))
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

HBM_BYTES_PER_S = 8.0e12


def med(v):
    return float(np.median(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--adam-rows", type=int, default=100_000)
    ap.add_argument("--adam-steps", type=int, default=10)
    ap.add_argument("--skip", default="", help="comma-separated sections to leave out: fits, resident, adam, frame")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    skip = set(filter(None, a.skip.split(",")))
    import torch
    import bayesiancoresets_amd as bc
    from bayesiancoresets_amd import _native
    from bayesiancoresets_amd.laplace_sampler import _LaplacePlan
    import model_lr
    import model_poiss
    if not torch.cuda.is_available():
        raise SystemExit("laplace_stream_bench needs a GPU: a timing from anywhere else says nothing")
    mods = {"logistic": model_lr, "poisson": model_poiss}
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps}
    sync = torch.cuda.synchronize

    def timed(fn):
        sync()
        t0 = time.perf_counter()
        r = fn()
        sync()
        return time.perf_counter() - t0, r

    def make_plan(smp, pts_dev, S):
        plan = _LaplacePlan(smp, S, pts_dev, smp._noise_block(2, S))
        return plan

    def fit_round(plan, w_dev, inner):
        """(cold s, warm s, Newton steps cold, warm) per fit: `inner` enqueued fits per timed window, one synchronise each.
        Step 0 of a plan starts at zero, step 1 at the mode the fit before it left; the warm fits alternate between the weights
        and a copy moved by up to 2 % (consecutive ADAM steps), so each of them has a step to take."""
        smp = plan.s
        if getattr(plan, "_alt", None) is None or plan._alt.shape != w_dev.shape:
            plan._alt = w_dev * (1.0 + 0.02 * torch.rand(w_dev.shape, dtype=torch.float64, device=w_dev.device))
        cold = timed(lambda: [plan.draw(w_dev, 0) for _ in range(inner)])[0] / inner
        steps_cold = int(smp._status.cpu()[1])
        warm = timed(lambda: [plan.draw(plan._alt if j % 2 == 0 else w_dev, 1) for j in range(inner)])[0] / inner
        steps_warm = int(smp._status.cpu()[1])
        return cold, warm, steps_cold, steps_warm

    def fits():
        out["fits"] = []
        for family in ("logistic", "poisson"):
            for k, D in ((1000, 10), (4096, 32)):
                rs = np.random.RandomState(k + D)
                pts = mods[family].synthetic_rows(k, D, rs)
                wts = np.abs(rs.randn(k)) * 3.0
                smp = bc.LaplacePosteriorSampler(family, D, seed=1, stream=True)
                pts_dev, w_dev = torch.from_numpy(pts).cuda(), torch.from_numpy(wts).cuda()
                plan = make_plan(smp, pts_dev, a.samples)
                fit_round(plan, w_dev, 2)                                 # warm-up
                host, rounds = [], []
                for _ in range(a.reps):                                   # alternating: host fit, device fits
                    host.append(timed(lambda: mods[family].laplace_fit(pts, wts))[0])
                    rounds.append(fit_round(plan, w_dev, 10))
                plan.check()
                mu_ref, _ = mods[family].laplace_fit(pts, wts)
                err = float(np.abs(smp._mu.cpu().numpy() - mu_ref).max())
                out["fits"].append({"family": family, "k": k, "D": D, "S": a.samples, "stream_cold_us": med([r[0] for r in rounds]) * 1e6,
                                    "stream_warm_us": med([r[1] for r in rounds]) * 1e6, "newton_steps_cold": rounds[-1][2],
                                    "newton_steps_warm": rounds[-1][3], "numpy_fit_us": med(host) * 1e6, "mode_max_abs_diff": err})
                print(json.dumps(out["fits"][-1]), flush=True)

    Zs = {}
    if "resident" not in skip or "frame" not in skip:
        for family in ("logistic", "poisson"):
            Zs[family] = mods[family].synthetic_rows(a.rows, 10, np.random.RandomState(5))

    def resident():
        out["resident"] = []
        for family in ("logistic", "poisson"):
            N, D = a.rows, 10
            Z = Zs[family]
            Zd = torch.from_numpy(Z).cuda()
            ones = torch.ones(N, dtype=torch.float64, device="cuda")
            smp = bc.LaplacePosteriorSampler(family, D, seed=1, stream=True)
            plan = make_plan(smp, Zd, a.samples)
            fit_round(plan, ones, 1)
            rounds = [fit_round(plan, ones, 3) for _ in range(a.reps)]
            plan.check()
            cold, warm, sc, sw = med([r[0] for r in rounds]), med([r[1] for r in rounds]), rounds[-1][2], rounds[-1][3]
            post, numpy_fit, torch_fit = [], [], []
            for _ in range(max(2, a.reps // 2)):
                post.append(timed(lambda: smp.posterior(None, Zd))[0])
                numpy_fit.append(timed(lambda: mods[family].laplace_fit(Zd.cpu().numpy(), None))[0])
                if family == "logistic":
                    torch_fit.append(timed(lambda: model_lr.laplace_fit(Zd))[0])
            mu_ref, _ = mods[family].laplace_fit(Z, None)
            mu, _ = smp.posterior(None, Zd)
            # one more Newton iteration = one pass over the rows + one solve: fits cut off after 1 and 3 iterations, cold
            per_iter = []
            for _ in range(a.reps):
                ts = []
                for it in (1, 3):
                    cut = bc.LaplacePosteriorSampler(family, D, seed=1, stream=True, max_iter=it)
                    cplan = _LaplacePlan(cut, a.samples, Zd, cut._noise_block(1, a.samples))
                    cplan.draw(ones, 0)
                    ts.append(timed(lambda: [cplan.draw(ones, 0) for _ in range(3)])[0] / 3)
                per_iter.append((ts[1] - ts[0]) / 2)
            model = N * (D + (family == "poisson")) * 8 / HBM_BYTES_PER_S
            out["resident"].append({"family": family, "N": N, "D": D, "stream_cold_us": cold * 1e6, "stream_warm_us": warm * 1e6,
                                    "newton_steps_cold": sc, "newton_steps_warm": sw, "posterior_call_us": med(post) * 1e6,
                                    "download_plus_numpy_fit_us": med(numpy_fit) * 1e6,
                                    "torch_fit_us": med(torch_fit) * 1e6 if torch_fit else None,
                                    "iteration_us": med(per_iter) * 1e6, "pass_model_us": model * 1e6,
                                    "model_over_measured_iteration": model / med(per_iter),
                                    "mode_max_abs_diff": float(np.abs(mu - mu_ref).max())})
            print(json.dumps(out["resident"][-1]), flush=True)
            del Zd, ones

    def adam():
        family, D, k, T, S, N = "logistic", 10, 1000, a.adam_steps, a.samples, a.adam_rows
        Z = model_lr.synthetic_rows(N, D, np.random.RandomState(7))

        def host_sampler(n, wts, pts):
            if wts is None or pts is None or np.asarray(pts).shape[0] == 0 or not (np.asarray(wts) > 0).any():
                return np.random.randn(n, D)
            keep = np.asarray(wts) > 0
            mu, Sig = model_lr.laplace_fit(np.atleast_2d(pts)[keep], np.asarray(wts)[keep])
            return np.atleast_2d(np.random.multivariate_normal(mu, Sig, n))

        def make(sampler, enqueue):
            np.random.seed(3)
            alg = bc.SparseVICoreset(Z, bc.DeviceProjector(family, sampler, S), opt_itrs=T)
            alg.ENQUEUE = enqueue
            idcs = np.random.RandomState(9).choice(N, k, replace=False)
            alg.idcs, alg.pts, alg.wts = idcs.astype(np.int64), Z[idcs].copy(), np.full(k, float(N) / k)
            return alg
        variants = {"enqueued_stream": make(bc.LaplacePosteriorSampler(family, D, seed=2, stream=True), True),
                    "host_loop_numpy_sampler": make(host_sampler, False)}
        assert variants["enqueued_stream"]._enqueue_plan() is not None
        times = {n: [] for n in variants}
        for r in range(a.reps + 1):
            for n, alg in variants.items():
                w0 = alg.wts.copy()
                dt = timed(alg._optimize)[0]
                alg.wts = w0
                if r:
                    times[n].append(dt / T)
        out["adam"] = {"family": family, "N": N, "D": D, "k": k, "S": S, "opt_itrs": T,
                       **{n + "_us_per_step": med(v) * 1e6 for n, v in times.items()}}
        print(json.dumps(out["adam"]), flush=True)

    def frame():
        family, D = "logistic", 10
        Zd = torch.from_numpy(Zs[family]).cuda()
        hmcs = {"device_frame": bc.DeviceHMC(family, D, chains=8, seed=1, device_frame=True),
                "download_plus_numpy_fit": bc.DeviceHMC(family, D, chains=8, seed=1)}
        times = {n: [] for n in hmcs}
        for r in range(max(2, a.reps // 2) + 1):
            for n, h in hmcs.items():
                dt = timed(lambda: h._default_frame(a.rows, Zd, None, Zd, None))[0]
                if r:
                    times[n].append(dt)
        out["frame"] = {"family": family, "N": a.rows, "D": D, **{n + "_us": med(v) * 1e6 for n, v in times.items()}}
        print(json.dumps(out["frame"]), flush=True)

    for name, fn in (("fits", fits), ("resident", resident), ("adam", adam), ("frame", frame)):
        if name in skip:
            continue
        try:
            fn()
        except (ValueError, AssertionError, AttributeError, TypeError, KeyError, IndexError, _native.EngineError) as e:
            # (a host-side mistake in one section keeps the others' numbers; anything from the device runtime ends the run)
            out[name + "_error"] = "%s: %s" % (type(e).__name__, e)
            print(out[name + "_error"], flush=True)
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
