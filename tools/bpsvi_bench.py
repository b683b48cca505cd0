#!/usr/bin/env python3
"""BatchPSVI on the device (coreset/bpsvi.py, csrc/psvi.hip): milliseconds per ADAM step, split into
  sampler    projector.update(w, P): the device sampler's draws at the current weights and points;
  colsum     the data's column sums (closed form or fused projection), inside psvi_gradient;
  gradient   the rest of psvi_gradient: projection of the pseudo-points, the fused pseudo-point gradient, the read-back;
  host       what remains of the step: host ADAM (util/opt.py), the weight upload, Python.
Every piece is timed between device synchronisations, so the sum is the step with the pieces serialised.
Shapes:
  i    linreg   N = 5M, D = 301, S = 256, k = 300, LinregPosteriorSampler, colsum "auto"
  ii   logistic N = 1M, D = 10,  S = 512, k = 100, LaplacePosteriorSampler
  iii  the fused gradient entry alone (bcx_psvi_gradient) at k = 1024, S = 1024, D = 512: 4 k S D flops over its time
--loop (shapes i, ii): "host" times the host loop as above (BatchPSVICoreset.ENQUEUE = False); "enqueued" the device-resident loop
(coreset/bpsvi.py _optimize_enqueued) -- nothing synchronises inside it, so a step is the distance between two events recorded on
the stream after consecutive draws, and the wall time of the whole loop over its steps is given next to it; "both" (default)
alternates host, enqueued, host, enqueued in one process on the same data and reports every run ("host_runs" / "enqueued_runs";
the line's own step_ms ... are the first host run's).
Prints one JSON line per shape (and writes them to --out).
    python tools/bpsvi_bench.py [--shape all|i|ii|iii] [--loop both|host|enqueued] [--steps 20] [--warmup 5] [--out profiles/bpsvi_bench.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "bayesian-coresets_amd"))

PEAK_FP64_MFMA = 78.6e12      # MI355X, v_mfma_f64_16x16x4_f64


def step_breakdown(torch, bc, family, Z, smp, S, k, steps, warmup, sigsq=1.0, colsum="auto"):
    prj = bc.DeviceProjector(family, smp, S, sigsq=sigsq, colsum=colsum)
    marks, parts = [], []

    def timed(fn, key):
        def f(*a, **kw):
            torch.cuda.synchronize()
            t = time.perf_counter()
            if key == "sampler":
                marks.append(t)
                parts.append({"sampler": 0.0, "colsum": 0.0, "psvi": 0.0})
            r = fn(*a, **kw)
            torch.cuda.synchronize()
            parts[-1][key] += time.perf_counter() - t
            return r
        return f
    prj.update = timed(prj.update, "sampler")
    prj._colsum_projected = timed(prj._colsum_projected, "colsum")
    prj._colsum_from_moments = timed(prj._colsum_from_moments, "colsum")
    prj.psvi_gradient = timed(prj.psvi_gradient, "psvi")
    np.random.seed(1)
    alg = bc.BatchPSVICoreset(Z, prj, warmup + steps, step_sched=lambda i: 0.1 / (1.0 + i))
    alg.ENQUEUE = False
    marks.clear(); parts.clear()                       # (the projector's first draw at construction)
    t0 = time.perf_counter()
    alg.build(k)
    torch.cuda.synchronize()
    marks.append(time.perf_counter())
    rows = []
    for i in range(warmup, warmup + steps):
        wall = marks[i + 1] - marks[i]
        p = parts[i]
        rows.append((wall, p["sampler"], p["colsum"], p["psvi"] - p["colsum"], wall - p["sampler"] - p["psvi"]))
    a = np.array(rows) * 1e3
    med = np.median(a, axis=0)
    return {"step_ms": float(med[0]), "sampler_ms": float(med[1]), "colsum_ms": float(med[2]), "gradient_ms": float(med[3]),
            "host_ms": float(med[4]), "step_ms_min": float(a[:, 0].min()), "step_ms_max": float(a[:, 0].max()),
            "build_s": time.perf_counter() - t0, "moments": prj.moments_info, "finite": bool(np.isfinite(alg.pts).all())}


class _StampedPlan(object):
    """A moving-points plan whose draws leave an event on the stream (no synchronisation)."""

    def __init__(self, torch, plan):
        self._torch, self._plan, self.events = torch, plan, []

    def __getattr__(self, name):
        return getattr(self._plan, name)

    def draw(self, w_dev, i):
        e = self._torch.cuda.Event(enable_timing=True)
        e.record()
        self.events.append(e)
        return self._plan.draw(w_dev, i)


def enqueued_steps(torch, bc, family, Z, smp, S, k, steps, warmup, sigsq=1.0, colsum="auto"):
    prj = bc.DeviceProjector(family, smp, S, sigsq=sigsq, colsum=colsum)
    np.random.seed(1)
    alg = bc.BatchPSVICoreset(Z, prj, warmup + steps + 1, step_sched=lambda i: 0.1 / (1.0 + i))
    keep, inner = {}, alg._enqueue_plan

    def wrapped():
        plan = inner()
        if plan is None:
            raise SystemExit("bpsvi_bench: the enqueued loop does not serve this shape")
        keep["plan"] = _StampedPlan(torch, plan)
        return keep["plan"]
    alg._enqueue_plan = wrapped
    wall = {}
    opt = alg._optimize_enqueued

    def timed(plan):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = opt(plan)
        torch.cuda.synchronize()
        wall["s"] = time.perf_counter() - t
        return r
    alg._optimize_enqueued = timed
    t0 = time.perf_counter()
    alg.build(k)
    torch.cuda.synchronize()
    ev = keep["plan"].events
    a = np.array([ev[i].elapsed_time(ev[i + 1]) for i in range(warmup, warmup + steps)])
    return {"step_ms": float(np.median(a)), "step_ms_min": float(a.min()), "step_ms_max": float(a.max()),
            "loop_wall_ms_per_step": wall["s"] * 1e3 / (warmup + steps + 1), "build_s": time.perf_counter() - t0,
            "moments": dict(prj.moments_info), "finite": bool(np.isfinite(alg.pts).all())}


def both_loops(torch, bc, loop, family, Z, make, S, k, steps, warmup):
    """host / enqueued alternating, twice each (``loop`` = "both"), or one kind twice."""
    runs = {"host": [], "enqueued": []}
    for _ in range(2):
        if loop in ("both", "host"):
            runs["host"].append(step_breakdown(torch, bc, family, Z, make(), S, k, steps, warmup))
        if loop in ("both", "enqueued"):
            runs["enqueued"].append(enqueued_steps(torch, bc, family, Z, make(), S, k, steps, warmup))
    r = dict(runs["host"][0]) if runs["host"] else {}
    r["loop"] = loop
    if runs["host"]:
        r["host_runs"] = runs["host"]
        r["host_step_ms"] = [x["step_ms"] for x in runs["host"]]
    if runs["enqueued"]:
        r["enqueued_runs"] = runs["enqueued"]
        r["enqueued_step_ms"] = [x["step_ms"] for x in runs["enqueued"]]
    return r


def shape_i(torch, bc, steps, warmup, loop="both"):
    N, D, S, k = 5_000_000, 301, 256, 300
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    Z = torch.empty((N, D + 1), dtype=torch.float64, device="cuda")
    Z[:, :D] = torch.randn(N, D, dtype=torch.float64, device="cuda", generator=g)
    th = torch.randn(D, dtype=torch.float64, device="cuda", generator=g)
    Z[:, D] = Z[:, :D] @ th + torch.randn(N, dtype=torch.float64, device="cuda", generator=g)
    r = both_loops(torch, bc, loop, "linreg", Z, lambda: bc.LinregPosteriorSampler(np.zeros(D), np.eye(D), 1.0, seed=2), S, k, steps, warmup)
    r.update({"shape": "i", "family": "linreg", "N": N, "D": D, "S": S, "k": k, "colsum": "auto",
              "gradient_flops": 2.0 * k * S * D + 2.0 * k * S * (D + 1)})
    return r


def shape_ii(torch, bc, steps, warmup, loop="both"):
    N, D, S, k = 1_000_000, 10, 512, 100
    g = torch.Generator(device="cuda"); g.manual_seed(3)
    X = torch.randn(N, D, dtype=torch.float64, device="cuda", generator=g)
    th = torch.randn(D, dtype=torch.float64, device="cuda", generator=g)
    p = torch.sigmoid(X @ th)
    y = torch.where(torch.rand(N, dtype=torch.float64, device="cuda", generator=g) <= p, 1.0, -1.0)
    Z = (y[:, None] * X).contiguous()
    del X
    r = both_loops(torch, bc, loop, "logistic", Z, lambda: bc.LaplacePosteriorSampler("logistic", D, seed=4), S, k, steps, warmup)
    r.update({"shape": "ii", "family": "logistic", "N": N, "D": D, "S": S, "k": k, "gradient_flops": 4.0 * k * S * D})
    return r


def shape_iii(torch, reps=50):
    from bayesiancoresets_amd import _native
    lib = _native.load()
    k, S, D = 1024, 1024, 512
    g = torch.Generator(device="cuda"); g.manual_seed(5)
    rnd = lambda *s: torch.randn(*s, dtype=torch.float64, device="cuda", generator=g)
    out = {"shape": "iii", "k": k, "S": S, "D": D, "reps": reps}
    for fam, name in ((0, "logistic"), (2, "linreg")):
        dz = D + 1 if fam == 2 else D
        P, th = rnd(k, D + (fam == 2)), rnd(S, D) / D ** 0.5
        colsum, cv, w = rnd(S), rnd(k, S), rnd(k).abs()
        res = torch.empty(S + k + k * dz, dtype=torch.float64, device="cuda")
        work = torch.empty(int(lib.bcx_psvi_gradient_scratch_bytes(k, S)) // 8, dtype=torch.float64, device="cuda")
        st = int(torch.cuda.current_stream().cuda_stream)
        args = [st, fam, P.data_ptr(), k, P.stride(0), D, -1 if fam == 0 else D, th.data_ptr(), S, th.stride(0), 1.0,
                colsum.data_ptr(), cv.data_ptr(), S, w.data_ptr(), 1.0, res.data_ptr(), work.data_ptr()]
        for _ in range(5):
            assert lib.bcx_psvi_gradient(*args) == 0, lib.bcx_project_last_error().decode()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            lib.bcx_psvi_gradient(*args)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / reps
        flops = 2.0 * k * S * D + 2.0 * k * S * dz
        out[name] = {"ms": ms, "gflop": flops / 1e9, "tflops": flops / ms / 1e9, "of_fp64_mfma_peak": flops / ms / 1e-3 / PEAK_FP64_MFMA}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", choices=("all", "i", "ii", "iii"))
    ap.add_argument("--loop", default="both", choices=("both", "host", "enqueued"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bpsvi_bench needs a GPU")
    import bayesiancoresets_amd as bc
    lines = []
    if a.shape in ("all", "iii"):
        lines.append(shape_iii(torch))
    if a.shape in ("all", "ii"):
        lines.append(shape_ii(torch, bc, a.steps, a.warmup, a.loop))
    if a.shape in ("all", "i"):
        lines.append(shape_i(torch, bc, a.steps, a.warmup, a.loop))
    for r in lines:
        print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
