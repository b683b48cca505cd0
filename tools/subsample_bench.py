#!/usr/bin/env python3
"""Sub-sampled steps on rows gathered on the device: what they cost, against what.

kernels  the gathered COLSUM / SELECT kernel (bcx_project_colsum_rows / bcx_project_select_rows_ws) at n_rows = 10 000 and 100 000
         uniformly drawn rows of (i) N = 5M, D = 301, S = 256 linreg and (ii) N = 1M, D = 10, S = 512 logistic, against the contiguous
         kernel on a resident copy of the same rows and against bcx_gather_rows + the contiguous kernel.  hipEvents around each call,
         median of --steps calls after --warmup; the three forms alternate inside one pass and the pass is made twice.
steps    one ADAM step with n_subsample_opt = 10 000 and 100 000 at shape (ii), SparseVI (k = 64 seeded points) and BatchPSVI
         (k = 100), LaplacePosteriorSampler: the sub-sampled loop of a package root given by --parent (a checkout of the parent
         commit with its own built library: its host loop with the host gather), this tree's subsample="device" loop (enqueued) and
         this tree's full-data enqueued loop.  Each (root, mode) runs in a child process of its own, the three alternate and the round
         is made twice.  A step is the wall time of a whole _optimize() of --steps steps over its steps (synchronised at both ends,
         after a first _optimize() of --warmup steps): the host's index draws and uploads are part of what a step costs in every form.
Appends one JSON line per measurement to --out.
    python tools/subsample_bench.py [--what kernels|steps|all] [--parent DIR] [--steps 20] [--warmup 5] [--out profiles/subsample_bench.jsonl]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def med_ms(torch, fn, steps, warmup):
    ev = []
    for i in range(warmup + steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        ev.append((a, b))
    torch.cuda.synchronize()
    t = np.array([a.elapsed_time(b) for a, b in ev[warmup:]])
    return float(np.median(t)), float(t.min()), float(t.max())


def kernels(args):
    sys.path.insert(0, os.path.join(ROOT, "bayesian-coresets_amd"))
    import torch
    import bayesiancoresets_amd as bc
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    for shape, family, N, D, S in (("i", "linreg", 5_000_000, 301, 256), ("ii", "logistic", 1_000_000, 10, 512)):
        cols = D + 1 if family == "linreg" else D
        Z = torch.randn(N, cols, dtype=torch.float64, device="cuda", generator=g)
        theta = 0.1 * np.random.RandomState(2).randn(S, D)
        prj = bc.DeviceProjector(family, lambda n, w, p: theta, S, colsum="mfma")
        lib, resid = prj._lib, torch.randn(S, dtype=torch.float64, device="cuda", generator=g)
        col, res = torch.empty(S, dtype=torch.float64, device="cuda"), torch.empty(2, dtype=torch.float64, device="cuda")
        for n_rows in (10_000, 100_000):
            idx = torch.from_numpy(np.random.RandomState(3).randint(N, size=n_rows)).cuda()
            copy = Z[idx]
            gbuf = torch.empty_like(copy)
            work = prj._workspace(S)
            sw = prj._select_scratch(n_rows, S)
            tail_c = [col.data_ptr(), work.data_ptr()]
            tail_s = [resid.data_ptr(), float(resid.sum()), res.data_ptr(), sw.data_ptr(), sw.numel() * 8]
            gather = lambda: prj._check(lib.bcx_gather_rows(prj._stream(), Z.data_ptr(), Z.stride(0), cols, idx.data_ptr(), n_rows,
                                                            gbuf.data_ptr(), gbuf.stride(0)))
            forms = {
                "colsum": {"gathered": lambda: prj._check(lib.bcx_project_colsum_rows(*(prj._common(Z) + [idx.data_ptr(), n_rows] + tail_c))),
                           "contiguous_copy": lambda: prj._check(lib.bcx_project_colsum(*(prj._common(copy) + tail_c))),
                           "gather_then_contiguous": lambda: (gather(), prj._check(lib.bcx_project_colsum(*(prj._common(gbuf) + tail_c))))},
                "select": {"gathered": lambda: prj._check(lib.bcx_project_select_rows_ws(*(prj._common(Z) + [idx.data_ptr(), n_rows] + tail_s))),
                           "contiguous_copy": lambda: prj._check(lib.bcx_project_select_ws(*(prj._common(copy) + tail_s))),
                           "gather_then_contiguous": lambda: (gather(), prj._check(lib.bcx_project_select_ws(*(prj._common(gbuf) + tail_s))))},
            }
            for consumer, fs in forms.items():
                for rep in range(2):
                    rec = {"what": "kernel", "shape": shape, "family": family, "N": N, "D": D, "S": S, "n_rows": n_rows,
                           "consumer": consumer, "pass": rep, "row_bytes": 8 * cols,
                           "line_bytes_per_row": 128 * ((8 * cols + 127) // 128)}
                    for name, fn in fs.items():
                        m, lo, hi = med_ms(torch, fn, args.steps, args.warmup)
                        rec[name + "_ms"], rec[name + "_ms_min"], rec[name + "_ms_max"] = m, lo, hi
                    rec["gathered_over_contiguous"] = rec["gathered_ms"] / rec["contiguous_copy_ms"]
                    emit(args.out, rec)
        del Z, copy, gbuf
        prj.release_scratch()
        torch.cuda.empty_cache()


def worker(args):
    """One (package root, mode): the four (coreset, n_sub) steps at shape (ii).  mode "sub-host": the root's default sub-sampled loop
    (no keyword: also what a parent checkout has); "sub-device": subsample="device"; "full": the full-data enqueued loop."""
    sys.path.insert(0, os.path.join(args.root, "bayesian-coresets_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import bayesiancoresets_amd as bc
    from lr_workload import make_data
    N, D, S = 1_000_000, 10, 512
    Z = make_data(1, N, D)
    kw = {"subsample": "device"} if args.mode == "sub-device" else {}
    for coreset, k in (("sparsevi", 64), ("bpsvi", 100)):
        for n_sub in ((None,) if args.mode == "full" else (10_000, 100_000)):
            times = []
            for T in (args.warmup, args.steps):
                smp = bc.LaplacePosteriorSampler("logistic", D, seed=1)
                prj = bc.DeviceProjector("logistic", smp, S)
                np.random.seed(1)
                if coreset == "sparsevi":
                    alg = bc.SparseVICoreset(Z, prj, n_subsample_opt=n_sub, opt_itrs=T, step_sched=lambda i: 0.1 / (1.0 + i), **kw)
                    idcs = np.sort(np.random.RandomState(4).choice(N, size=k, replace=False))
                    alg.wts, alg.idcs, alg.pts = np.full(k, N / k), idcs, Z[idcs].copy()
                    if args.mode != "sub-host":
                        prj._dev(Z)                     # (resident before the clock starts, as it is from the first greedy step on)
                        if kw:
                            alg._resident()
                    run = alg._optimize
                else:
                    alg = bc.BatchPSVICoreset(Z, prj, T, n_subsample_opt=n_sub, step_sched=lambda i: 0.1 / (1.0 + i), **kw)
                    first = np.random.choice(N, size=k, replace=False)
                    alg.pts, alg.wts, alg.idcs = Z[first].copy(), N / k * np.ones(k), -1 * np.ones(k)
                    if args.mode != "sub-host":
                        prj._dev(Z)
                        if kw:
                            alg._resident()
                    run = alg._optimize
                torch.cuda.synchronize()
                t = time.perf_counter()
                run()
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t) * 1e3 / T)
            enq = (alg._enqueue_plan() if n_sub is None else getattr(alg, "_enqueue_plan_subsampled", lambda: None)()) is not None
            emit(args.out, {"what": "step", "root": args.tag, "mode": args.mode, "coreset": coreset, "k": k, "N": N, "D": D, "S": S,
                            "n_sub": n_sub, "steps": args.steps, "step_ms": times[1], "warmup_step_ms": times[0], "enqueued": bool(enq),
                            "round": args.round, "finite": bool(np.isfinite(alg.wts).all())})


def steps(args):
    runs = [("this", ROOT, "sub-device"), ("this", ROOT, "full")]
    if args.parent:
        runs.insert(0, ("parent", os.path.abspath(args.parent), "sub-host"))
    else:
        emit(args.out, {"what": "note", "text": "no --parent root given: the parent's step was not measured"})
    for rnd in range(2):
        for tag, root, mode in runs:
            rc = subprocess.call([sys.executable, os.path.abspath(__file__), "--what", "worker", "--root", root, "--tag", tag, "--mode", mode,
                                  "--round", str(rnd), "--steps", str(args.steps), "--warmup", str(args.warmup), "--out", args.out or ""],
                                 timeout=600)
            if rc != 0:
                raise SystemExit("subsample_bench: %s / %s ended with status %d" % (tag, mode, rc))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="all", choices=("kernels", "steps", "all", "worker"))
    ap.add_argument("--parent", default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subsample_bench.jsonl"))
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--tag", default="this")
    ap.add_argument("--mode", default="sub-device")
    ap.add_argument("--round", type=int, default=0)
    a = ap.parse_args()
    if a.what == "worker":
        worker(a)
    else:
        if a.what in ("kernels", "all"):
            kernels(a)
        if a.what in ("steps", "all"):
            steps(a)
