"""The 8-bit screening tier's own counters on a bench.py workload: the same rows (bench.load_synthetic, same seed), the same
warm-up and timed build as the plain bench run, then Engine.screen_stats() / stats(), the time the shadow build took and the
device memory it added.

    python tools/screen8_stats.py [--config c4] [--steps 300] [--warmup 30] [--dtype float32]

Prints one JSON line.  The cap of the tier's issue: at c4, at most 3 of the 300 timed iterations redone with the
storage-precision scan and none with the exact scan."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "bayesian-coresets_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c4", choices=["c2", "c4"])
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--dtype", default="float32", choices=["float32", "float16"])
    args = ap.parse_args()
    import torch
    import bench
    from bayesiancoresets_amd import _native as nat
    from bayesiancoresets_amd.sharded import ShardedSolver
    cfg = bench.CONFIGS[args.config]
    args.rows, args.dim, args.seed = cfg["rows"], cfg["dim"], 1
    alg = {"giga": nat.ALG_GIGA, "fw": nat.ALG_FW}[cfg["alg"]]
    free0 = torch.cuda.mem_get_info()[0]
    s = ShardedSolver(alg, args.rows, args.dim, device=0, store_dtype=nat.F16 if args.dtype == "float16" else nat.F32)
    bench.load_synthetic(args, torch, s)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    assert s.finalize(None) == nat.OK
    torch.cuda.synchronize()
    fin_s = time.perf_counter() - t0
    free1 = torch.cuda.mem_get_info()[0]
    s.build(args.warmup)
    torch.cuda.synchronize()
    free2 = torch.cuda.mem_get_info()[0]
    before = s.engine.screen_stats()
    t0 = time.perf_counter()
    s.build(args.steps)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    after, st = s.engine.screen_stats(), s.engine.stats()
    print(json.dumps({
        "config": args.config, "dtype": args.dtype, "steps": args.steps, "warmup": args.warmup,
        "its_per_s": args.steps / el, "finalize_ms": fin_s * 1e3, "shadow_build_ms": after["build_us"] / 1e3,
        "device_bytes_before_first_build": free0 - free1, "device_bytes_added_by_first_build": free1 - free2,
        "tier_device_bytes": after["device_bytes"], "state": after["state"],
        "timed_screened": after["screened"] - before["screened"], "timed_survivors": after["survivors"] - before["survivors"],
        "timed_capture_overflows": after["overflows"] - before["overflows"],
        "timed_storage_redos": after["storage_redos"] - before["storage_redos"],
        # the 4-bit front pass (csrc/screen4.hip)
        "front4_state": after["front4_state"], "front4_device_bytes": after["front4_device_bytes"],
        "timed_front4_iterations": after["front4_iterations"] - before["front4_iterations"],
        "timed_front4_listed": after["front4_listed"] - before["front4_listed"],
        "timed_front4_overflows": after["front4_overflows"] - before["front4_overflows"],
        "timed_front4_redos": after["front4_redos"] - before["front4_redos"],
        "exact_fallbacks": st["exact_fallbacks"], "fp64_candidates": st["candidates"], "resolves": st["resolves"]}))


if __name__ == "__main__":
    main()
