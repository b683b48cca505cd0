"""Dev tool: time of the pair-statistic kernel behind bc.energy_distance / bc.stein_discrepancy (csrc/pairstat.hip)
per call, in pairs per second and in fp64 lane-operations per second at S in {4096, 32 768, 262 144} draws a side and D in {3, 10,
32}: both kinds (0: distances, 1: Stein terms), A against itself (only the tiles on and above the diagonal are computed; the
pairs counted are those) and two samples of S draws each.  The inputs are resident on the device; a call is
discrepancy._pair_stat, i.e. the scratch allocation, bcx_pair_stat's two launches and the read-back of its two doubles.

Every timed window is warmed up by one untimed call of the same shape, ends in a device synchronise (the read-back) and is repeated
10 times; a line carries the median and the extremes.  Lane-operations are counted from the compiled loop: per pair and coordinate
2 fp64 VALU instructions (kind 0: one subtract, one FMA) or 5 (kind 1: two subtracts, three FMAs), and behind the loop 15 (the
correctly rounded square root, the select, the sum) or 19 (the reciprocal square root, ten multiply-adds, the select, the sums) --
the v_*_f64 instructions of the kernel's basic blocks over the 16 pairs of a thread's block.  The ceiling is DESIGN.md 4.19's:
256 CUs x 4 SIMDs x 16 fp64 lanes per clock at 2.4 GHz = 3.9e13 lane-operations per second.  One JSON line.

    python tools/discrepancy_bench.py [--quick]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "bayesian-coresets_amd")):
    sys.path.insert(0, p)

VALU_RATE = 256 * 4 * 16 * 2.4e9          # fp64 lane-operations per second
OPS_PER_K = {0: 2.0, 1: 5.0}              # fp64 VALU instructions per pair and coordinate in the compiled loop
OPS_BEHIND = {0: 15.0, 1: 19.0}           # ... and per pair behind it
TILE = 64


def timed(fn, reps):
    fn()                                                                        # (first-use costs, this shape)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()                                                                    # (ends in the read-back: a synchronise)
        ts.append(time.perf_counter() - t0)
    return dict(median_ms=float(np.median(ts)) * 1e3, min_ms=min(ts) * 1e3, max_ms=max(ts) * 1e3, reps=reps)


def main():
    import torch
    from bayesiancoresets_amd import discrepancy
    if not torch.cuda.is_available():
        raise RuntimeError("discrepancy_bench needs a GPU")
    sizes = (4096, 32768) if "--quick" in sys.argv else (4096, 32768, 262144)
    gen = torch.Generator(device="cuda").manual_seed(0)
    cases = []
    for S in sizes:
        for D in (3, 10, 32):
            X, Y, GX, GY = (torch.randn(S, D, dtype=torch.float64, device="cuda", generator=gen) for _ in range(4))
            for kind in (0, 1):
                for sym in (True, False):
                    args = (kind, X, GX if kind else None) + ((None, None) if sym else (Y, GY if kind else None))
                    t = timed(lambda: discrepancy._pair_stat(*args), 10)
                    tiles = (S + TILE - 1) // TILE
                    pairs = float(tiles * (tiles + 1) // 2) * TILE * TILE if sym else float(S) * S      # (the pairs computed)
                    ops = pairs * (OPS_PER_K[kind] * D + OPS_BEHIND[kind])
                    sec = t["median_ms"] * 1e-3
                    cases.append(dict(kind=kind, symmetric=sym, S=S, D=D, call=t, pairs=pairs, pairs_per_second=pairs / sec,
                                      lane_ops_per_second=ops / sec, fraction_of_valu_ceiling=ops / sec / VALU_RATE))
                    print("kind %d %s S %6d D %2d: %9.3f ms (%.3f - %.3f)  %.3g pairs/s  %.3g lane-ops/s  %.2f of the ceiling"
                          % (kind, "sym" if sym else "two", S, D, t["median_ms"], t["min_ms"], t["max_ms"], pairs / sec, ops / sec,
                             ops / sec / VALU_RATE), file=sys.stderr, flush=True)
            del X, Y, GX, GY
    print(json.dumps(dict(tool="discrepancy_bench", device=torch.cuda.get_device_name(0), valu_ceiling=VALU_RATE, cases=cases)), flush=True)


if __name__ == "__main__":
    main()
