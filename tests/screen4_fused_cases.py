"""The builds tests/test_gpu_screen4_fused.py compares between the default path (the front pass computes its own threshold
from the sentinels the previous refine kernel left) and a child process started with BCX_DEV=1 BCX_SCREEN4=0 (the 8-bit tier
alone).  Run as a script it computes every case and writes one .npz:

    BCX_DEV=1 BCX_SCREEN4=0 python tests/screen4_fused_cases.py OUT.npz

Shapes are the smallest at which the code takes another path: one d per pair of 4-bit / 8-bit lane geometry the launchers
instantiate, row counts that are no multiple of a workgroup trip, one row past a trip, fewer rows than one trip and than
there are sentinels, and rank-100 rows of which one wave lists all four once.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# d -> rows; (G, CH | G8, CH8): 16 (1,1|1,1)  24 (1,1|2,1)  40 (2,1|4,1)  100 (4,1|8,1)  256 (8,1|16,1)  512 (16,1|32,1)
# 520 (32,1|64,1: 17 and 33 pieces, the clamped lanes)  1000 (32,1|64,1)  2048 (64,1|64,2)  4096 (64,2|64,4)
GEOMETRY = {16: 19999, 24: 10001, 40: 8197, 100: 6001, 256: 5003, 512: 4099, 520: 3001, 1000: 3001, 2048: 2051, 4096: 2051}


def rows_per_trip(d):
    """Rows one workgroup of front4_kernel takes per trip, and the workgroups / list segments of a launch over n rows."""
    ldv = (d + 31) // 32
    G = 1
    while G < 64 and G < ldv:
        G <<= 1
    CH = 1
    while CH * G < ldv:
        CH <<= 1
    return 4 * (64 // G) * (8 if CH == 1 else 4)


def segments(n, d):
    rpb = rows_per_trip(d)
    return 4 * max(1, min(512, (n + rpb - 1) // rpb))


def _cls(bc, alg):
    return {"fw": bc.snnls.FrankWolfe, "omp": bc.snnls.OrthoPursuit}[alg]


CASES = {}   # name: (algorithm, seed, rows, d, build() calls; "reset" stands for reset())
# (seed 50 at d = 4096: with four rows per wave the 8-bit capture behind the list, two slots per wave, halts several iterations
# for most seeds, with or without the front pass; this one has none)
for _k, (_d, _n) in enumerate(sorted(GEOMETRY.items())):
    CASES["geom_d%d" % _d] = ("fw" if _k % 2 == 0 else "omp", 50 if _d == 4096 else 30 + _k, _n, _d, (16,))
CASES["remainder"] = ("fw", 41, 9001, 512, (16,))               # 284 segments: some list nothing, some a single row
CASES["ragged_one"] = ("omp", 42, 128 * 40 + 1, 512, (16,))     # one row past a trip: the clamped rows n - 1 beside it
CASES["tiny_fw"] = ("fw", 43, 50, 16, (12,))                    # one workgroup, 8 candidates for 64 sentinels
CASES["tiny_omp"] = ("omp", 44, 50, 16, (12,))
# run with BCX_SCREEN4_SEGCAP=3 by the test, plainly here.  Rank-100 rows: the front pass lists 10 to 250 of them, two or three
# of a wave's four, and with this seed all four of one wave in exactly one 4-bit iteration (tools/screen4_model.py, case
# "lowrank", seg_cap = 3: one redo; seeds 118, 121, 123, 140 and 144 of 100..149 do that)
CASES["segcap3"] = ("fw", 118, 2048, 4096, (16,))
CASES["calls_3x8"] = ("omp", 47, 9001, 256, (8, 8, 8))
CASES["calls_24"] = ("omp", 47, 9001, 256, (24,))
CASES["reset_rebuild"] = ("fw", 48, 9001, 256, (12, "reset", 12))


def rows_of(name):
    _, seed, n, d, _ = CASES[name]
    rs = np.random.RandomState(seed)
    if name == "segcap3":
        return rs.randn(n, 100) @ rs.randn(100, d)
    return rs.randn(n, d)


def run_case(bc, name):
    alg, _, _, _, calls = CASES[name]
    X = rows_of(name)
    s = _cls(bc, alg)(X.T, X.sum(axis=0), dtype="float32")
    out = {}
    for i, c in enumerate(calls):
        if c == "reset":
            s.reset()
            continue
        s.build(c)
        sel, err, status = s.last_trace
        out["sel%d" % i], out["err%d" % i], out["status%d" % i] = np.array(sel), np.array(err), np.array(status)
    out["w"] = np.array(s.weights())
    out["error"] = np.array(s.error())
    return out, s._eng.screen_stats()


def main(path):
    for p in (ROOT, os.path.join(ROOT, "bayesian-coresets_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import bayesiancoresets_amd as bc
    flat = {}
    for name in CASES:
        out, st = run_case(bc, name)
        assert st["front4_iterations"] == 0 and not st["front4_active"], (name, st)
        for k, v in out.items():
            flat[name + "/" + k] = v
    np.savez(path, **flat)


if __name__ == "__main__":
    main(sys.argv[1])
