"""The builds tests/test_gpu_screen4.py compares between the default (4-bit front pass on) and a child process started with
BCX_DEV=1 BCX_SCREEN4=0 (the 8-bit tier alone).  Run as a script it computes every case and writes one .npz:

    BCX_DEV=1 BCX_SCREEN4=0 python tests/screen4_cases.py OUT.npz
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cls(bc, alg):
    return {"giga": bc.snnls.GIGA, "fw": bc.snnls.FrankWolfe, "omp": bc.snnls.OrthoPursuit}[alg]


def _rows(name):
    if name.startswith("randn"):
        return np.random.RandomState(5).randn(65536, 128)
    if name == "ragged":
        return np.random.RandomState(6).randn(8191 + 5, 40)       # ragged last trip, d no multiple of 32: padding nibbles
    if name == "long":
        return np.random.RandomState(7).randn(2048, 4096)
    if name == "repeated":
        return np.random.RandomState(8).randn(200, 64)[np.arange(20000) % 200]
    if name in ("reset", "incremental", "giga"):
        return np.random.RandomState(9).randn(30000, 64)
    raise AssertionError(name)


CASES = {  # name: (algorithm, dtype, build() calls; "reset" stands for reset())
    "randn_fw_f32": ("fw", "float32", (60,)), "randn_fw_f16": ("fw", "float16", (60,)),
    "randn_omp_f32": ("omp", "float32", (60,)), "randn_omp_f16": ("omp", "float16", (60,)),
    "ragged": ("fw", "float32", (40,)), "long": ("fw", "float32", (20,)), "repeated": ("fw", "float32", (40,)),
    "reset": ("fw", "float32", (20, "reset", 20)), "incremental": ("omp", "float32", (10, 10, 10)),
    "incremental_whole": ("omp", "float32", (30,)), "giga": ("giga", "float32", (40,)),
}


def run_case(bc, name):
    alg, dtype, calls = CASES[name]
    X = _rows("incremental" if name == "incremental_whole" else name)
    s = _cls(bc, alg)(X.T, X.sum(axis=0), dtype=dtype)
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
    return out, s._eng.screen_stats(), s._eng.stats()


def main(path):
    for p in (ROOT, os.path.join(ROOT, "bayesian-coresets_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import bayesiancoresets_amd as bc
    flat = {}
    for name in CASES:
        out, st, _ = run_case(bc, name)
        assert st["front4_iterations"] == 0 and not st["front4_active"], (name, st)
        for k, v in out.items():
            flat[name + "/" + k] = v
    np.savez(path, **flat)


if __name__ == "__main__":
    main(sys.argv[1])
