#!/usr/bin/env python3
"""How well does the NumPy restatement of BatchPSVI (tests/test_bpsvi_host.py restated_bpsvi) reproduce ITSELF?  CPU only.
One run records the draws of a NumPy sampler; a second run replays them from the same starting rows with the rows of the data in
another order (the same sums, rounded in another order).  Prints, per shape, the weights' worst relative difference and the
points' worst |diff| / (atol + rtol |want|) at the tolerances the device tests use (rtol 1e-6, atol 1e-8): with fewer points than
columns (k < D + 1) the trajectory amplifies float64 rounding beyond them, so the restatement cannot referee there.
    python tools/bpsvi_smallk_sensitivity.py"""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
for p in (os.path.join(ROOT, "bayesian-coresets_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

from models import linreg_log_likelihood, linreg_sampler, make_linreg_data      # noqa: E402
from test_bpsvi_host import linreg_grad, restated_bpsvi                        # noqa: E402


class _Record(object):
    def __init__(self, inner):
        self.inner, self.draws = inner, []

    def __call__(self, n, w, p):
        th = np.array(self.inner(n, w, p))
        self.draws.append(th)
        return th


class _Replay(object):
    def __init__(self, draws):
        self.draws, self.i = draws, 0

    def __call__(self, n, w, p):
        self.i += 1
        return self.draws[self.i - 1]


def main():
    sig, sched = 1.0, (lambda i: 0.2 / (1.0 + i))
    ll, gll = (lambda z, t: linreg_log_likelihood(z, t, sig)), (lambda z, t: linreg_grad(z, t, sig))
    choice = np.random.choice
    for (N, D, S, k, T) in ((20000, 12, 64, 4, 15), (20000, 12, 64, 8, 15), (20000, 12, 64, 13, 15), (20000, 12, 64, 20, 15),
                            (20000, 4, 64, 6, 15), (20000, 5, 64, 6, 15), (200000, 5, 128, 6, 20)):
        Z = make_linreg_data(11, N, D)
        rec, got = _Record(linreg_sampler(np.zeros(D), np.eye(D), sig)), {}

        def keep(n, size, replace):
            got["first"] = choice(n, size=size, replace=replace)
            return got["first"]
        np.random.seed(3)
        np.random.choice = keep
        try:
            w, P = restated_bpsvi(Z, rec, S, ll, gll, k, T, None, sched)
            perm = np.random.RandomState(1).permutation(N)
            inv = np.argsort(perm)
            np.random.choice = lambda n, size, replace: inv[got["first"]]
            w2, P2 = restated_bpsvi(Z[perm], _Replay(rec.draws), S, ll, gll, k, T, None, sched)
        finally:
            np.random.choice = choice
        print("N %6d D %2d S %3d k %2d T %2d: weights %.3e relative, points %.3e of the bound"
              % (N, D, S, k, T, (np.abs(w - w2) / np.abs(w)).max(), (np.abs(P - P2) / (1e-8 + 1e-6 * np.abs(P))).max()), flush=True)


if __name__ == "__main__":
    main()
