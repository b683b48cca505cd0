#!/usr/bin/env python3
"""Golden vectors for the MCMC evaluation: the reference's weighted log joint and its gradient (examples/common/
model_lr.py:34-39, 59-64; model_poiss.py:40-46, 69-74) on small seeded logistic / Poisson sets of the F15 shapes (N = 900,
D = 3 / 4), unweighted and with 25 weighted points, at a handful of parameter vectors.  The reference is imported AT GENERATION
TIME only; the fixture holds inputs and outputs.
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mcmc.py

The parameter vectors: five of moderate size, and two that put EVERY row on a tail branch (|s| > 100).  For the logistic model
those are large multiples of a direction (both sides use e / (1 + e), which is stable everywhere).  For the Poisson model they
move the intercept alone to +-150, so that s = x.theta is within a few units of +-150 for all rows: the reference's gradient
(y e^-s - 1)(1 - exp(-e^s)) loses digits to cancellation in 1 - exp(-rate) where the rate is small but above its 1e-15
switch (relative error ~ 2^-53 / rate), a property of that formula and not of the model, so the fixture stays out of
-40 < s < -8 and compares where the reference is accurate to a few ulp per term."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(1, "/root/reference/examples/common")
import model_lr as ref_lr  # noqa: E402 (reference)
import model_poiss as ref_poiss  # noqa: E402 (reference)

OUT = os.path.join(HERE, "mcmc_golden.npz")


def main():
    rs = np.random.RandomState(41)
    out = {}
    N = 900
    w = np.zeros(N)
    sel = rs.choice(N, 25, replace=False)
    w[sel] = rs.uniform(5.0, 60.0, 25)
    # Poisson: rows [x, 1, y]
    D = 4
    X = np.hstack((rs.randn(N, D - 1), np.ones((N, 1))))
    y = rs.poisson(np.log1p(np.exp(X.dot(np.array([0.7, -0.4, 0.3, 0.2]))))).astype(np.float64)
    Zp = np.hstack((X, y[:, None]))
    thp = np.vstack((0.5 * rs.randn(5, D), [0.1, -0.1, 0.05, 150.0], [0.1, -0.1, 0.05, -150.0]))
    # logistic: rows y x
    Xl = np.hstack((rs.randn(N, 2), np.ones((N, 1))))
    p = 1.0 / (1.0 + np.exp(-Xl.dot(np.array([1.5, -1.0, 0.3]))))
    yl = np.where(rs.rand(N) <= p, 1.0, -1.0)
    Zl = yl[:, None] * Xl
    thl = np.vstack((rs.randn(5, 3), [200.0, -200.0, 100.0], [-400.0, 300.0, 50.0]))
    for tag, ref, Z, th in (("poiss", ref_poiss, Zp, thp), ("lr", ref_lr, Zl, thl)):
        out[tag + "_Z"], out[tag + "_th"] = Z, th
        for wtag, wts in (("full", np.ones(N)), ("wtd", w)):
            out["%s_%s_lj" % (tag, wtag)] = ref.log_joint(Z.copy(), th.copy(), wts)
            out["%s_%s_grad" % (tag, wtag)] = ref.grad_th_log_joint(Z.copy(), th.copy(), wts)
    out["w"] = w
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
