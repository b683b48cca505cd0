#!/usr/bin/env python3
"""Golden vectors for the held-out log predictive density (bc.log_predictive, csrc/predict.hip): per family N = 40 seeded rows and
S = 96 draws (D = 3 logistic, D = 4 Poisson), the reference's own log_likelihood(Z, Theta) table (examples/common/model_lr.py:25-32,
model_poiss.py:25-38) and lppd = logsumexp_s - log S and mean_ll formed from that table.  The reference is imported AT GENERATION
TIME only; the fixture holds inputs and outputs.
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_predictive.py

The draws: 94 moderate ones from N(theta*, 0.3^2 I) and the two all-tail draws of make_golden_mcmc.py (|x.theta| ~ 150: logistic
large multiples of a direction, Poisson the intercept alone at +-150).  Before anything is written the reference's float64 table is
held against the long-double restatement (tests/predictive_restatement.py) entry by entry: within 8 x 2^-52 x max(1, |value|).
An input where the reference itself were less accurate than that would be dropped, not papered over; with this seed none is
(worst entry 1.6 x 2^-52 of the Poisson table -- 2.1 x 2^-52 on the +150 draw, whose rate e^150 is the whole value -- and 4.5 x
2^-52 of the logistic one), so the fixture holds every draw listed above."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(1, "/root/reference/examples/common")
sys.path.insert(1, os.path.dirname(HERE))
import model_lr as ref_lr  # noqa: E402 (reference)
import model_poiss as ref_poiss  # noqa: E402 (reference)
import predictive_restatement as restate  # noqa: E402

try:
    from scipy.special import logsumexp
except ImportError:                                   # (the same quantity without scipy)
    def logsumexp(a, axis):
        return np.logaddexp.reduce(a, axis=axis)

OUT = os.path.join(HERE, "predictive_golden.npz")
N, S = 40, 96


def main():
    rs = np.random.RandomState(43)
    out = {}
    # Poisson: rows [x, 1, y]
    D = 4
    tstar = np.array([0.7, -0.4, 0.3, 0.2])
    X = np.hstack((rs.randn(N, D - 1), np.ones((N, 1))))
    y = rs.poisson(np.log1p(np.exp(X.dot(tstar)))).astype(np.float64)
    Zp = np.hstack((X, y[:, None]))
    thp = np.vstack((tstar + 0.3 * rs.randn(S - 2, D), [0.1, -0.1, 0.05, 150.0], [0.1, -0.1, 0.05, -150.0]))
    # logistic: rows y x
    tstar = np.array([1.5, -1.0, 0.3])
    Xl = np.hstack((rs.randn(N, 2), np.ones((N, 1))))
    p = 1.0 / (1.0 + np.exp(-Xl.dot(tstar)))
    yl = np.where(rs.rand(N) <= p, 1.0, -1.0)
    Zl = yl[:, None] * Xl
    thl = np.vstack((tstar + 0.3 * rs.randn(S - 2, 3), [200.0, -200.0, 100.0], [-400.0, 300.0, 50.0]))
    for tag, family, ref, Z, th in (("poiss", "poisson", ref_poiss, Zp, thp), ("lr", "logistic", ref_lr, Zl, thl)):
        assert Z.shape[0] == N and th.shape[0] == S
        ll = np.asarray(ref.log_likelihood(Z.copy(), th.copy()), dtype=np.float64)
        referee = restate.log_likelihood(family, Z, th, np.longdouble)
        dev = np.abs(ll - referee) / np.maximum(1.0, np.abs(referee))
        worst = float(dev.max())
        print("%s: reference table against the long-double restatement: worst %.3g x 2^-52 (draw %d)"
              % (tag, worst / 2.0 ** -52, int(np.argmax(dev.max(axis=0)))))
        assert worst <= 8 * 2.0 ** -52, (tag, worst)
        out[tag + "_Z"], out[tag + "_th"], out[tag + "_ll"] = Z, th, ll
        out[tag + "_lppd"] = logsumexp(ll, axis=1) - np.log(S)
        out[tag + "_mean_ll"] = ll.mean(axis=1)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, {k: v.shape for k, v in out.items()}, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
