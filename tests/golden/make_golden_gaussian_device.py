#!/usr/bin/env python3
"""Golden vectors F18: the reference's Monte-Carlo projection of the Gaussian-mean model -- BlackBoxProjector with
model_gaussian's log_likelihood / grad_x_log_likelihood and the weighted-posterior sampler of examples/gaussian/main.py:107-112
-- on the F16 data (tests/golden/gaussian_golden.npz: N = 500, D = 6, full covariance): what the device projector's "gaussian"
family has to reproduce.
  * project(x) and project(P, grad=True) at stored draws;
  * SparseVICoreset (np.random.seed(5), opt_itrs = 12, 5 steps), weights and indices after every step;
  * BatchPSVICoreset (opt_itrs = 30, build(8)), full data and n_subsample_opt = 100;
  * HilbertCoreset (GIGA, 10 steps) at draws from the full-data posterior.
The reference is imported AT GENERATION TIME; the fixture holds inputs and outputs only.
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gaussian_device.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
sys.path.insert(1, "/root/reference/examples/common")
import bayesiancoresets as bc  # noqa: E402 (reference)
import model_gaussian as gaussian  # noqa: E402 (reference example model)

OUT = os.path.join(HERE, "gaussian_device_golden.npz")
S_PROJ, S_RUN = 40, 50
SVI_SEED, SVI_ITRS, SVI_STEPS = 5, 12, 5
PSVI_SEED, PSVI_ITRS, PSVI_K, PSVI_NSUB = 9, 30, 8, 100
GIGA_SEED, GIGA_STEPS = 3, 10


def main():
    f16 = np.load(os.path.join(HERE, "gaussian_golden.npz"))
    x, Sig, mu0, Sig0inv = f16["x"], f16["Sig"], f16["mu0"], f16["Sig0inv"]
    N, D = x.shape
    Siginv = np.linalg.inv(Sig)
    logdet = np.linalg.slogdet(Sig)[1]
    ll = lambda pts, th: gaussian.log_likelihood(pts, th, Siginv, logdet)
    gll = lambda pts, th: gaussian.grad_x_log_likelihood(pts, th, Siginv)

    def sampler_w(n, wts, pts):
        if wts is None or pts is None or pts.shape[0] == 0:
            wts = np.zeros(1)
            pts = np.zeros((1, mu0.shape[0]))
        muw, USigw, _ = gaussian.weighted_post(mu0, Sig0inv, Siginv, pts, wts)
        return muw + np.random.randn(n, muw.shape[0]).dot(USigw.T)

    g = dict(x=x, Sig=Sig, mu0=mu0, Sig0inv=Sig0inv)
    # ---- projections at stored draws: around the full-data posterior (tight, mean far from 0) ----
    rs = np.random.RandomState(18)
    mup, Up, _ = gaussian.weighted_post(mu0, Sig0inv, Siginv, x, np.ones(N))
    th = mup + rs.randn(S_PROJ, D).dot(Up.T)
    P = x[rs.choice(N, 7, replace=False)] + 0.3 * rs.randn(7, D)
    prj = bc.BlackBoxProjector(lambda n, w, p: th.copy(), S_PROJ, ll, gll)
    g["th"], g["P"] = th, P
    g["proj_x"] = prj.project(x)
    g["proj_P_lls"], g["proj_P_glls"] = prj.project(P, grad=True)
    # ---- SparseVI ----
    np.random.seed(SVI_SEED)
    s = bc.SparseVICoreset(x, bc.BlackBoxProjector(sampler_w, S_RUN, ll, gll), opt_itrs=SVI_ITRS, step_sched=lambda i: 1.0 / (1.0 + i))
    wts_steps = np.zeros((SVI_STEPS, SVI_STEPS))
    for t in range(SVI_STEPS):
        s.build(1)
        w, p, idcs = s.get()
        wts_steps[t, :len(s.wts)] = s.wts
    g["svi_idcs_order"], g["svi_wts_steps"] = np.asarray(s.idcs), wts_steps
    # ---- BatchPSVI ----
    for tag, nsub in (("full", None), ("sub", PSVI_NSUB)):
        np.random.seed(PSVI_SEED)
        alg = bc.BatchPSVICoreset(x, bc.BlackBoxProjector(sampler_w, S_RUN, ll, gll), opt_itrs=PSVI_ITRS, n_subsample_opt=nsub,
                                  step_sched=lambda i: 0.5 / (1.0 + i))
        alg.build(PSVI_K)
        g["psvi_%s_wts" % tag], g["psvi_%s_pts" % tag] = alg.wts.copy(), alg.pts.copy()
    # ---- Hilbert (GIGA) at fixed draws from the full-data posterior ----
    np.random.seed(GIGA_SEED)
    h = bc.HilbertCoreset(x, bc.BlackBoxProjector(lambda n, w, p: mup + np.random.randn(n, D).dot(Up.T), S_RUN, ll, gll))
    h.build(GIGA_STEPS)
    wts, pts, idcs = h.get()
    g["giga_wts"], g["giga_idcs"] = wts, idcs
    assert all(np.isfinite(v).all() for v in g.values())
    np.savez_compressed(OUT, **g)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
    print("SVI rows", g["svi_idcs_order"], "\nSVI wts", wts_steps[-1], "\nPSVI wts", g["psvi_full_wts"], "\nGIGA idcs", idcs)


if __name__ == "__main__":
    main()
