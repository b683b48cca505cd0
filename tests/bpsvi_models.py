"""Test-side inputs of the BatchPSVI tests (fixture F17, tests/golden/make_golden_bpsvi.py): a logistic-regression data
set and a small NumPy Gaussian sampler for it.  The product never imports this."""
import numpy as np


def make_logistic_data(seed, N, D):
    """Rows z = y x with labels y in {-1, 1} drawn from a logistic model (the form of examples/common/model_lr.py)."""
    rs = np.random.RandomState(seed)
    X = rs.randn(N, D)
    th = rs.randn(D)
    y = np.where(rs.rand(N) <= 1.0 / (1.0 + np.exp(-X.dot(th))), 1.0, -1.0)
    return y[:, None] * X


def logistic_sampler(N, D, scale=0.5):
    """Draws around the weighted mean of the points divided by N: cheap, and it moves with (w, P)."""
    def sampler(n, wts, pts):
        pts = np.asarray(pts)
        m = np.zeros(D) if pts.shape[0] == 0 else (np.asarray(wts)[:, None] * pts).sum(axis=0) / N
        return m + scale * np.random.randn(n, D)
    return sampler
