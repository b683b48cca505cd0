"""A helper, not a test: the log predictive density of held-out rows restated plainly in NumPy, parameterised by dtype --
np.longdouble as the referee of the device tests, np.float64 as the yardstick that says what plain double arithmetic loses.
The two likelihoods are the reference's formulas (examples/common/model_lr.py:25-32, model_poiss.py:25-38) written out; the
reduction is a max-shifted log-sum-exp done ONCE per row over the whole table, no online rescaling.  Shares no code with the
library (csrc/predict.hip, bayesiancoresets_amd/predictive.py)."""
import math

import numpy as np


def _log_factorial(y, dtype):
    """log y! for non-negative integer-valued y.  long double: the sum of logs (2^-64 per term); float64: libm's lgamma."""
    y = np.asarray(y, dtype=np.float64)
    assert np.all(y >= 0) and np.all(y == np.round(y)), "counts"
    if dtype == np.float64:
        return np.array([math.lgamma(v + 1.0) for v in y.ravel()], dtype=np.float64).reshape(y.shape)
    top = int(y.max()) if y.size else 0
    table = np.concatenate((np.zeros(2, dtype=dtype), np.cumsum(np.log(np.arange(2, top + 2, dtype=dtype)))))   # table[k] = log k!
    return table[y.astype(np.int64)]


def log_likelihood(family, Z, Th, dtype=np.longdouble):
    """The N x S table ll(z_n, theta_s) in ``dtype``.  Z: rows y x (logistic) or [x, y] (Poisson); Th: S x D."""
    Z = np.atleast_2d(np.asarray(Z, dtype=np.float64)).astype(dtype)
    Th = np.atleast_2d(np.asarray(Th, dtype=np.float64)).astype(dtype)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if family == "logistic":
            m = -(Z.dot(Th.T))
            small = m < 100
            return np.where(small, -np.log1p(np.exp(np.where(small, m, 0))), -m)
        if family != "poisson":
            raise ValueError(family)
        x, y = Z[:, :-1], Z[:, -1:]
        s = x.dot(Th.T)
        rate = np.maximum(s, 0) + np.log1p(np.exp(-np.abs(s)))
        body = s > -100
        log_rate = np.where(body, np.log(np.where(body, rate, 1)), s)
        return y * log_rate - rate - _log_factorial(y, dtype).astype(dtype)


def reduce_table(ll):
    """(lppd, mean_ll) of a table (N x S): logsumexp over the draws minus log S with one shift per row, and the plain mean."""
    ll = np.asarray(ll)
    S = ll.shape[1]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        m = ll.max(axis=1)
        shift = np.where(np.isfinite(m), m, 0)
        lppd = shift + np.log(np.exp(ll - shift[:, None]).sum(axis=1) / ll.dtype.type(S))
        mean = ll.sum(axis=1) / ll.dtype.type(S)
    return lppd, mean


def log_predictive(family, Z, Th, dtype=np.longdouble):
    """(lppd, mean_ll), each N values of ``dtype``."""
    return reduce_table(log_likelihood(family, Z, Th, dtype))
