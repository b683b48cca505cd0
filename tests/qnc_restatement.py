"""Plain NumPy restatement of the quasi-Newton coreset step (Naik, Rousseau and Campbell, 2022), the yardstick
of tests/test_qnc_host.py and tests/test_gpu_qnc.py:

    V      = V_raw - row means                         (projector.py:21)
    resid  = c - V^T w
    b      = V resid / S
    G      = V V^T / S
    d      : (G + tau I) d = b
    w      <- max(w + gamma d, 0)                      (np.maximum: a NaN stays a NaN)

in ``np.float64`` -- the product's host loop in its own arithmetic and library (``np.linalg.cholesky`` / ``solve``) -- and in
``np.longdouble``, the referee: every product and sum in long double, the factorisation and the two triangular solves written
out column by column (``np.linalg`` does not take long double).  The written-out forms take either type."""
import numpy as np


def cholesky(A):
    """Lower factor of A (any float dtype), column by column.  ``LinAlgError`` on a pivot that is not positive or NaN."""
    A = np.array(A)
    k = A.shape[0]
    L = np.zeros_like(A)
    for c in range(k):
        piv = A[c, c] - L[c, :c].dot(L[c, :c])
        if not piv > 0:
            raise np.linalg.LinAlgError("pivot %d is not positive: %r" % (c, piv))
        L[c, c] = np.sqrt(piv)
        if c + 1 < k:
            L[c + 1:, c] = (A[c + 1:, c] - L[c + 1:, :c].dot(L[c, :c])) / L[c, c]
    return L


def solve_lower(L, b):
    y = np.zeros_like(b)
    for i in range(b.shape[0]):
        y[i] = (b[i] - L[i, :i].dot(y[:i])) / L[i, i]
    return y


def solve_upper(U, y):
    x = np.zeros_like(y)
    for i in range(y.shape[0] - 1, -1, -1):
        x[i] = (y[i] - U[i, i + 1:].dot(x[i + 1:])) / U[i, i]
    return x


def system(c, V_raw, w, tau, dtype):
    """(V centred, A = G + tau I, b) in ``dtype``."""
    V = np.asarray(V_raw, dtype=dtype)
    c, w = np.asarray(c, dtype=dtype), np.asarray(w, dtype=dtype)
    S = V.shape[1]
    V = V - V.mean(axis=1)[:, None]
    resid = c - w.dot(V)
    b = V.dot(resid) / S
    A = V.dot(V.T) / S + dtype(tau) * np.eye(V.shape[0], dtype=dtype)
    return V, A, b


def step(c, V_raw, w, gamma, tau, dtype=np.float64):
    """One step: (new weights, direction).  ``c``: scaling x the data's column sums; ``V_raw``: k x S uncentred rows."""
    _, A, b = system(c, V_raw, w, tau, dtype)
    if dtype is np.float64:
        L = np.linalg.cholesky(A)
        d = np.linalg.solve(L.T, np.linalg.solve(L, b))
    else:
        L = cholesky(A)
        d = solve_upper(L.T, solve_lower(L, b))
    return np.maximum(np.asarray(w, dtype=dtype) + dtype(gamma) * d, dtype(0)), d


def loop(inputs, w0, sched, tau, dtype=np.float64):
    """``len(sched)`` steps from ``w0``: ``inputs(i, w)`` returns (c, V_raw) of step i at the float64 weights ``w`` (the draws
    come from a sampler that takes float64 weights: the referee is fed the call form rounded to float64)."""
    w = np.asarray(w0, dtype=dtype)
    for i, gamma in enumerate(sched):
        c, V_raw = inputs(i, np.asarray(w, dtype=np.float64))
        w, _ = step(c, V_raw, w, gamma, tau, dtype)
    return w
