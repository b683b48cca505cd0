"""A helper, not a test: the energy distance and the IMQ kernel Stein discrepancy restated plainly in NumPy, straight from their
definitions -- ALL pairs, no symmetry shortcut, differences formed coordinate by coordinate -- and parameterised by dtype:
np.longdouble as the referee of the device tests, np.float64 as the yardstick that says what plain double arithmetic loses.
Shares no code with the library (csrc/pairstat.hip, bayesiancoresets_amd/discrepancy.py).

Every sum comes with its sum of absolute ELEMENTARY terms, the scale its rounding error is relative to: for distances the sum
itself; for a Stein term the absolute values of its four parts with the two dot products taken term by term,
    D q^(-3/2) + 3 |r|^2 q^(-5/2) + sum_k |(g_y - g_x)_k r_k| q^(-3/2) + sum_k |g_x,k g_y,k| q^(-1/2),
so that scores of size 1e6 whose products cancel are measured against what was added up, not against what was left."""
import numpy as np

CHUNK = 64          # rows of the first operand per pass: the pair table is never held whole


def _as(a, dtype):
    return np.atleast_2d(np.asarray(a)).astype(dtype)


def distance_sum(A, B, dtype=np.longdouble):
    """(sum over all (i, j) of |a_i - b_j|_2, the same: every term is its own absolute value)."""
    A, B = _as(A, dtype), _as(B, dtype)
    total = dtype(0)
    with np.errstate(invalid="ignore", over="ignore"):
        for i0 in range(0, A.shape[0], CHUNK):
            r = A[i0:i0 + CHUNK, None, :] - B[None, :, :]
            total += np.sqrt((r * r).sum(axis=2)).sum()
    return total, total


def stein_terms(A, GA, B, GB, c, dtype=np.longdouble):
    """(k_p(a_i, b_j) as an nA x nB table, the table of the absolute elementary terms)."""
    A, GA, B, GB = _as(A, dtype), _as(GA, dtype), _as(B, dtype), _as(GB, dtype)
    D = A.shape[1]
    c2 = dtype(c) * dtype(c)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        r = A[:, None, :] - B[None, :, :]
        d2 = (r * r).sum(axis=2)
        q = c2 + d2
        q12 = 1 / np.sqrt(q)
        q32 = q12 / q
        q52 = q32 / q
        dgr = (GB[None, :, :] - GA[:, None, :]) * r
        gg = GA[:, None, :] * GB[None, :, :]
        kp = D * q32 - 3 * d2 * q52 - dgr.sum(axis=2) * q32 + gg.sum(axis=2) * q12
        mag = D * q32 + 3 * d2 * q52 + np.abs(dgr).sum(axis=2) * q32 + np.abs(gg).sum(axis=2) * q12
    return kp, mag


def stein_sum(A, GA, B, GB, c, dtype=np.longdouble):
    """(sum over all (i, j) of k_p(a_i, b_j), the sum of the absolute elementary terms, the sum of the terms i = j -- which means
    something only when B is A)."""
    A, GA, B, GB = _as(A, dtype), _as(GA, dtype), _as(B, dtype), _as(GB, dtype)
    total, mag, diag = dtype(0), dtype(0), dtype(0)
    for i0 in range(0, A.shape[0], CHUNK):
        kp, m = stein_terms(A[i0:i0 + CHUNK], GA[i0:i0 + CHUNK], B, GB, c, dtype)
        total += kp.sum()
        mag += m.sum()
        n = min(kp.shape[0], B.shape[0] - i0)
        if n > 0:
            diag += kp[np.arange(n), i0 + np.arange(n)].sum()
    return total, mag, diag


def energy_distance(X, Y, dtype=np.longdouble):
    """(energy^2 = 2 m_xy - m_xx - m_yy, m_xy, m_xx, m_yy): the V-statistic, i = j included."""
    X, Y = _as(X, dtype), _as(Y, dtype)
    S, T = X.shape[0], Y.shape[0]
    m_xy = distance_sum(X, Y, dtype)[0] / (dtype(S) * dtype(T))
    m_xx = distance_sum(X, X, dtype)[0] / (dtype(S) * dtype(S))
    m_yy = distance_sum(Y, Y, dtype)[0] / (dtype(T) * dtype(T))
    return 2 * m_xy - m_xx - m_yy, m_xy, m_xx, m_yy


def stein_discrepancy(X, G, c=1.0, dtype=np.longdouble):
    """(ksd^2 the V-statistic, the U-statistic (NaN for one draw), the sum of the absolute elementary terms over S^2)."""
    X = _as(X, dtype)
    S = X.shape[0]
    total, mag, diag = stein_sum(X, G, X, G, c, dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        u = (total - diag) / (dtype(S) * dtype(S - 1)) if S > 1 else dtype(np.nan)
    return total / (dtype(S) * dtype(S)), u, mag / (dtype(S) * dtype(S))


def imq(x, y, c):
    """The base kernel (c^2 + |x - y|^2)^(-1/2)."""
    x, y = np.asarray(x), np.asarray(y)
    return 1 / np.sqrt(c * c + ((x - y) ** 2).sum(axis=-1))
