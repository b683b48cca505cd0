"""Test-side referee of the weighted conjugate posterior of Gaussian linear regression (examples/common/model_linreg.py:26-41;
the product never imports this):

    P = Sig0^-1 + X^T diag(max(w, 0)) X / sigsq = L L^T,      Sigma_w = P^-1,      mu_w = P^-1 (Sig0^-1 mu0 + X^T (w y) / sigsq)

evaluated in ``np.longdouble`` (64-bit significand on x86) by plain loops over rows and columns -- no LAPACK, no BLAS (NumPy has
neither for long double), and Sig0 is inverted here, through its own Cholesky factor, not taken inverted from float64.  The same
loops at ``dtype=np.float64`` are the second float64 evaluation of the reference's algorithm (``reference_loop``; the first, in
LAPACK's order, is tests/models.py linreg_weighted_post).

A candidate (mu, U) with Sigma = U U^T is measured in the posterior's own metric:

    e_cov  = max |L^T (U U^T) L - I|          (the identity when U U^T = P^-1, whatever the factor U)
    e_mean = ||L^T (mu - mu_w)||_2             (the mean's distance in posterior standard deviations)

and ``floor`` = 2^-53 max|mu_w| ||L||_F is what storing a draw in float64 costs in that metric (half an ulp of the largest
component of the mean in every component, against the factor's Frobenius norm): no float64 output can be held closer."""
import numpy as np

LD = np.longdouble


def cholesky(A, dtype=LD):
    """Lower factor of A by columns (inner products along the rows: the row-Cholesky / Cholesky-Banachiewicz order)."""
    A = np.asarray(A, dtype=dtype)
    n = A.shape[0]
    L = np.zeros((n, n), dtype=dtype)
    for j in range(n):
        d = A[j, j] - (L[j, :j] * L[j, :j]).sum(dtype=dtype)
        if not d > 0:
            raise np.linalg.LinAlgError("pivot %d is not positive" % j)
        L[j, j] = np.sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - (L[j + 1:, :j] * L[j, :j]).sum(axis=1, dtype=dtype)) / L[j, j]
    return L


def lower_inverse(L, dtype=LD):
    """L^-1 by forward substitution, row by row."""
    L = np.asarray(L, dtype=dtype)
    n = L.shape[0]
    X = np.zeros((n, n), dtype=dtype)
    for i in range(n):
        r = -(L[i, :i, None] * X[:i, :]).sum(axis=0, dtype=dtype)
        r[i] += dtype(1)
        X[i] = r / L[i, i]
    return X


def _matmul(A, B, dtype):
    """A B without BLAS at any dtype: NumPy's own loop for long double (it has no BLAS to call there), explicit sums by rows of A
    otherwise."""
    A, B = np.asarray(A, dtype=dtype), np.asarray(B, dtype=dtype)
    if dtype is LD and np.finfo(LD).eps < np.finfo(np.float64).eps:
        return np.matmul(A, B)
    out = np.zeros((A.shape[0], B.shape[1]), dtype=dtype)
    for i in range(A.shape[0]):
        out[i] = (A[i, :, None] * B).sum(axis=0, dtype=dtype)
    return out


def spd_inverse(A, dtype=LD):
    Ci = lower_inverse(cholesky(A, dtype), dtype)
    return _matmul(Ci.T, Ci, dtype)


def precision(Sig0, sigsq, pts, w, dtype=LD, Sig0inv=None):
    """(P, Sig0^-1) at ``dtype``; negative weights count as zero (the kernels clamp them)."""
    S0i = spd_inverse(Sig0, dtype) if Sig0inv is None else np.asarray(Sig0inv, dtype=dtype)
    pts = np.asarray(pts, dtype=dtype).reshape(-1, S0i.shape[0] + 1)
    X = pts[:, :-1]
    wc = np.maximum(np.asarray(w, dtype=dtype), dtype(0))
    return S0i + _matmul((X * wc[:, None]).T, X, dtype) / dtype(sigsq), S0i


def rhs(mu0, S0i, sigsq, pts, w, dtype=LD):
    pts = np.asarray(pts, dtype=dtype).reshape(-1, S0i.shape[0] + 1)
    X, y = pts[:, :-1], pts[:, -1]
    wc = np.maximum(np.asarray(w, dtype=dtype), dtype(0))
    return (S0i * np.asarray(mu0, dtype=dtype)[None, :]).sum(axis=1, dtype=dtype) + ((wc * y)[:, None] * X).sum(axis=0, dtype=dtype) / dtype(sigsq)


class Referee(object):
    """P, L_R, L_R^-1 and mu_R of one case in long double, and the two errors of a candidate against them."""

    def __init__(self, mu0, Sig0, sigsq, pts, w, dtype=LD):
        self.dtype = dtype
        self.P, self.S0i = precision(Sig0, sigsq, pts, w, dtype)
        self.L = cholesky(self.P, dtype)
        self.Linv = lower_inverse(self.L, dtype)
        b = rhs(mu0, self.S0i, sigsq, pts, w, dtype)
        u = (self.Linv * b[None, :]).sum(axis=1, dtype=dtype)                    # L^-1 b
        self.uvec = u
        self.mu = (self.Linv * u[:, None]).sum(axis=0, dtype=dtype)              # L^-T (L^-1 b)
        self.D = self.L.shape[0]
        self.floor = float(dtype(2.0) ** -53 * np.abs(self.mu).max() * np.sqrt((self.L * self.L).sum(dtype=dtype)))

    def e_cov(self, U):
        """max |L^T (U U^T) L - I| for a D x D factor U of the candidate's covariance (any factor: U U^T is what counts)."""
        M = _matmul(self.L.T, np.asarray(U, dtype=self.dtype), self.dtype)
        G = _matmul(M, M.T, self.dtype)
        G[np.diag_indices(self.D)] -= self.dtype(1)
        return float(np.abs(G).max())

    def e_mean(self, mu):
        d = np.asarray(mu, dtype=self.dtype) - self.mu
        v = (self.L * d[:, None]).sum(axis=0, dtype=self.dtype)                  # L^T d
        return float(np.sqrt((v * v).sum(dtype=self.dtype)))

    def d_cov(self, U1, U2):
        """max |L^T (U1 U1^T - U2 U2^T) L|: two candidates against each other, in the same metric."""
        M1 = _matmul(self.L.T, np.asarray(U1, dtype=self.dtype), self.dtype)
        M2 = _matmul(self.L.T, np.asarray(U2, dtype=self.dtype), self.dtype)
        return float(np.abs(_matmul(M1, M1.T, self.dtype) - _matmul(M2, M2.T, self.dtype)).max())

    def d_mean(self, mu1, mu2):
        d = np.asarray(mu1, dtype=self.dtype) - np.asarray(mu2, dtype=self.dtype)
        v = (self.L * d[:, None]).sum(axis=0, dtype=self.dtype)
        return float(np.sqrt((v * v).sum(dtype=self.dtype)))

    def cond(self):
        """cond_2(P), from float64 eigenvalues of the long-double P (a figure for a precondition, not a referee's value)."""
        ev = np.linalg.eigvalsh(np.asarray(self.P, dtype=np.float64))
        return float(ev[-1] / ev[0])


def reference_loop(mu0, Sig0inv, sigsq, pts, w, dtype=np.float64):
    """The reference's algorithm (Cholesky of P, U = L^-T, mu = (U U^T) rhs: the covariance is FORMED and then applied, as
    tests/models.py linreg_weighted_post restates it in LAPACK's order) by this module's loops at ``dtype``, from the float64
    Sig0^-1 the reference itself starts from: (mu, U)."""
    S0i = np.asarray(Sig0inv, dtype=dtype)
    P, _ = precision(None, sigsq, pts, w, dtype, Sig0inv=S0i)
    Li = lower_inverse(cholesky(P, dtype), dtype)
    b = rhs(mu0, S0i, sigsq, pts, w, dtype)
    Sigma = _matmul(Li.T, Li, dtype)
    return (Sigma * b[None, :]).sum(axis=1, dtype=dtype), Li.T.copy()
