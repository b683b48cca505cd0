"""CPU-only: what the streamed NUTS (csrc/nuts_stream.hip) is held to on the host.  (1) the resumable statement
of the transition (tests/nuts_stream_restatement.py: one evaluation per call, the kernel's chain record) agrees bit for bit with
the iterative statement of tests/nuts_restatement.py in float64 -- state, depth, leapfrog count, divergence, accept statistic,
dsel and next step -- over 2400 transitions of the prior (with warm-up: the divergences at 10 eps0 occur) and 600 + 600 of the
logistic golden case, whitened and plain; (2) on the inputs of tests/test_gpu_nuts_stream.py at most 1 % of the transitions are
too close to call (margin below 1e-9 in long double) and none of the others differs between float64 and long double; (3) the ABI
and the scratch size; (4) the constructor's keyword."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bayesian-coresets_amd", "examples", "common"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import nuts_restatement as nr  # noqa: E402
import nuts_stream_restatement as ns  # noqa: E402
from test_gpu_hmc import _case  # noqa: E402
from test_nuts_host import _frames  # noqa: E402

J, EPS0 = 6, 0.5
CLOSE = 1e-9


def _iterative(tgt, z, nw):
    """The chain by transition_iterative, with what run_chain leaves out (dsel, the next step)."""
    D, dt = tgt.D, tgt.dt
    xi = np.zeros(D, dtype=dt)
    carried = tgt.eval(xi)
    base, hbar, lebar = dt(EPS0), dt(0), dt(0)
    out = []
    for t in range(z.shape[0]):
        r = nr.transition_iterative(tgt, xi, z[t], base, J, carried)
        xi, carried = r["state"], (r["logp"], r["grad"])
        if t < nw:
            base, hbar, lebar = nr.dual_average_alpha(t + 1, r["alpha"], hbar, lebar, EPS0, t + 1 == nw, dt)
        r["base"] = base
        out.append(r)
    return out


@pytest.mark.parametrize("name,C,nw,ns_", (("prior", 8, 150, 150), ("whitened", 5, 60, 60), ("plain", 5, 60, 60)))
def test_resumable_statement_equals_iterative(name, C, nw, ns_):
    family, pts, wts, D, mu, Wm = _frames()[name][:6]
    tgt = nr.Target(family, pts, wts, D, mu, Wm)
    rs = np.random.RandomState(13)
    n = divergent = 0
    depths = []
    for c in range(C):
        z = rs.randn(nw + ns_, nr.noise_columns(D, J))
        want = _iterative(tgt, z, nw)
        chain = ns.run_chain(tgt, z, nw, J, EPS0)
        assert len(chain.out) == len(want) == nw + ns_
        assert chain.rounds == 1 + sum(r["n_leapfrog"] for r in want)        # (one evaluation per leaf and one for the start)
        for t, (a, b) in enumerate(zip(chain.out, want)):
            for q in ("state", "logp", "grad", "alpha", "dsel", "base"):
                assert np.array_equal(a[q], b[q]), (name, c, t, q)
            assert (a["depth"], a["n_leapfrog"], a["divergent"]) == (b["depth"], b["n_leapfrog"], b["divergent"]), (name, c, t)
            assert np.array_equal(a["theta"], tgt.theta(b["state"]))
        n += len(want)
        divergent += sum(r["divergent"] for r in want)
        depths += [r["depth"] for r in want]
    print("%s: %d transitions, depth histogram %s, divergent %d" % (name, n, np.bincount(depths, minlength=J + 1).tolist(), divergent))
    assert n >= (2000 if name == "prior" else 500)
    if name == "prior":
        assert divergent > 0                                   # (the dual averaging's first try at 10 eps0)


@pytest.mark.parametrize("family", ("logistic", "poisson"))
def test_close_calls_on_the_gpu_tests_inputs(family):
    """16 chains x (30 + 30) transitions at J = 6 on the golden cases in their Laplace frame, as the teacher-forced GPU test runs
    them: float64 chains, every transition restarted in long double from the same state, step and noise."""
    import model_lr
    import model_poiss
    gold = np.load(os.path.join(ROOT, "tests", "golden", "mcmc_golden.npz"))
    pts, wts, D = _case(gold, family)
    mu, cov = (model_lr if family == "logistic" else model_poiss).laplace_fit(pts, wts)
    Wm = np.linalg.cholesky(cov).T
    td, tl = nr.Target(family, pts, wts, D, mu, Wm), nr.Target(family, pts, wts, D, mu, Wm, np.longdouble)
    rs = np.random.RandomState(2024)
    total = close = wrong = 0
    smallest = np.inf
    for c in range(16):
        z = rs.randn(60, nr.noise_columns(D, J))
        rec = nr.run_chain(td, z, 30, J, EPS0)
        for t in range(60):
            xi = rec["xi"][t - 1] if t else np.zeros(D)
            r = nr.transition_recursive(tl, xi, z[t], rec["base"][t], J)
            total += 1
            smallest = min(smallest, r["margin"])
            if r["margin"] < CLOSE:
                close += 1
                continue
            wrong += (r["depth"], r["n_leapfrog"], r["divergent"]) != (rec["depth"][t], rec["n_leapfrog"][t], rec["divergent"][t])
    print("%s: %d transitions, %d too close (smallest margin %.3g), %d differ" % (family, total, close, smallest, wrong))
    assert close < 0.01 * total
    assert wrong == 0


def test_abi_lists_the_streamed_nuts():
    from bayesiancoresets_amd import _native
    text = open(os.path.join(ROOT, "include", "bcx.h")).read()
    for name in ("bcx_nuts_stream", "bcx_nuts_stream_scratch_bytes"):
        assert name in _native.SYMBOLS
        assert name + "(" in text
    lib = _native.load()
    vp, i32, i64, dbl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    # bcx_nuts_coreset's arguments with a 64-bit row count, then the scratch and its size
    assert list(lib.bcx_nuts_stream.argtypes) == [vp, i32, i64] + list(lib.bcx_nuts_coreset.argtypes[3:]) + [vp, i64]
    assert lib.bcx_nuts_stream.restype is ctypes.c_int
    sb = lib.bcx_nuts_stream_scratch_bytes
    assert list(sb.argtypes) == [i64, i32, i32, i32] and sb.restype is ctypes.c_int64
    assert dbl in lib.bcx_nuts_stream.argtypes


def test_scratch_bytes():
    from bayesiancoresets_amd import _native
    sb = _native.load().bcx_nuts_stream_scratch_bytes
    for bad in ((-1, 4, 8, 6), (100, 0, 8, 6), (100, 33, 8, 6), (100, 4, 0, 6), (100, 4, 257, 6), (100, 4, 8, 0), (100, 4, 8, 11)):
        assert sb(*bad) == -1, bad
    for N in (0, 1, 129, 3000, 1000000, 1 << 40):
        for D in (1, 10, 32):
            by_chains = [sb(N, D, c, 6) for c in (1, 2, 8, 64, 255, 256)]
            by_depth = [sb(N, D, 16, j) for j in range(1, 11)]
            assert by_chains[0] > 128 and all(b > a for a, b in zip(by_chains, by_chains[1:])), (N, D, by_chains)
            assert all(b > a for a, b in zip(by_depth, by_depth[1:])), (N, D, by_depth)
    rows = [sb(N, 10, 64, 8) for N in (0, 1, 128, 129, 4096, 32768, 1000000, 1 << 40)]
    assert all(b >= a for a, b in zip(rows, rows[1:])) and rows[-1] == rows[-2]      # (a record per workgroup, not per tile)
    assert rows[-1] <= 16 << 20


def test_bad_arguments_are_refused_before_any_launch():
    from bayesiancoresets_amd import _native
    lib = _native.load()
    one, D, C, Jd = ctypes.c_void_p(8), 4, 8, 3                # (never dereferenced: the checks come first)
    R = nr.noise_columns(D, Jd)
    need = lib.bcx_nuts_stream_scratch_bytes(100, D, C, Jd)
    names = ("stream", "family", "N", "D", "w", "Z", "ldz", "mu", "W", "ldw", "chains", "n_warmup", "n_samples", "max_depth", "eps0", "fixed",
             "noise", "noise_ld", "ld", "samples", "xi", "prop", "diag", "accept", "eps", "status", "scratch", "scratch_bytes")
    good = dict(stream=None, family=0, N=100, D=D, w=one, Z=one, ldz=D, mu=one, W=one, ldw=D, chains=C, n_warmup=2, n_samples=2, max_depth=Jd,
                eps0=0.5, fixed=0.0, noise=one, noise_ld=R, ld=D, samples=one, xi=None, prop=None, diag=one, accept=one, eps=one, status=one,
                scratch=one, scratch_bytes=need)
    for kw in (dict(family=2), dict(D=0), dict(D=33, ld=33), dict(max_depth=0), dict(max_depth=11), dict(noise_ld=R - 1), dict(ld=D - 1),
               dict(ld=33), dict(ldw=D - 1), dict(ldz=D - 1), dict(family=1, ldz=D), dict(chains=0), dict(chains=257),
               dict(n_warmup=0, n_samples=0), dict(scratch_bytes=need - 1), dict(scratch=None), dict(N=-1), dict(eps0=0.0)):
        args = [dict(good, **kw)[n] for n in names]
        assert lib.bcx_nuts_stream(*args) == _native.ERR_ARG, kw
        assert b"bcx_nuts_stream" in lib.bcx_project_last_error()


def test_constructor_keyword_needs_no_gpu():
    import bayesiancoresets_amd as bc
    p = inspect.signature(bc.DeviceHMC.__init__).parameters
    assert p["stream"].kind is inspect.Parameter.KEYWORD_ONLY and p["stream"].default is False
    with pytest.raises(ValueError, match="hmc"):
        bc.DeviceHMC("logistic", 4, kernel="hmc", stream=True)
    with pytest.raises(ValueError, match="hmc"):
        bc.DeviceHMC("logistic", 4, stream=True)
