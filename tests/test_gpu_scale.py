"""GPU: the greedy engine under a power-of-two scaling of the data, against the CPU oracle run on the SCALED input (the
oracle is exactly equivariant: tests/test_scale_host.py) and against the engine's own run at scale 1.

Every operation of the fp64 state machine is homogeneous in the data, so selections and statuses must not move, the
weights must be bit-equal and the error must scale exactly.  The fp32 / fp16 scan and the 8-bit tier read a fp32 query:
it is stored as q * 2^-E (E the exponent of |q|, csrc/apply_common.h), so neither it nor the scan's error term leaves
fp32's range at any scale -- and no iteration is sent to the fp64 scan because of the scale."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scan_emulation as em  # noqa: E402
from test_gpu_parity import ERR_RTOL, WEIGHT_ATOL_REL, WEIGHT_RTOL  # noqa: E402

pytestmark = pytest.mark.gpu

ERR_ATOL = 1e-9     # test_gpu_parity._check's absolute floor of the error, in units of the unscaled data: OMP on F2 ends at
                    # k = d = 100 columns, where the error (1e-12 of |b|) is the rounding of the final solve
KS = (0, 40, -40, 100, -100, 126, -126, 140, -140, 160, -160, 300, -300)
FIXTURES = {"F9": (7, 3000, 64, "F9_input_sha256", 60), "F2": (1, 10000, 100, "F2_input_sha256", 100)}
# storage type, 8-bit tier (None: fp64 storage has none)
CONFIGS = (("float32", True), ("float32", False), ("float16", True), ("float16", False), ("float64", None))


@pytest.fixture(scope="module")
def bc():
    import bayesiancoresets_amd as bc
    return bc


@pytest.fixture(autouse=True)
def _restore_switch():
    old = os.environ.get("BCX_SCREEN8")
    yield
    if old is None:
        os.environ.pop("BCX_SCREEN8", None)
    else:
        os.environ["BCX_SCREEN8"] = old


def _cls(bc, alg):
    return {"giga": bc.snnls.GIGA, "fw": bc.snnls.FrankWolfe, "omp": bc.snnls.OrthoPursuit}[alg]


def _make(bc, X, alg, dtype, tier, b=None, **kw):
    """The switch of tests/test_gpu_screen8.py: BCX_SCREEN8 is read when a solver is created."""
    if tier is not None:
        os.environ["BCX_SCREEN8"] = "1" if tier else "0"
    s = _cls(bc, alg)(X.T, X.sum(axis=0) if b is None else b, dtype=dtype, **kw)
    if tier is not None:
        assert s._eng.screen_stats()["active"] == bool(tier)
    return s


_oracles, _base = {}, {}


def _oracle(X, fx, alg, k, itrs):
    """The oracle on the scaled input, in the mode the golden F2 / F9 vectors pin (faithful: the reference's own
    operation sequence); one per (fixture, algorithm, scale), shared by the storage configurations."""
    from oracle.snnls_oracle import SnnlsOracle
    key = (fx, alg, k)
    if key not in _oracles:
        Xs = np.ldexp(X, k)
        o = SnnlsOracle(Xs.T, Xs.sum(axis=0), alg=alg, mode="faithful")
        o.build(itrs)
        _oracles[key] = (np.array([t[0] for t in o.trace]), np.array([t[2] for t in o.trace]), o.weights(), o.error(), o)
    return _oracles[key]


def _engine_run(bc, X, fx, alg, dtype, tier, k, itrs):
    s = _make(bc, np.ldexp(X, k), alg, dtype, tier)
    s.build(itrs)
    sel, err, status = s.last_trace
    return {"sel": sel.copy(), "err": err.copy(), "status": status.copy(), "w": s.weights(), "error": s.error(),
            "fallbacks": s._eng.stats()["exact_fallbacks"], "solver": s}


def _first_diff(a, b):
    n = min(len(a), len(b))
    d = np.flatnonzero(np.asarray(a[:n]) != np.asarray(b[:n]))
    return int(d[0]) if d.size else (n if len(a) != len(b) else -1)


def _close_weights(w, ow):
    idx, oidx = np.flatnonzero(w > 0), np.flatnonzero(ow > 0)
    assert np.array_equal(idx, oidx)
    np.testing.assert_allclose(w[idx], ow[oidx], rtol=WEIGHT_RTOL, atol=WEIGHT_ATOL_REL * ow.max())


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("dtype,tier", CONFIGS)
@pytest.mark.parametrize("alg", ("giga", "fw", "omp"))
@pytest.mark.parametrize("fx", ("F9", "F2"))
def test_scaled_build(bc, normal_inputs, fx, alg, dtype, tier, k):
    seed, N, d, key, itrs = FIXTURES[fx]
    X = normal_inputs(seed, N, d, key)
    bkey = (fx, alg, dtype, tier)
    if bkey not in _base:
        r0 = _engine_run(bc, X, fx, alg, dtype, tier, 0, itrs)
        r0.pop("solver")
        _base[bkey] = r0
    r0 = _base[bkey]
    r = _engine_run(bc, X, fx, alg, dtype, tier, k, itrs)
    osel, ostatus, ow, oerr, _ = _oracle(X, fx, alg, k, itrs)
    print("scale", fx, alg, dtype, tier, k, "first differing iteration vs oracle:", _first_diff(r["sel"], osel),
          "vs k=0:", _first_diff(r["sel"], r0["sel"]), "fallbacks", r["fallbacks"], "(k=0:", r0["fallbacks"], ")",
          "error * 2^-k", np.ldexp(r["error"], -k), "oracle", np.ldexp(oerr, -k))
    # against the oracle on the scaled input
    assert np.array_equal(r["sel"], osel), "selection differs from the oracle's at iteration %d" % _first_diff(r["sel"], osel)
    assert np.array_equal(r["status"], ostatus)
    _close_weights(r["w"], ow)
    np.testing.assert_allclose(np.ldexp(r["error"], -k), np.ldexp(oerr, -k), rtol=ERR_RTOL, atol=ERR_ATOL)
    # against the engine's own run at scale 1
    assert np.array_equal(r["sel"], r0["sel"]) and np.array_equal(r["status"], r0["status"])
    assert np.array_equal(r["w"], r0["w"]), "weights are not bit-equal to the run at scale 1"
    assert r["error"] == np.ldexp(r0["error"], k)
    assert np.array_equal(r["err"], np.ldexp(r0["err"], k))
    assert r["fallbacks"] <= r0["fallbacks"], "the scale sent iterations to the exact fp64 scan"


@pytest.mark.parametrize("k", (140, -140))
@pytest.mark.parametrize("dtype,tier", (("float32", True), ("float16", True), ("float64", None)))
@pytest.mark.parametrize("alg", ("giga", "fw", "omp"))
def test_scaled_optimize(bc, normal_inputs, alg, dtype, tier, k):
    """optimize() after the scaled build: weights and error against the oracle's re-solve on the scaled input."""
    seed, N, d, key, itrs = FIXTURES["F9"]
    X = normal_inputs(seed, N, d, key)
    r = _engine_run(bc, X, "F9", alg, dtype, tier, k, itrs)
    from oracle.snnls_oracle import SnnlsOracle
    Xs = np.ldexp(X, k)
    o = SnnlsOracle(Xs.T, Xs.sum(axis=0), alg=alg, mode="faithful")
    o.build(itrs)
    assert np.array_equal(r["sel"], np.array([t[0] for t in o.trace]))
    s = r["solver"]
    s.optimize()
    o.optimize()
    print("optimize", alg, dtype, k, np.ldexp(s.error(), -k), np.ldexp(o.error(), -k))
    _close_weights(s.weights(), o.weights())
    np.testing.assert_allclose(np.ldexp(s.error(), -k), np.ldexp(o.error(), -k), rtol=ERR_RTOL, atol=ERR_ATOL)


def _fw_engine(bc, X, dtype):
    """A Frank-Wolfe handle as coreset/sparsevi.py _engine_for makes it."""
    from bayesiancoresets_amd import _native as nat
    store = {"float32": nat.F32, "float16": nat.F16, "float64": nat.F64}[dtype]
    eng = nat.Engine(nat.ALG_FW, X.shape[0], X.shape[1], store_dtype=store, keep_exact_rows=True)
    eng.use_current_stream()
    eng.load_rows_any(np.ascontiguousarray(X))
    assert eng.finalize(None) == nat.OK
    return eng


@pytest.mark.parametrize("dtype", ("float32", "float16", "float64"))
def test_argmax_correlation_scaled_query(bc, normal_inputs, dtype):
    """bcx_argmax_correlation with the query scaled by 2^k, and with a query whose elements span 2^-60 .. 2^60: index and
    score * 2^-k against the long-double reference."""
    X = normal_inputs(7, 3000, 64, "F9_input_sha256")
    eng = _fw_engine(bc, X, dtype)
    rs = np.random.RandomState(5)
    q = rs.randn(64)
    ex = em.exact_scores(X, q)
    for k in KS:
        row, score = eng.argmax_correlation(np.ldexp(q, k))
        print("argmax", dtype, k, row, np.ldexp(score, -k), float(ex.max()))
        assert row == em.first_argmax(ex), (dtype, k)
        np.testing.assert_allclose(np.ldexp(score, -k), float(ex.max()), rtol=1e-12)
    wide = q * np.exp2(rs.uniform(-60, 60, size=64))
    exw = em.exact_scores(X, wide)
    for k in (0, 140, -140):
        row, score = eng.argmax_correlation(np.ldexp(wide, k))
        assert row == em.first_argmax(exw), (dtype, k)
        np.testing.assert_allclose(np.ldexp(score, -k), float(exw.max()), rtol=1e-12)
    eng.close()


def test_project_select_scaled_residual(bc):
    """DeviceProjector.project_select (fp64 kernel) with the residual scaled: same row, score scaled."""
    from oracle.sparsevi_oracle import linreg_loglik
    rs = np.random.RandomState(4)
    Z, theta, resid = rs.randn(3000, 21), rs.randn(64, 20), rs.randn(64)
    vecs = linreg_loglik(Z, theta, 0.8)
    vecs -= vecs.mean(axis=1)[:, None]
    ex = em.exact_scores(vecs, resid) / 64
    prj = bc.DeviceProjector("linreg", lambda n, w, p: theta, 64, sigsq=0.8)
    for k in (0, 140, -140, 300, -300):
        best, row = prj.project_select(Z, np.ldexp(resid, k))
        assert row == em.first_argmax(ex), k
        np.testing.assert_allclose(np.ldexp(best, -k), float(ex.max()), rtol=1e-8)


@pytest.mark.parametrize("k", (140, -140))
def test_no_exact_rows_mode_scaled(bc, golden, normal_inputs, k):
    """keep_exact_rows=False (test_gpu_parity.test_no_exact_rows_mode): the stored rows are all there is, so a
    low-precision score may be final -- it has to come back in the caller's scale.  Frank-Wolfe, same checks as at scale 1,
    the weights against the oracle on the scaled input."""
    X = normal_inputs(7, 3000, 64, "F9_input_sha256")
    Xs = np.ldexp(X, k)
    s = _cls(bc, "fw")(Xs.T, Xs.sum(axis=0), keep_exact_rows=False)
    s.build(60)
    sel = s.last_trace[0]
    assert np.array_equal(sel[sel >= 0], golden["F9_fw_sel"])
    w = s.weights()
    idx = np.flatnonzero(w > 0)
    assert np.array_equal(idx, golden["F9_fw_idx"])
    np.testing.assert_allclose(w[idx], golden["F9_fw_w"], rtol=1e-4)
    np.testing.assert_allclose(np.ldexp(s.error(), -k), float(golden["F9_fw_final_err"]), rtol=1e-4)
    # 100 copies of each of 10 rows: the candidate window overflows, and without resident fp64 rows the retry's score is the
    # fp32 scan's own upper bound -- within twice the scan's error term (bcx_scan_plan: d = 64 is G = 16, CH = 1) of the
    # exact score, in the caller's scale
    Y = np.tile(np.random.RandomState(9).randn(10, 64), (100, 1))
    q = np.random.RandomState(10).randn(64)
    t = _cls(bc, "fw")(np.ldexp(Y, k).T, np.ldexp(Y, k).sum(axis=0), keep_exact_rows=False)
    row, score = t._eng.argmax_correlation(np.ldexp(q, k))
    ex = em.exact_scores(Y, q)
    assert row == em.first_argmax(ex)
    bound = 2.0 * (1.3 * 2.0 ** -24 * (4 * 1 + 4 + 3.0) + 2e-7) * float(np.sqrt((q * q).sum()))
    assert abs(np.ldexp(score, -k) - float(ex.max())) <= bound, (np.ldexp(score, -k), float(ex.max()), bound)
