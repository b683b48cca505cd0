"""CPU: (1) the oracle -- the referee of tests/test_gpu_scale.py -- is exactly equivariant under a power-of-two scaling of
the data, as the reference's arithmetic is: same selections and statuses, bit-identical weights, error scaled exactly;
(2) the adversarial inputs of tests/test_gpu_scan_enclosure.py meet their preconditions (tests/scan_emulation.py), shown
here at two row lengths per storage type without a GPU; (3) the restated launch plan reaches every variant the GPU file
claims to reach."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scan_emulation as em  # noqa: E402
from oracle.snnls_oracle import SnnlsOracle  # noqa: E402


def _run_oracle(X, alg, itrs):
    o = SnnlsOracle(X.T, X.sum(axis=0), alg=alg, mode="faithful")
    o.build(itrs)
    return o


@pytest.mark.parametrize("alg", ("giga", "fw", "omp"))
@pytest.mark.parametrize("k", (-300, 300))
def test_oracle_is_exactly_equivariant(alg, k):
    """randn data, N = 3000, d = 64, 60 iterations, scaled by 2^k (np.ldexp: exact)."""
    X = np.random.RandomState(7).randn(3000, 64)
    o0, ok = _run_oracle(X, alg, 60), _run_oracle(np.ldexp(X, k), alg, 60)
    assert [t[0] for t in o0.trace] == [t[0] for t in ok.trace]
    assert [t[2] for t in o0.trace] == [t[2] for t in ok.trace]
    assert np.array_equal(o0.weights(), ok.weights())
    assert ok.error() == np.ldexp(o0.error(), k)
    assert np.array_equal(np.array([t[1] for t in ok.trace]), np.ldexp(np.array([t[1] for t in o0.trace]), k))


HOST_D = {"float32": (33, 4097), "float16": (100, 1025), "float64": (9, 2049)}


@pytest.mark.parametrize("storage", em.STORAGES)
@pytest.mark.parametrize("which", (0, 1))
def test_adversarial_inputs_meet_their_preconditions(storage, which):
    d = HOST_D[storage][which]
    N = 1000 if d < 1000 else 130
    rpb = em.scan_plan(d, storage)["rpb"]
    for M, winner, dup in ((3, 0, False), (40, N - 1, False), (em.MAX_CAND + 16, min(rpb + 1, N - 1), False),
                           (40, max(rpb - 1, 0), True)):
        X, q, info = em.cluster_case(d, storage, N, M, winner, seed=d + M, duplicate=dup)
        em.check_cluster(X, q, storage, info)
        assert not dup or info["dup"] is not None
    if storage != "float64":
        X, q, info = em.aligned_case(d, storage, N, N // 2, seed=d)
        em.check_aligned(X, q, storage, info)
        # nearly the full resolution: the stored order is off by more than half of resolution * |q|
        st = em.stored_scores(X, q, storage)
        assert st[info["runner"]] - st[info["winner"]] > 0.5 * em.RESOLUTION[storage] * np.sqrt((q * q).sum())
    if storage == "float16":
        X, q, info = em.subnormal_case(d, N, N // 3, seed=d)
        em.check_subnormal(X, q, info)
    X, q = em.negative_case(d, N, seed=d)
    ex = em.exact_scores(X, q)
    assert (ex < 0).all()
    X, q = em.padzero_case(d, storage, N, seed=d)
    assert q[-1] == 0.0 and np.any(q)


def test_short_rows_meet_their_preconditions():
    """d = 3, 4, 5: the shortest rows the aligned and subnormal constructions take."""
    for d in (3, 4, 5):
        for storage in ("float32", "float16"):
            X, q, info = em.aligned_case(d, storage, 63, 62, seed=d)
            em.check_aligned(X, q, storage, info)
            X, q, info = em.cluster_case(d, storage, 63, 40, 0, seed=d)
            em.check_cluster(X, q, storage, info)
    X, q, info = em.subnormal_case(5, 63, 7, seed=5)
    em.check_subnormal(X, q, info)


def test_stored_scores_follow_the_scale_of_the_query():
    """The emulation stores the query as q * 2^-E: its stored score is exactly equivariant too."""
    rs = np.random.RandomState(3)
    X, q = rs.randn(50, 37), rs.randn(37)
    for storage in ("float32", "float16"):
        s0 = em.stored_scores(X, q, storage)
        for k in (-300, -160, 140, 300):
            assert np.array_equal(em.stored_scores(X, np.ldexp(q, k), storage), np.ldexp(s0, k))


def test_plan_reaches_every_variant():
    """The row lengths of tests/test_gpu_scan_enclosure.py reach every group width, every chunk count of the register
    kernel, the ragged and deep doublings and the long-row kernel for each storage type."""
    for storage in em.STORAGES:
        plans = [em.scan_plan(d, storage) for d in em.D_LIST]
        assert {p["G"] for p in plans} == {1, 2, 4, 8, 16, 32, 64}
        assert {p["CH"] for p in plans if not p["long_rows"]} == {1, 2, 4, 8, 16}
        assert any(p["ragged"] and p["deep"] for p in plans) and any(p["deep"] and not p["ragged"] for p in plans)
        assert any(p["long_rows"] for p in plans) and any(p["UR"] == 8 for p in plans)
    assert any(p["ragged"] and not p["deep"] for p in (em.scan_plan(d, "float32") for d in em.D_LIST))
