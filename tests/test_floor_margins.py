"""The decision-margin rule of the CPU oracle (oracle/snnls_oracle.py, record_margins=True) on the oracle's own two modes.
CPU only.

`faithful` recomputes A.dot(w) as the reference does; `onepass` keeps an incremental xw as the device engine does.  Through
the config-1 harness schedule (examples/synthetic_vectors, M up to 1000) the two agree exactly for as long as every
decision is decided by more than twice the proven bound of the state (xw_bound), and may part after that.  The same rule
holds the engine to the oracle in tests/test_gpu_numeric_floor.py, so it is checked here where both sides are known.

Non-vacuity: the decided prefix must reach every iteration whose error is above 1e-7 ||b||.  (1e-9 ||b|| is out of reach
of any bound at or above the rounding that actually happens: GIGA trial 2, iteration 302, error 2.3e-9 ||b||, has a select
gap that a state error of 4 u |A||w| -- what the incremental update really accumulates -- already covers.)"""
import numpy as np
import pytest

from oracle.snnls_oracle import (SnnlsOracle, ST_OK, decided, first_undecided, harness_sizes, run_harness,
                                 synthetic_normal)

CASES = [(t, a) for t in (1, 2, 3) for a in ("giga", "fw", "omp")]
NOT_VACUOUS_BELOW = 1e-7     # the decided prefix covers every iteration with error above this fraction of ||b||


@pytest.fixture(scope="module")
def runs(golden):
    """(trial, alg) -> (faithful oracle with margins, onepass oracle, faithful csize, faithful err); computed once."""
    from conftest import sha256
    cache = {}

    def get(trial, alg):
        if (trial, alg) not in cache:
            X = synthetic_normal(trial, 10000, 100)
            assert sha256(X) == str(golden["F3_t%d_input_sha256" % trial]), "seeded input drifted from the golden digest"
            Ms = harness_sizes()
            assert np.array_equal(Ms, golden["F3_Ms"])
            f = SnnlsOracle(X.T, X.sum(axis=0), alg=alg, mode="faithful", record_margins=True)
            p = SnnlsOracle(X.T, X.sum(axis=0), alg=alg, mode="onepass")
            fc, fe = run_harness(f, Ms)
            run_harness(p, Ms)
            cache[(trial, alg)] = (f, p, fc, fe, float(np.linalg.norm(X.sum(axis=0))))
        return cache[(trial, alg)]

    return get


@pytest.mark.parametrize("trial,alg", CASES)
def test_margins_do_not_change_the_faithful_arithmetic(runs, golden, trial, alg):
    """Recording margins leaves the reference's operation sequence alone: csize, err and the latch equal the reference's
    stored harness run bit for bit (trial 1 is pinned without margins by test_oracle_golden.py; trials 2 and 3 only here)."""
    f, p, fc, fe, bn = runs(trial, alg)
    k = "F3_t%d_%s_" % (trial, alg)
    assert np.array_equal(fc, golden[k + "csize"])
    assert np.array_equal(fe, golden[k + "err"])
    assert f.reached_numeric_limit == bool(golden[k + "limit"])
    assert len(f.margins) == len(f.trace)
    for m in f.margins:
        assert all(np.isfinite(bd) and bd >= 0.0 and sl >= 0.0 for _, sl, bd in m["decisions"]), m


@pytest.mark.parametrize("trial,alg", CASES)
def test_margin_rule_holds_on_the_oracle_modes(runs, trial, alg):
    """Equal picks and statuses (errors to rounding) on every iteration before the first undecided one; the first
    divergence, if any, at or after it."""
    f, p, fc, fe, bn = runs(trial, alg)
    u = first_undecided(f.margins)
    n = min(len(f.trace), len(p.trace))
    div = next((i for i in range(n) if f.trace[i][0] != p.trace[i][0] or f.trace[i][2] != p.trace[i][2]), None)
    if div is None and len(f.trace) != len(p.trace):
        div = n
    print("trial %d %s: decided prefix %d (err %.2e ||b||), first divergence %s, final |dcsize| %d"
          % (trial, alg, u, f.trace[min(u, len(f.trace) - 1)][1] / bn, div, abs(f.size() - p.size())))
    assert u <= len(f.trace)
    assert div is None or div >= u, (div, u, f.margins[div]["decisions"] if div < len(f.margins) else None)
    assert len(p.trace) >= u
    for i in range(u):
        assert f.trace[i][0] == p.trace[i][0] and f.trace[i][2] == p.trace[i][2]
        np.testing.assert_allclose(p.trace[i][1], f.trace[i][1], rtol=1e-9, atol=1e-13 * bn)


@pytest.mark.parametrize("trial,alg", CASES)
def test_margin_rule_is_not_vacuous(runs, trial, alg):
    """The decided prefix reaches every iteration whose error is above NOT_VACUOUS_BELOW ||b|| (FW / GIGA: about iteration
    300 of these runs; OMP: k = d = 100, past which the error is at the floor)."""
    f, p, fc, fe, bn = runs(trial, alg)
    u = first_undecided(f.margins)
    errs = np.array([t[1] for t in f.trace])
    above = np.flatnonzero((errs > NOT_VACUOUS_BELOW * bn) & (np.array([t[2] for t in f.trace]) == ST_OK))
    assert above.size and u > above.max(), (u, above.max())
    assert u >= (95 if alg == "omp" else 250), u


def test_decided_needs_slack_above_twice_the_bound():
    """The rule itself: slack exactly at twice the bound is not decided; an iteration with no decision is."""
    assert not decided({"decisions": [("select", 2.0, 1.0)]})
    assert decided({"decisions": [("select", 2.0000001, 1.0), ("monotone", 1.0, 0.0)]})
    assert not decided({"decisions": [("select", 3.0, 1.0), ("gnum-0", 0.0, 0.0)]})
    assert decided({"decisions": []})
    assert first_undecided([{"decisions": []}, {"decisions": [("s", 1.0, 1.0)]}]) == 1
