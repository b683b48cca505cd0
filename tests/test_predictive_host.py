"""CPU-only: the yardsticks of the held-out log predictive density.  The plain NumPy restatement
(tests/predictive_restatement.py) in long double -- the referee of the device tests -- and in float64 against the reference's own
table and reduction (tests/golden/predictive_golden.npz), the cases with a closed form, and the compiled kernels' resources."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import predictive_restatement as restate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
CASES = (("lr", "logistic"), ("poiss", "poisson"))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "predictive_golden.npz"))


def _dev(got, want):
    want = np.asarray(want, dtype=np.longdouble)
    return float((np.abs(np.asarray(got, dtype=np.longdouble) - want) / np.maximum(1, np.abs(want))).max())


def test_the_referee_is_wider_than_double():
    assert np.finfo(np.longdouble).eps < 2.0 ** -60


@pytest.mark.parametrize("tag,family", CASES)
@pytest.mark.parametrize("dtype", (np.longdouble, np.float64))
def test_restatement_against_the_reference(gold, tag, family, dtype):
    Z, th, S = gold[tag + "_Z"], gold[tag + "_th"], gold[tag + "_th"].shape[0]
    assert Z.shape[0] == 40 and S == 96
    ll = restate.log_likelihood(family, Z, th, dtype)
    assert ll.dtype == dtype and ll.shape == (40, 96)
    # the table: the generator held the reference to 8 x 2^-52 of the long-double statement; float64 against float64 twice that
    bound = (8 if dtype == np.longdouble else 16) * 2.0 ** -52
    assert _dev(gold[tag + "_ll"], ll) <= bound
    # the reduction: S same-sign terms, the floor of the device test (S + 64) u, for either side's rounding
    lppd, mean = restate.reduce_table(ll)
    d_lppd, d_mean = _dev(gold[tag + "_lppd"], lppd), _dev(gold[tag + "_mean_ll"], mean)
    print("%s %s: lppd %.3g u, mean_ll %.3g u" % (tag, np.dtype(dtype).name, d_lppd / U, d_mean / U))
    assert d_lppd <= 2 * (S + 64) * U and d_mean <= 2 * (S + 64) * U
    assert np.all(np.isfinite(np.asarray(lppd, dtype=np.float64))) and np.all(lppd <= 0)
    assert np.all(mean <= lppd)                                                 # (Jensen)


@pytest.mark.parametrize("family,D", (("logistic", 3), ("poisson", 4)))
@pytest.mark.parametrize("dtype", (np.longdouble, np.float64))
def test_closed_forms(family, D, dtype):
    rs = np.random.RandomState(5)
    X = rs.randn(30, D)
    Z = X if family == "logistic" else np.hstack((X, rs.poisson(2.0, 30)[:, None].astype(np.float64)))
    th = 0.5 * rs.randn(1, D)
    ll = restate.log_likelihood(family, Z, th, dtype)
    eps = float(np.finfo(dtype).eps)
    # one draw: lppd = mean_ll = ll
    lppd, mean = restate.log_predictive(family, Z, th, dtype)
    assert np.array_equal(mean, ll[:, 0]) and _dev(lppd, ll[:, 0]) <= 2 * eps
    # all draws equal: the same
    lppd, mean = restate.log_predictive(family, Z, np.repeat(th, 7, axis=0), dtype)
    assert _dev(lppd, ll[:, 0]) <= 8 * eps and _dev(mean, ll[:, 0]) <= 8 * eps


@pytest.mark.parametrize("dtype", (np.longdouble, np.float64))
def test_a_row_at_minus_800(dtype):
    # logistic, -s >= 100: ll = s exactly; one row, x = 1, every draw -800
    lppd, mean = restate.log_predictive("logistic", np.array([[1.0]]), np.full((50, 1), -800.0), dtype)
    assert lppd[0] == -800 and mean[0] == -800
    # and the table itself handed in: a draw 800 below the best adds an exact zero
    lppd, _ = restate.reduce_table(np.array([[-1.0, -801.0, -1.0, -2000.0]], dtype=dtype))
    assert lppd[0] == dtype(-1.0) + np.log(dtype(2.0) / dtype(4.0))


def test_no_spill_no_scratch_in_any_instantiation():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"),
                          os.path.join(ROOT, "bayesian-coresets_amd", "csrc", "predict.hip")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    print(out.stdout)
    assert lines[-1] == "kernels with spills or scratch: 0"
    rows = [ln for ln in lines if "pred_rows_kernel<" in ln]
    assert len(rows) == 2, lines                                                # (logistic and Poisson)
    assert len([ln for ln in lines if "pred_combine_kernel" in ln]) == 1, lines
    for ln in lines[:-1]:
        assert re.search(r"spill\s+0 scratch\s+0 B", ln), ln
