"""GPU: the harness side of the batched NUTS launch.  examples/common/mcmc.py `run_many` returns per problem what
`run` returns -- the draws bit for bit, the kernel that ran -- with one launch for the problems that fit the LDS-resident NUTS and
`run`'s fallbacks for the others; examples/logistic_poisson_regression/main.py `--mcmc_batch` scores every size behind the build
and saves the unbatched trial's columns, `mcmc_time_per_itr` excepted."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "bayesian-coresets_amd", "examples", "logistic_poisson_regression", "main.py")
sys.path.insert(0, os.path.join(ROOT, "bayesian-coresets_amd", "examples", "common"))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rows():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import model_lr
    return model_lr.synthetic_rows(24000, 3, np.random.RandomState(2))


@pytest.mark.parametrize("metric", (None, "dense"))
def test_run_many_equals_run(rows, metric):
    import mcmc
    rs = np.random.RandomState(3)
    problems = [(rows[a:a + k], rs.uniform(1.0, 20.0, k)) for a, k in ((0, 3), (100, 50), (200, 17))]
    kw = dict(kernel="nuts", max_depth=5, chains=16, adapt_metric=metric)
    got = mcmc.run_many(problems, 320, "lr", 1, **kw)
    assert len(got) == 3
    for (Z, w), (s, t, ran) in zip(problems, got):
        s0, t0, ran0 = mcmc.run(Z, w, 320, "lr", 1, **kw)
        assert ran == ran0 == "nuts" and s.shape == (320, 3) and t > 0
        assert np.array_equal(s, s0)
    assert got[0][1] == got[1][1] == got[2][1]                                  # (one launch's time over its three problems)


def test_a_problem_past_the_lds_takes_the_fallback(rows):
    import mcmc
    w = np.random.RandomState(4).uniform(1.0, 20.0, 40)
    problems = [(rows[:40], w), (rows, None)]
    got = mcmc.run_many(problems, 64, "lr", 1, kernel="nuts", max_depth=5, chains=16, adapt_metric="diag")
    assert [ran for _, _, ran in got] == ["nuts", "hmc"]
    for (Z, wts), (s, t, ran) in zip(problems, got):
        s0, _, ran0 = mcmc.run(Z, wts, 64, "lr", 1, kernel="nuts", max_depth=5, chains=16, adapt_metric="diag")
        assert ran == ran0 and np.array_equal(s, s0)
    with pytest.raises(ValueError, match="no rows|without rows"):
        mcmc.run_many([(rows[:0], None)], 64, "lr", 1)
    with pytest.raises(ValueError, match="nuts"):
        mcmc.run_many(problems[:1], 64, "lr", 1, kernel="hmc", adapt_metric="dense")


def _trial(folder, *more):
    cmd = [sys.executable, SCRIPT, "--model", "lr", "--dataset", "synth_lr", "--alg", "GIGA-OPT", "--trial", "1", "--data_num", "3000",
           "--data_dim", "4", "--proj_dim", "64", "--coreset_size_max", "30", "--coreset_num_sizes", "3", "--mcmc_samples_full", "1000",
           "--mcmc_samples_coreset", "1000", "--results_folder", folder, "--eval", "mcmc"] + list(more) + ["run"]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=600)


def test_one_trial_with_and_without_the_batch(tmp_path):
    import pandas as pd
    folder = str(tmp_path / "r") + "/"
    tabs = {}
    for more in ((), ("--mcmc_batch",)):
        out = _trial(folder, "--mcmc_kernel", "nuts", *more)
        assert out.returncode == 0, out.stderr[-3000:]
        files = sorted(f for f in os.listdir(folder) if f.endswith(".csv") and f != "manifest.csv")
        new = [f for f in files if f not in tabs]
        assert len(new) == 1, files                                             # (a result file of its own)
        tabs[new[0]] = pd.read_csv(os.path.join(folder, new[0]))
    plain, batched = [tabs[f] for f in tabs]
    assert "mcmc_batch" not in plain.columns and batched["mcmc_batch"].all()
    assert len(plain) == len(batched) == 3
    # every argument and result column but the sampler's time; cputs / walls are the two processes' own construction clocks, which
    # no two runs share (full_mcmc_time_per_itr is the cached full-data run's and is compared)
    for col in plain.columns:
        if col not in ("mcmc_time_per_itr", "cputs", "walls"):
            assert plain[col].equals(batched[col]), col
    assert (batched["mcmc_time_per_itr"] > 0).all() and batched["mcmc_time_per_itr"].nunique() == 1


def test_the_flag_goes_with_the_nuts_kernel(tmp_path):
    folder = str(tmp_path / "r") + "/"
    for more in (("--mcmc_batch",), ("--mcmc_batch", "--mcmc_kernel", "hmc")):
        out = _trial(folder, *more)
        assert out.returncode != 0 and "--mcmc_batch goes with --eval mcmc --mcmc_kernel nuts" in out.stderr
    assert not os.path.exists(folder) or not [f for f in os.listdir(folder) if f.endswith(".csv")]
