"""GPU: examples/logistic_poisson_regression/main.py `--eval mcmc --mcmc_test_rows K` holds out the last K rows
before anything is fitted or built and adds the columns `test_ll` / `full_test_ll` -- the mean log predictive density of the
held-out rows under every coreset's and under the full data's draws (bc.log_predictive) -- with and without `--mcmc_batch`;
without the flag the run and its result file are what they were.  The harness runs in this process."""
import importlib.util
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "bayesian-coresets_amd", "examples", "logistic_poisson_regression", "main.py")
sys.path.insert(0, os.path.join(ROOT, "bayesian-coresets_amd", "examples", "common"))

pytestmark = pytest.mark.gpu

BASE = ["--model", "lr", "--dataset", "synth_lr", "--alg", "GIGA-OPT", "--trial", "1", "--data_num", "600", "--data_dim", "3",
        "--proj_dim", "64", "--coreset_size_max", "50", "--coreset_num_sizes", "3", "--mcmc_samples_full", "1000",
        "--mcmc_samples_coreset", "1000"]
MCMC = ["--eval", "mcmc", "--mcmc_kernel", "nuts"]


@pytest.fixture(scope="module")
def main():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    spec = importlib.util.spec_from_file_location("_lpr_main_predictive", SCRIPT)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _run(main, folder, *more):
    """One trial in this process; the name of the result file it added to `folder`."""
    before = set(os.listdir(folder)) if os.path.isdir(folder) else set()
    args = main.parser().parse_args(BASE + ["--results_folder", folder] + list(more) + ["run"])
    args.func(args)
    new = [f for f in os.listdir(folder) if f.endswith(".csv") and f != "manifest.csv" and f not in before]
    assert len(new) == 1, new
    return new[0]


@pytest.fixture(scope="module")
def trials(main, tmp_path_factory):
    import pandas as pd
    folder = str(tmp_path_factory.mktemp("predictive")) + "/"
    plain = _run(main, folder, *MCMC, "--mcmc_test_rows", "100")
    batched = _run(main, folder, *MCMC, "--mcmc_test_rows", "100", "--mcmc_batch")
    assert plain != batched
    return folder, pd.read_csv(os.path.join(folder, plain)), pd.read_csv(os.path.join(folder, batched))


def test_the_two_columns(trials):
    _, t, _ = trials
    assert len(t) == 3 and (t["mcmc_test_rows"] == 100).all() and t["Ms"].is_monotonic_increasing
    for col in ("test_ll", "full_test_ll"):
        assert col in t.columns and np.isfinite(t[col]).all() and (t[col] < 0).all(), col
    assert t["full_test_ll"].nunique() == 1
    # a larger coreset predicts the held-out rows more like the full data does: a condition, not a threshold.  Observed on an
    # MI355X with this seed (Ms = 1, 7, 49): test_ll -0.021020, -0.007648, -0.008118 against full_test_ll -0.007861 -- 0.00026
    # from it at the largest size, 0.01316 at size 1, a factor of 51
    full, first, last = t["full_test_ll"].iloc[0], t["test_ll"].iloc[0], t["test_ll"].iloc[-1]
    print("test_ll %s, full_test_ll %.6f" % (list(t["test_ll"]), full))
    assert abs(last - full) < abs(first - full)


def test_the_batch_gives_the_same_columns(trials):
    _, plain, batched = trials
    assert "mcmc_batch" not in plain.columns and batched["mcmc_batch"].all()
    # (as tests/test_gpu_nuts_batch_harness.py: every column but the sampler's time and the two runs' own construction clocks)
    for col in plain.columns:
        if col not in ("mcmc_time_per_itr", "cputs", "walls"):
            assert plain[col].equals(batched[col]), col
    assert batched["test_ll"].equals(plain["test_ll"]) and batched["full_test_ll"].equals(plain["full_test_ll"])


def test_without_the_flag_nothing_changes(main, trials):
    import pandas as pd
    import results
    folder, flagged, _ = trials
    name = _run(main, folder, *MCMC)
    # the file name is the hash of the argument set as it was before the flag existed: no `mcmc_test_rows` entry
    args = vars(main.parser().parse_args(BASE + ["--results_folder", folder] + MCMC + ["run"]))
    assert "mcmc_test_rows" not in args
    assert name == results.hash_namespace(args) + ".csv"
    t = pd.read_csv(os.path.join(folder, name))
    for col in ("mcmc_test_rows", "test_ll", "full_test_ll"):
        assert col not in t.columns
    assert [c for c in flagged.columns if c not in t.columns] == ["mcmc_test_rows", "test_ll", "full_test_ll"]
    # all 600 rows were the data: a full-data cache of its own, next to the one of the 500 rows
    assert sorted(os.listdir(os.path.join(folder, "mcmc_cache"))) == ["full_samples_lr_synth_lr_600_3_1_1000.npz",
                                                                      "full_samples_lr_synth_lr_600_3_1_1000_t100.npz"]


def test_the_flag_goes_with_the_mcmc_evaluation(main, tmp_path):
    folder = str(tmp_path / "r") + "/"
    for more in (("--mcmc_test_rows", "100"), ("--mcmc_test_rows", "100", "--eval", "laplace")):
        with pytest.raises(ValueError, match="--mcmc_test_rows goes with --eval mcmc"):
            _run(main, folder, *more)
    with pytest.raises(ValueError, match="hold out"):
        _run(main, folder, *MCMC, "--mcmc_test_rows", "600")
    assert not os.path.exists(folder) or not [f for f in os.listdir(folder) if f.endswith(".csv")]
