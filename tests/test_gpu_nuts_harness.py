"""GPU: the harness side of the NUTS kernel.  examples/common/mcmc.py `run(..., kernel="nuts")` uses it where the rows fit its
LDS-resident path and falls back to HMC where they do not, and says which ran; examples/logistic_poisson_regression/main.py
`--eval mcmc --mcmc_kernel nuts` runs one trial end to end under a result-file name of its own."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "bayesian-coresets_amd", "examples", "logistic_poisson_regression", "main.py")
sys.path.insert(0, os.path.join(ROOT, "bayesian-coresets_amd", "examples", "common"))

pytestmark = pytest.mark.gpu


def test_run_says_which_kernel_ran():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mcmc
    import model_lr
    Z = model_lr.synthetic_rows(24000, 3, np.random.RandomState(2))
    w = np.random.RandomState(3).uniform(1.0, 20.0, 50)
    s, t, ran = mcmc.run(Z[:50], w, 640, "lr", 1, kernel="nuts", max_depth=6)
    assert ran == "nuts" and s.shape == (640, 3) and np.all(np.isfinite(s)) and t > 0
    s, t, ran = mcmc.run(Z, None, 64, "lr", 1, kernel="nuts")              # past one workgroup's LDS: the streamed HMC
    assert ran == "hmc" and s.shape == (64, 3) and np.all(np.isfinite(s))
    s, t, ran = mcmc.run(Z[:50], w, 64, "lr", 1)
    assert ran == "hmc"


def test_one_trial_end_to_end(tmp_path):
    import pandas as pd
    folder = str(tmp_path / "r") + "/"
    cmd = [sys.executable, SCRIPT, "--model", "lr", "--dataset", "synth_lr", "--alg", "GIGA-OPT", "--trial", "1", "--data_num", "3000",
           "--data_dim", "4", "--proj_dim", "64", "--coreset_size_max", "30", "--coreset_num_sizes", "2", "--mcmc_samples_full", "1000",
           "--mcmc_samples_coreset", "1000", "--results_folder", folder, "--eval", "mcmc", "--mcmc_kernel", "nuts", "run"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    files = [f for f in os.listdir(folder) if f.endswith(".csv") and f != "manifest.csv"]
    assert len(files) == 1, files
    tab = pd.read_csv(os.path.join(folder, files[0]))
    assert (tab["mcmc_kernel"] == "nuts").all() and (tab["eval"] == "mcmc").all()
    for col in ("Fs", "mcmc_time_per_itr", "rklw", "fklw", "mu_errs", "Sig_errs"):
        assert np.isfinite(tab[col]).all(), col
    assert (tab["mcmc_time_per_itr"] > 0).all()
