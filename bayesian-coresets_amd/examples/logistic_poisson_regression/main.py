#!/usr/bin/env python3
"""Logistic / Poisson regression coreset experiment on the device engine (BASELINE.json configs[2] names this harness),
command-line compatible with the reference's examples/logistic_poisson_regression/main.py:232-289 for the `run` sub-command:

    python main.py --model lr --dataset synth_lr --alg GIGA-OPT --proj_dim 500 --coreset_size_max 1000 run
    python main.py --model poiss --dataset synth_poiss --alg SVI --opt_itrs 100 run

Construction follows main.py:66-185: the model (`lr`: rows y x, `poiss`: rows [x, y] with a softplus rate), the three
projectors -- `GIGA-OPT` samples from the Laplace approximation of the full-data posterior, `GIGA-REAL` from that of a
sqrt(N)-point subsample, `SVI` from the Laplace approximation of the weighted coreset, refreshed at every step -- the
incremental build over the size schedule, and `US` as the uniform baseline.  The projections run on the GPU
(bc.DeviceProjector "logistic" / "poisson"), the greedy construction on the device engine.
`--dataset synth_lr | synth_poiss` generates the data (`--data_num` rows, `--data_dim` columns); a path to an .npz with
arrays X, y (the reference's data/*.npz layout, last column of X the intercept) is standardised as load_data does.
The reference evaluates a coreset by Stan MCMC on it (main.py:107-127, 205-232).  `--eval laplace` (the default) reports the
metric columns -- reverse / forward KL to the full-data posterior, relative errors of mean and covariance -- between the
LAPLACE approximations of the coreset posterior and of the full-data posterior.  `--eval mcmc` samples both posteriors with
bc.DeviceHMC (examples/common/mcmc.py; `--mcmc_samples_full` / `--mcmc_samples_coreset` draws, the full-data draws cached under
<results_folder>/mcmc_cache), takes the Gaussian moments of the draws for the same columns and adds the reference's others: `Fs`
(the mean squared difference of the coreset's and the full data's log-joint gradients over the full-data draws, two
bc.log_joint_grad calls), `full_mcmc_time_per_itr`, `mcmc_time_per_itr`.  `--mcmc_kernel nuts` samples every coreset's posterior
with the No-U-Turn transition (bc.DeviceHMC(kernel="nuts"): Stan's sampler; a coreset past one workgroup's LDS falls back to HMC);
the full-data chain stays HMC.  `--mcmc_kernel nuts --mcmc_nuts_stream`: coresets past the LDS and the full-data chain run the
streamed NUTS (bc.DeviceHMC(kernel="nuts", stream=True)); the full-data cache file then carries the kernel in its name.  `--mcmc_kernel nuts --mcmc_adapt_metric diag|dense`: every coreset
that fits the adapting LDS-resident NUTS learns a metric in its windowed warm-up; the others run as without it.
`--mcmc_kernel nuts --mcmc_batch`: the coresets of all sizes are kept during the build and scored after it by one
mcmc.run_many -- ONE launch for all that fit the LDS-resident NUTS; every column is the unbatched run's but
`mcmc_time_per_itr`, which is the launch's time over the coresets in it.
`--eval mcmc --mcmc_test_rows K`: the last K rows of the loaded data are held out before anything is fitted or built, and two
columns score the draws on them by bc.log_predictive: `test_ll`, the mean over the held-out rows of the log
predictive density under the draws of every coreset size (the prior draws for an empty coreset), and `full_test_ll`, the same
under the full-data draws.
`--eval mcmc --mcmc_discrepancy K`: three columns that compare the draws themselves, not their moments, each side
thinned evenly to at most K draws, in the frame of the full-data draws (mu their mean, W = L^T with L L^T their covariance):
`energy`, the squared energy distance between every coreset's draws and the full-data draws (bc.energy_distance(...).value);
`ksd`, the IMQ kernel Stein discrepancy of every coreset's draws under the FULL-data score (bc.stein_discrepancy with
family / pts = the full data); `full_ksd`, the same of the full-data draws themselves."""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(1, os.path.join(HERE, "..", "common"))
import results  # noqa: E402
import mcmc  # noqa: E402
import model_lr  # noqa: E402
import model_poiss  # noqa: E402


def gaussian_kl(mu0, Sig0, mu1, Sig1inv):
    """KL(N(mu0, Sig0) || N(mu1, Sig1)) (model_gaussian.py KL: the metric of main.py:226-227)."""
    diff = mu1 - mu0
    return 0.5 * (np.trace(Sig1inv.dot(Sig0)) + diff.dot(Sig1inv).dot(diff)
                  - np.linalg.slogdet(Sig1inv)[1] - np.linalg.slogdet(Sig0)[1] - mu0.shape[0])


def load(a, rs):
    """Z (rows as the model wants them) for the data set named on the command line."""
    if os.path.exists(a.dataset):
        d = np.load(a.dataset)
        X, y = model_poiss.standardized(d["X"]), np.asarray(d["y"], dtype=np.float64)
        return y[:, None] * X if a.model == "lr" else np.hstack((X, y[:, None]))
    if a.model == "lr":
        Zx = model_lr.synthetic_rows(a.data_num, a.data_dim - 1, rs)          # y x
        y = np.sign(Zx[:, :1] / np.where(Zx[:, :1] == 0.0, 1.0, Zx[:, :1]))   # (recover y to append the intercept column y * 1)
        return np.hstack((Zx, y))
    return model_poiss.synthetic_rows(a.data_num, a.data_dim, rs)


def full_data_samples(a, Z, nuts_stream=False, held_out=0):
    """The full-data draws and the sampler's time per iteration, cached per model / data set / trial (main.py:107-127) -- and per
    kernel when the full-data chain is the streamed NUTS: a cached HMC run is never read as a NUTS one, nor the reverse -- and per
    number of held-out rows (--mcmc_test_rows), which are not part of the full data."""
    folder = os.path.join(a.results_folder, "mcmc_cache")
    name = "full_samples_%s_%s_%d_%d_%d_%d%s.npz" % (a.model, os.path.basename(a.dataset), a.data_num, a.data_dim, a.trial, a.mcmc_samples_full,
                                                     ("_nuts" if nuts_stream else "") + ("_t%d" % held_out if held_out else ""))
    path = os.path.join(folder, name)
    if os.path.exists(path):
        d = np.load(path)
        return d["samples"], float(d["t"])
    if nuts_stream:
        samples, t, ran = mcmc.run(Z, None, a.mcmc_samples_full, a.model, a.trial, kernel="nuts", nuts_stream=True)
        print("full-data chain: %s" % ran)
    else:
        samples, t, _ = mcmc.run(Z, None, a.mcmc_samples_full, a.model, a.trial)
    t_per_itr = t / (a.mcmc_samples_full * 2)                                  # (main.py:123-124: warm-up = sampling)
    os.makedirs(folder, exist_ok=True)
    np.savez(path, samples=samples, t=t_per_itr)
    return samples, t_per_itr


def run(a):
    use_mcmc = getattr(a, "eval", "laplace") == "mcmc"
    if not use_mcmc and hasattr(a, "eval"):
        delattr(a, "eval")              # (the default evaluation's result files keep the argument set they always had)
    mcmc_kernel = getattr(a, "mcmc_kernel", "hmc")
    if mcmc_kernel == "hmc" and hasattr(a, "mcmc_kernel"):
        delattr(a, "mcmc_kernel")       # (likewise, given explicitly: the default sampler's result files keep their names)
    nuts_stream = bool(getattr(a, "mcmc_nuts_stream", False))      # (absent unless given: the parser suppresses its default)
    if nuts_stream and not (use_mcmc and mcmc_kernel == "nuts"):
        raise ValueError("--mcmc_nuts_stream goes with --eval mcmc --mcmc_kernel nuts")
    adapt_metric = getattr(a, "mcmc_adapt_metric", None)           # (absent unless given: the parser suppresses its default)
    if adapt_metric is not None and not (use_mcmc and mcmc_kernel == "nuts"):
        raise ValueError("--mcmc_adapt_metric goes with --eval mcmc --mcmc_kernel nuts")
    batch = bool(getattr(a, "mcmc_batch", False))                  # (absent unless given: the parser suppresses its default)
    if batch and not (use_mcmc and mcmc_kernel == "nuts"):
        raise ValueError("--mcmc_batch goes with --eval mcmc --mcmc_kernel nuts")
    test_rows = getattr(a, "mcmc_test_rows", None)                 # (absent unless given: the parser suppresses its default)
    if test_rows is not None and not use_mcmc:
        raise ValueError("--mcmc_test_rows goes with --eval mcmc")
    if test_rows is not None and test_rows < 1:
        raise ValueError("--mcmc_test_rows: at least one row")
    disc = getattr(a, "mcmc_discrepancy", None)                    # (absent unless given: the parser suppresses its default)
    if disc is not None and not use_mcmc:
        raise ValueError("--mcmc_discrepancy goes with --eval mcmc")
    if disc is not None and disc < 2:
        raise ValueError("--mcmc_discrepancy: at least two draws a side")
    stream = bool(getattr(a, "laplace_stream", False))     # (absent unless given: the parser suppresses its default)
    if results.check_exists(a, a.results_folder):
        print("Results already exist for arguments " + str(a))
        print("Quitting.")
        return
    import bayesiancoresets_amd as bc
    np.random.seed(a.trial)
    bc.util.set_verbosity(a.verbosity)
    if a.coreset_size_spacing == "log":
        Ms = np.unique(np.logspace(0.0, np.log10(a.coreset_size_max), a.coreset_num_sizes, dtype=np.int32))
    else:
        Ms = np.unique(np.linspace(1, a.coreset_size_max, a.coreset_num_sizes, dtype=np.int32))
    Z = load(a, np.random)
    Zt = None
    if test_rows is not None:                                                  # held out before anything is fitted or built
        if test_rows >= Z.shape[0]:
            raise ValueError("--mcmc_test_rows: %d rows to hold out of %d" % (test_rows, Z.shape[0]))
        Z, Zt = Z[:-test_rows], Z[-test_rows:]
    D = Z.shape[1] if a.model == "lr" else Z.shape[1] - 1
    family = "logistic" if a.model == "lr" else "poisson"
    print("dataset %s: %d rows, %d parameters, model %s, trial %d" % (a.dataset, Z.shape[0], D, a.model, a.trial))

    def laplace(pts, wts):
        if a.model == "lr":
            return model_lr.laplace_fit(pts, wts)
        return model_poiss.laplace_fit(pts, wts)

    # --laplace_stream: the SVI sampler streams the points beyond one workgroup's LDS (csrc/laplace_stream.hip), and the
    # full-data and sub-sample fits run on the rows where they are resident, through the same sampler
    fitter, Z_dev = None, None
    if stream and D <= 32 and not getattr(a, "host_sampler", False):
        import torch
        fitter = bc.LaplacePosteriorSampler(family, D, seed=a.trial, stream=True)
        Z_dev = torch.from_numpy(np.ascontiguousarray(Z, dtype=np.float64)).to(fitter.device)

    def laplace_resident(rows):
        mu, W = fitter.posterior(None, rows)
        return mu, W.T.dot(W)

    mup, Sigp = laplace(Z, None) if fitter is None else laplace_resident(Z_dev)   # main.py:145 (tangent space of GIGA-OPT)
    SigpInv = np.linalg.inv(Sigp)
    hat = np.random.randint(0, Z.shape[0], int(np.sqrt(Z.shape[0])))
    Zhat = Z[hat]                                                              # main.py:150-152
    muh, Sigh = laplace(Zhat, None) if fitter is None else laplace_resident(Z_dev[torch.from_numpy(hat).to(Z_dev.device)])
    gauss = lambda mu, Sig: (lambda n, w, p: np.atleast_2d(np.random.multivariate_normal(mu, Sig, n)))

    def sampler_w(n, wts, pts):                                                # main.py:155-162
        if wts is None or pts is None or np.asarray(pts).shape[0] == 0:
            return np.random.randn(n, D)                                       # the prior N(0, I)
        keep = np.asarray(wts) > 0
        if not keep.any():
            return np.random.randn(n, D)
        mu, Sig = laplace(np.atleast_2d(pts)[keep], np.asarray(wts)[keep])
        return np.atleast_2d(np.random.multivariate_normal(mu, Sig, n))

    # the same sampler on the device (csrc/laplace.hip: one launch per call, and -- through enqueue_plan -- from weights that
    # never leave the device, so SparseVI enqueues its whole ADAM loop) where the model fits it: D <= 32 parameters
    sampler_host = sampler_w
    if D <= 32 and not getattr(a, "host_sampler", False):
        try:
            sampler_w = bc.LaplacePosteriorSampler(family, D, seed=a.trial, stream=stream)
        except RuntimeError:
            sampler_w = sampler_host
    dev = lambda sampler: bc.DeviceProjector(family, sampler, a.proj_dim)
    build = {
        # (--subsample_select / --subsample_opt: the drawn rows are projected where the data is resident, never gathered on the host)
        "SVI": lambda: bc.SparseVICoreset(Z, dev(sampler_w), n_subsample_select=a.subsample_select, n_subsample_opt=a.subsample_opt,
                                          opt_itrs=a.opt_itrs, step_sched=eval(a.step_sched), subsample="device"),
        # (the quasi-Newton coreset: M uniformly drawn points, opt_itrs Newton steps on all weights; every size is built afresh)
        "QNC": lambda: bc.QuasiNewtonCoreset(Z, dev(sampler_w), n_subsample_opt=a.subsample_opt, opt_itrs=a.opt_itrs,
                                             step_sched=eval(a.step_sched), tau=getattr(a, "qn_tau", 1e-2), subsample="device"),
        # (Coreset MCMC: M uniformly drawn points, the weights learned from chains on the coreset posterior while they run; its own
        # step schedule -- --step_sched is tuned for SVI's gradients -- and, as QNC, every size built afresh)
        "CMC": lambda: bc.CoresetMCMC(Z, family, opt_itrs=a.opt_itrs, n_subsample=a.subsample_opt, seed=a.trial),
        "GIGA-OPT": lambda: bc.HilbertCoreset(Z, dev(gauss(mup, Sigp))),
        "GIGA-REAL": lambda: bc.HilbertCoreset(Z, dev(gauss(muh, Sigh))),
        "US": lambda: bc.UniformSamplingCoreset(Z),
    }
    alg = build[a.alg]()
    n = Ms.shape[0]
    extra = {}
    if use_mcmc:
        full_samples, full_t = full_data_samples(a, Z, nuts_stream, test_rows or 0)
        mup, Sigp = full_samples.mean(axis=0), np.cov(full_samples, rowvar=False)     # main.py:137-138
        SigpInv = np.linalg.inv(Sigp)
        _, gfs = bc.log_joint_grad(family, Z, None, full_samples)
        extra = dict(Fs=np.zeros(n), full_mcmc_time_per_itr=np.full(n, full_t), mcmc_time_per_itr=np.zeros(n))
        if Zt is not None:
            extra.update(test_ll=np.zeros(n), full_test_ll=np.full(n, bc.log_predictive(family, Zt, full_samples).lppd.mean()))
        if disc is not None:                                                   # the frame of the full-data draws: theta = mup + L xi
            frame = dict(transform=np.linalg.cholesky(Sigp).T, center=mup, max_draws=disc)
            full_ksd = bc.stein_discrepancy(full_samples, family=family, pts=Z, **frame).ksd
            extra.update(energy=np.zeros(n), ksd=np.zeros(n), full_ksd=np.full(n, full_ksd))
    cputs, walls, csizes = np.zeros(n), np.zeros(n), np.zeros(n)
    rklw, fklw, mu_errs, Sig_errs = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)

    def score(m, muw, Sigw):
        rklw[m] = gaussian_kl(muw, Sigw, mup, SigpInv)
        fklw[m] = gaussian_kl(mup, Sigp, muw, np.linalg.inv(Sigw))
        mu_errs[m] = np.sqrt(((mup - muw) ** 2).sum()) / np.sqrt((mup ** 2).sum())
        Sig_errs[m] = np.sqrt(((Sigp - Sigw) ** 2).sum()) / np.sqrt((Sigp ** 2).sum())

    def score_draws(m, cst, t_cst, cpts, cwts):
        _, gcs = bc.log_joint_grad(family, cpts, cwts, full_samples)
        extra["Fs"][m] = ((gcs - gfs) ** 2).sum(axis=1).mean()                  # main.py:226-228
        extra["mcmc_time_per_itr"][m] = t_cst / (a.mcmc_samples_coreset * 2)
        if Zt is not None:
            extra["test_ll"][m] = bc.log_predictive(family, Zt, cst).lppd.mean()
        if disc is not None:
            extra["energy"][m] = bc.energy_distance(cst, full_samples, **frame).value
            extra["ksd"][m] = bc.stein_discrepancy(cst, family=family, pts=Z, **frame).ksd
        score(m, cst.mean(axis=0), np.cov(cst, rowvar=False))

    kept = []                               # --mcmc_batch: (m, points, weights) of every size, scored behind the loop
    for m in range(n):
        print("M = %d: coreset construction, %s %s %d" % (Ms[m], a.alg, a.dataset, a.trial))
        c0, t0 = time.process_time(), time.perf_counter()
        if a.alg in ("QNC", "CMC"):
            alg.reset()
            alg.build(int(Ms[m]))
        else:
            alg.build(int(Ms[m] if m == 0 else Ms[m] - Ms[m - 1]))
        cputs[m] = time.process_time() - c0 + (cputs[m - 1] if m else 0.0)
        walls[m] = time.perf_counter() - t0 + (walls[m - 1] if m else 0.0)
        wts, pts, idcs = alg.get()
        csizes[m] = (wts > 0).sum()
        if use_mcmc:
            if csizes[m] > 0 and batch:
                kept.append((m, pts[wts > 0], wts[wts > 0]))
            elif csizes[m] > 0:
                cst, t_cst, _ = mcmc.run(pts[wts > 0], wts[wts > 0], a.mcmc_samples_coreset, a.model, a.trial, kernel=mcmc_kernel,
                                           nuts_stream=nuts_stream, adapt_metric=adapt_metric)
                score_draws(m, cst, t_cst, pts[wts > 0], wts[wts > 0])
            else:
                score_draws(m, np.random.RandomState(a.trial).randn(a.mcmc_samples_coreset, D), 0.0, pts[wts > 0], wts[wts > 0])   # the prior
        elif csizes[m] > 0:
            score(m, *laplace(pts[wts > 0], wts[wts > 0]))
        else:
            score(m, np.zeros(D), np.eye(D))
    if kept:
        scored = mcmc.run_many([(cpts, cwts) for _, cpts, cwts in kept], a.mcmc_samples_coreset, a.model, a.trial, kernel=mcmc_kernel,
                               nuts_stream=nuts_stream, adapt_metric=adapt_metric)
        for (m, cpts, cwts), (cst, t_cst, _) in zip(kept, scored):
            score_draws(m, cst, t_cst, cpts, cwts)
    print("final: csize %d, reverse KL %.6g, forward KL %.6g, %.2f s wall" % (csizes[-1], rklw[-1], fklw[-1], walls[-1]))
    results.save(a, a.results_folder, csizes=csizes, Ms=Ms, cputs=cputs, walls=walls, rklw=rklw, fklw=fklw, mu_errs=mu_errs,
                 Sig_errs=Sig_errs, **extra)


def parser():
    ap = argparse.ArgumentParser("Runs logistic or poisson regression (employing coreset contruction) on the specified dataset")
    sub = ap.add_subparsers(help="sub-command help")
    rp = sub.add_parser("run", help="Runs the main computational code")
    rp.set_defaults(func=run)
    ap.add_argument("--model", type=str, choices=["lr", "poiss"], default="lr")
    ap.add_argument("--dataset", type=str, default="synth_lr")
    ap.add_argument("--data_num", type=int, default=10000)
    ap.add_argument("--data_dim", type=int, default=3)
    ap.add_argument("--alg", type=str, default="SVI", choices=["SVI", "GIGA-OPT", "GIGA-REAL", "US", "QNC", "CMC"])
    ap.add_argument("--mcmc_samples_full", type=int, default=10000, help="--eval mcmc: draws from the full-data posterior")
    ap.add_argument("--mcmc_samples_coreset", type=int, default=10000, help="--eval mcmc: draws from every coreset's posterior")
    ap.add_argument("--eval", type=str, choices=["laplace", "mcmc"], default="laplace",
                    help="score a coreset by the Laplace approximation of its posterior, or by HMC on it (bc.DeviceHMC)")
    ap.add_argument("--mcmc_kernel", type=str, choices=["hmc", "nuts"], default=argparse.SUPPRESS,    # (absent = hmc: result files keep their argument set)
                    help="--eval mcmc: the transition on every coreset's posterior, default hmc (nuts: bc.DeviceHMC(kernel='nuts')); the full "
                         "data stays HMC")
    ap.add_argument("--mcmc_nuts_stream", action="store_true", default=argparse.SUPPRESS,   # (result files keep their argument set)
                    help="with --mcmc_kernel nuts: coresets past one workgroup's LDS and the full-data chain run the streamed NUTS "
                         "(bc.DeviceHMC(kernel='nuts', stream=True))")
    ap.add_argument("--mcmc_adapt_metric", type=str, choices=["diag", "dense"], default=argparse.SUPPRESS,   # (result files keep their argument set)
                    help="with --mcmc_kernel nuts: every coreset that fits the adapting LDS-resident NUTS learns a metric in its warm-up "
                         "(bc.DeviceHMC(kernel='nuts', adapt_metric=...)); the others run as without it")
    ap.add_argument("--mcmc_batch", action="store_true", default=argparse.SUPPRESS,         # (result files keep their argument set)
                    help="with --mcmc_kernel nuts: keep every size's coreset and score them behind the build in one launch "
                         "(bc.DeviceHMC.sample_many); mcmc_time_per_itr is then the launch's time over the coresets in it")
    ap.add_argument("--mcmc_test_rows", type=int, default=argparse.SUPPRESS,                 # (result files keep their argument set)
                    help="with --eval mcmc: hold out the last K rows of the data before anything is fitted or built and add the columns "
                         "test_ll / full_test_ll, their mean log predictive density under each coreset's / the full data's draws "
                         "(bc.log_predictive)")
    ap.add_argument("--mcmc_discrepancy", type=int, default=argparse.SUPPRESS,               # (result files keep their argument set)
                    help="with --eval mcmc: add the columns energy / ksd / full_ksd -- the squared energy distance of each coreset's "
                         "draws to the full-data draws and the IMQ kernel Stein discrepancy of each coreset's / the full data's draws "
                         "under the full-data score, each side thinned to at most K draws (bc.energy_distance, bc.stein_discrepancy)")
    ap.add_argument("--proj_dim", type=int, default=500)
    ap.add_argument("--coreset_size_max", type=int, default=1000)
    ap.add_argument("--coreset_num_sizes", type=int, default=7)
    ap.add_argument("--coreset_size_spacing", type=str, choices=["log", "linear"], default="log")
    ap.add_argument("--opt_itrs", type=int, default=100)
    ap.add_argument("--step_sched", type=str, default="lambda i : 1./(1+i)")
    ap.add_argument("--qn_tau", type=float, default=argparse.SUPPRESS,                       # (absent = 1e-2: result files keep their argument set)
                    help="QNC: the regularisation tau of (G + tau I) d = b")
    ap.add_argument("--subsample_select", type=int, default=None, help="SVI: rows drawn for every selection step (default: all)")
    ap.add_argument("--subsample_opt", type=int, default=None, help="SVI / QNC / CMC: rows drawn for every weight step (default: all)")
    ap.add_argument("--trial", type=int, default=1)
    ap.add_argument("--results_folder", type=str, default="results/")
    ap.add_argument("--verbosity", type=str, default="error", choices=["error", "warning", "critical", "info", "debug"])
    ap.add_argument("--laplace_stream", action="store_true", default=argparse.SUPPRESS,     # (result files keep their argument set)
                    help="SVI: bc.LaplacePosteriorSampler(stream=True) -- any coreset size on the device; the full-data and sub-sample "
                         "Laplace fits on the resident rows through the same kernel")
    ap.add_argument("--host_sampler", action="store_true", help="SVI: the Laplace fit of every sampler call on the host (NumPy) instead of csrc/laplace.hip")
    return ap


if __name__ == "__main__":
    args = parser().parse_args()
    if not hasattr(args, "func"):
        parser().error("choose a sub-command: run")
    args.func(args)
