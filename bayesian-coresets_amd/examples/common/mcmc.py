"""MCMC for the experiments' evaluation: the role of the reference's examples/common/mcmc.py:60-70 (`run`: Stan on the data
with per-point weights, as many warm-up as sampling iterations), on ``bc.DeviceHMC`` -- Hamiltonian Monte Carlo on the GPU,
whitened by the Laplace approximation of the same weighted posterior; ``kernel="nuts"``: its No-U-Turn transition (Stan's
sampler) where the rows fit one workgroup's LDS, i.e. on coresets; with ``nuts_stream=True`` on any rows (the streamed NUTS of
csrc/nuts_stream.hip: larger coresets, the full data set).  ``run_many`` scores a sequence of coresets -- the sizes of one build,
several algorithms or trials -- with ONE launch for all that fit the LDS-resident NUTS (``bc.DeviceHMC.sample_many``, DESIGN.md
4.18) and ``run`` for each of the others; the draws are those of ``run`` per coreset."""
import numpy as np

FAMILY = {"lr": "logistic", "poiss": "poisson"}
MIN_WARMUP = 200


def run(Z, wts, n_samples, model_name, seed, chains=64, leapfrog=8, device="cuda", kernel="hmc", max_depth=8, nuts_stream=False,
        adapt_metric=None):
    """(samples (n_samples x D), seconds, the kernel that ran -- "nuts" only where it was asked for and the rows fit its
    LDS-resident path or ``nuts_stream`` lets the others stream, else "hmc" with ``leapfrog`` steps; ``adapt_metric`` ("diag" /
    "dense", with ``kernel="nuts"``): the LDS-resident NUTS learns a metric in its warm-up where the rows fit next to its
    accumulators, elsewhere the same fallbacks without one): ``n_samples`` draws from the posterior of the rows ``Z`` (host array or device
    tensor, the model's layout; None / empty: the prior) with weights ``wts`` (None: ones), pooled over ``chains`` chains
    that each warm up for as long as they sample (at least MIN_WARMUP transitions)."""
    import bayesiancoresets_amd as bc
    family = FAMILY[model_name]
    k = 0 if Z is None else len(Z)
    if k == 0:
        raise ValueError("mcmc.run: no rows (the prior needs no sampler)")
    D = Z.shape[1] - (1 if family == "poisson" else 0)
    per_chain = -(-int(n_samples) // chains)
    hmc = bc.DeviceHMC(family, D, chains=chains, leapfrog=leapfrog, seed=seed, device=device, kernel=kernel, max_depth=max_depth,
                       stream=bool(nuts_stream) and kernel == "nuts")
    ran = kernel
    if adapt_metric is not None:
        if kernel != "nuts":
            raise ValueError("mcmc.run: adapt_metric goes with kernel=\"nuts\"")
        if hmc.adapt_path(k):             # (the rows fit next to the metric's accumulators; else the fallbacks below, no metric)
            hmc = bc.DeviceHMC(family, D, chains=chains, seed=seed, device=device, kernel="nuts", max_depth=max_depth,
                               adapt_metric=adapt_metric)
    if kernel == "nuts" and not hmc.stream and not hmc.nuts_path(k):
        hmc = bc.DeviceHMC(family, D, chains=chains, leapfrog=leapfrog, seed=seed, device=device)
        ran = "hmc"
    res = hmc.sample(Z, wts, per_chain, max(per_chain, MIN_WARMUP))
    samples = res.samples.transpose(1, 0, 2).reshape(-1, D)[:int(n_samples)]
    seconds = res.seconds_per_iteration * (per_chain + res.n_warmup)
    return samples, seconds, ran


def run_many(problems, n_samples, model_name, seed, chains=64, leapfrog=8, device="cuda", kernel="nuts", max_depth=8, nuts_stream=False,
             adapt_metric=None):
    """``run`` for every ``(Z, wts)`` of ``problems``, the same draws and the same kernel named, a list in their order.  With
    ``kernel="nuts"`` the problems whose rows fit the LDS-resident NUTS share one launch (``adapt_metric``: one for those that fit
    next to the metric's accumulators, one without a metric for those that fit only the plain kernel), every problem with the noise
    of a fresh sampler of seed ``seed`` as ``run`` gives it; the others take ``run`` and its fallbacks one by one.  ``seconds`` of
    a batched problem is its launch's wall time over the problems in it."""
    import bayesiancoresets_amd as bc
    family = FAMILY[model_name]
    problems = list(problems)
    if any(Z is None or len(Z) == 0 for Z, _ in problems):
        raise ValueError("mcmc.run_many: a problem without rows (the prior needs no sampler)")
    if adapt_metric is not None and kernel != "nuts":
        raise ValueError("mcmc.run_many: adapt_metric goes with kernel=\"nuts\"")
    out = [None] * len(problems)
    per_chain = -(-int(n_samples) // chains)
    samplers, groups = {}, {}

    def sampler(D, metric):
        if (D, metric) not in samplers:
            samplers[D, metric] = bc.DeviceHMC(family, D, chains=chains, seed=seed, device=device, kernel="nuts", max_depth=max_depth,
                                               adapt_metric=metric)
        return samplers[D, metric]

    for i, (Z, _) in enumerate(problems if kernel == "nuts" else ()):
        D, k = Z.shape[1] - (1 if family == "poisson" else 0), len(Z)
        if sampler(D, None).nuts_path(k):         # (else run: the streamed NUTS or the fallback to HMC)
            metric = adapt_metric if adapt_metric is not None and sampler(D, None).adapt_path(k) else None
            groups.setdefault((D, metric), []).append(i)
    from bayesiancoresets_amd.mcmc import NUTS_NOISE_BYTES_MAX
    n_warmup = max(per_chain, MIN_WARMUP)
    for (D, metric), every in groups.items():
        row = D + 3 * max_depth + 2 * ((1 << max_depth) - 1)
        most = max(1, NUTS_NOISE_BYTES_MAX // (8 * chains * (per_chain + n_warmup) * row))     # (problems whose noise one call may hold)
        for at in (every[b:b + most] for b in range(0, len(every), most)):
            res = sampler(D, metric).sample_many([problems[i] for i in at], per_chain, n_warmup, seeds=[seed] * len(at))
            for i, r in zip(at, res):
                out[i] = (r.samples.transpose(1, 0, 2).reshape(-1, D)[:int(n_samples)], r.batch_seconds / len(at), "nuts")
    for i, (Z, wts) in enumerate(problems):
        if out[i] is None:
            out[i] = run(Z, wts, n_samples, model_name, seed, chains=chains, leapfrog=leapfrog, device=device, kernel=kernel,
                         max_depth=max_depth, nuts_stream=nuts_stream, adapt_metric=adapt_metric)
    return out
