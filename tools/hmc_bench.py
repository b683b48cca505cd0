"""Dev tool: time of the device HMC (bc.DeviceHMC, csrc/hmc.hip) per leapfrog step and per transition, and effective samples
per second -- coreset path at k in {30, 300, 1000}, D = 10, 64 and 256 chains; streamed path at N = 1M, D = 10, 64 chains -- next
to the NumPy restatement's time per transition on the host (tests/hmc_restatement.py) and the log-joint pass against its
fp64-VALU model.  One JSON line per case.  `--kernel nuts`: the coreset cases only, every one with the NUTS
kernel (csrc/nuts.hip, max_depth 8) beside the HMC kernel at L = 8 from the same run -- time per leaf (one target evaluation), time
per transition, mean tree depth, mean leapfrog steps, effective samples per second pooled over the chains.
`--kernel nuts --stream`: the streamed NUTS (csrc/nuts_stream.hip) at k = 4096 and N = 1M, D = 10, 64 and 256 chains,
each beside the streamed HMC at L = 8 on the same rows, the two alternating -- time per round (one leaf of every running chain), time
per transition, the rounds of the launch over the mean leaves per chain (the price of ending with the slowest chain), effective
samples per second, and the passes' share of the fp64-VALU model of DESIGN.md 4.12.
`--kernel nuts --adapt_metric diag|dense`: the NUTS rows with the metric learned in the windowed warm-up (csrc/nuts_adapt.h,
DESIGN.md 4.17).  `--identity`: center 0 and transform I in place of the Laplace frame; `--scale S`: the feature columns scaled
geometrically from 1 to S (badly scaled data, where a learned metric pays).
`--kernel nuts --batch [--adapt_metric diag|dense]`: the seven coreset sizes of the logistic / Poisson harness at `coreset_size_max`
1000 (k = 1, 3, 10, 31, 100, 316, 1000), 64 chains, scored by seven successive `sample` calls and by one `sample_many` with the same
seeds (csrc/nuts.hip nuts_batch_kernel), the two alternating, three repeats each: both wall times, and the largest
problem alone and inside the batch in us per leaf.  The draws are checked to be equal before anything is printed.

    python tools/hmc_bench.py [--quick] [--kernel nuts [--stream | --batch [--adapt_metric diag|dense] |
                                                         [--adapt_metric diag|dense] [--identity] [--scale S]]]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "bayesian-coresets_amd"), os.path.join(ROOT, "bayesian-coresets_amd", "examples", "common"),
          os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import hmc_restatement as hr  # noqa: E402
import model_lr  # noqa: E402

L = 8


def ess_per_chain(x):
    """Effective sample size of one coordinate of one chain by the initial positive sequence of its autocorrelations."""
    x = x - x.mean()
    n = x.shape[0]
    f = np.fft.rfft(x, 2 * n)
    ac = np.fft.irfft(f * np.conj(f))[:n]
    ac /= ac[0]
    s = 0.0
    for t in range(1, n - 1, 2):
        pair = ac[t] + ac[t + 1]
        if pair < 0:
            break
        s += pair
    return n / (1.0 + 2.0 * s)


def data(n, d, rs):
    X = np.hstack((rs.randn(n, d - 1), np.ones((n, 1))))
    y = np.where(rs.rand(n) < 1 / (1 + np.exp(-X.dot(np.ones(d) / np.sqrt(d)))), 1.0, -1.0)
    return y[:, None] * X


def case(bc, torch, name, pts, wts, chains, n, center=None, transform=None):
    D = pts.shape[1]
    hmc = bc.DeviceHMC("logistic", D, chains=chains, leapfrog=L, seed=1)
    hmc.sample(pts, wts, 10, 10, center=center, transform=transform)               # (first-use costs)
    res = hmc.sample(pts, wts, n, n, center=center, transform=transform)
    per_tr = res.seconds_per_iteration
    ess = np.mean([ess_per_chain(res.samples[c, :, j]) for c in range(min(chains, 16)) for j in range(D)]) * chains
    out = dict(case=name, path="streamed" if res.streamed else "coreset", k=int(pts.shape[0]), D=D, chains=chains,
               us_per_transition=per_tr * 1e6, us_per_leapfrog=per_tr * 1e6 / L, us_per_transition_per_chain=per_tr * 1e6 / chains,
               accept=float(res.accept_rate.mean()), step=float(res.step_size.mean()), rhat_max=float(np.nanmax(res.rhat)),
               ess_per_second=float(ess / (per_tr * 2 * n)))
    print(json.dumps(out), flush=True)
    return res


def case_nuts(bc, name, pts, wts, chains, n, center, transform, hmc_res, adapt_metric=None):
    """The NUTS kernel on the case `hmc_res` ran.  A launch ends with its slowest chain (a workgroup each, all resident at
    once), so the time per leaf is the launch time over the largest number of evaluations any chain made."""
    D = pts.shape[1]
    nuts = bc.DeviceHMC("logistic", D, chains=chains, seed=1, kernel="nuts", max_depth=8, adapt_metric=adapt_metric)
    nuts.sample(pts, wts, 10, 10, center=center, transform=transform)              # (first-use costs)
    res = nuts.sample(pts, wts, n, n, center=center, transform=transform)
    rows = []
    for kernel, r in (("hmc", hmc_res), ("nuts", res)):
        per_tr = r.seconds_per_iteration
        ess = np.mean([ess_per_chain(r.samples[c, :, j]) for c in range(min(chains, 16)) for j in range(D)]) * chains
        if kernel == "nuts":
            evals, depth, leaps = float(r.leapfrog_total.max()) + 1.0, float(r.tree_depth.mean()), float(r.n_leapfrog.mean())
        else:
            evals, depth, leaps = 2.0 * n * L + 1.0, None, float(L)
        rows.append(dict(case=name, kernel=kernel, k=int(pts.shape[0]), D=D, chains=chains, us_per_leaf=per_tr * 2 * n * 1e6 / evals,
                         us_per_transition=per_tr * 1e6, mean_tree_depth=depth, mean_leapfrogs=leaps, accept=float(r.accept_rate.mean()),
                         step=float(r.step_size.mean()), rhat_max=float(np.nanmax(r.rhat)), ess_per_second=float(ess / (per_tr * 2 * n))))
        if kernel == "nuts":
            rows[-1].update(adapt_metric=adapt_metric, divergent=int(r.divergent.sum()))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def option(name):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else None


def case_stream(bc, name, pts, wts, chains, n, center, transform, reps=2):
    """Streamed HMC and streamed NUTS on the same rows, alternating.  A round of the NUTS launch is one pass over the rows for
    the chains still running and one leaf of each; the launch takes 1 + (the most leaves any chain took) rounds."""
    D, N = pts.shape[1], int(pts.shape[0])
    hmc = bc.DeviceHMC("logistic", D, chains=chains, leapfrog=L, seed=1)
    nuts = bc.DeviceHMC("logistic", D, chains=chains, seed=1, kernel="nuts", max_depth=8, stream=True)
    kw = dict(center=center, transform=transform, _dev_force_stream=True)
    hmc.sample(pts, wts, 2, 2, **kw)                                               # (first-use costs)
    nuts.sample(pts, wts, 2, 2, **kw)
    rate = 256 * 4 * 16 * 2.4e9                                                    # fp64 lane-operations per second
    for rep in range(reps):
        for kernel, smp in (("hmc", hmc), ("nuts", nuts)):
            r = smp.sample(pts, wts, n, n, **kw)
            assert r.streamed
            total = r.seconds_per_iteration * 2 * n
            ess = np.mean([ess_per_chain(r.samples[c, :, j]) for c in range(min(chains, 16)) for j in range(D)]) * chains
            row = dict(case=name, kernel=kernel, rep=rep, N=N, D=D, chains=chains, transitions=2 * n, us_per_transition=total * 1e6 / (2 * n),
                       accept=float(r.accept_rate.mean()), step=float(r.step_size.mean()), rhat_max=float(np.nanmax(r.rhat)),
                       ess_per_second=float(ess / total))
            if kernel == "nuts":
                leaves = r.leapfrog_total.astype(np.float64)
                rounds = float(leaves.max()) + 1.0
                evals = float((leaves + 1.0).sum())                                # chain evaluations of all passes
                row.update(rounds=rounds, us_per_round=total * 1e6 / rounds, mean_leaves_per_chain=float(leaves.mean()),
                           rounds_over_mean_leaves=rounds / float(leaves.mean()), mean_tree_depth=float(r.tree_depth.mean()),
                           mean_leapfrogs=float(r.n_leapfrog.mean()), mean_active_chains=evals / rounds,
                           pass_fraction_of_valu_model=evals * N * (100 + 2 * D) / rate / total)
            else:
                evals = chains * (2.0 * n * L + 1.0)
                row.update(us_per_leapfrog=total * 1e6 / (2 * n * L), pass_fraction_of_valu_model=evals * N * (100 + 2 * D) / rate / total)
            print(json.dumps(row), flush=True)


def case_batch(bc, rs, D, chains, n, adapt_metric, reps=3):
    """Seven successive sample calls against one sample_many on the harness's size schedule, alternating."""
    sizes = [int(k) for k in np.unique(np.logspace(0.0, 3.0, 7, dtype=np.int32))]
    problems = []
    for k in sizes:
        pts, wts = data(k, D, rs), rs.uniform(1.0, 50.0, k)
        mu, cov = model_lr.laplace_fit(pts, wts)
        problems.append(dict(pts=pts, wts=wts, center=mu, transform=np.linalg.cholesky(cov).T))
    kw = dict(chains=chains, kernel="nuts", max_depth=8, adapt_metric=adapt_metric)
    many = bc.DeviceHMC("logistic", D, seed=1, **kw)
    many.sample_many(problems, 10, 10, seeds=[1] * len(sizes))                     # (first-use costs, both ways)
    for q in problems:
        bc.DeviceHMC("logistic", D, seed=1, **kw).sample(q["pts"], q["wts"], 10, 10, center=q["center"], transform=q["transform"])
    rows = []
    for rep in range(reps):
        t0 = time.perf_counter()
        singles = [bc.DeviceHMC("logistic", D, seed=1, **kw).sample(q["pts"], q["wts"], n, n, center=q["center"], transform=q["transform"])
                   for q in problems]
        t_seq = time.perf_counter() - t0
        t0 = time.perf_counter()
        batch = many.sample_many(problems, n, n, seeds=[1] * len(sizes))
        t_many = time.perf_counter() - t0
        for a, b in zip(singles, batch):
            for name in ("samples", "step_size", "accept_rate", "tree_depth", "n_leapfrog", "leapfrog_total"):
                assert np.array_equal(getattr(a, name), getattr(b, name)), name
        evals = float(singles[-1].leapfrog_total.max()) + 1.0                      # (the largest problem's slowest chain)
        rows.append(dict(case="batch", adapt_metric=adapt_metric, rep=rep, sizes=sizes, D=D, chains=chains, transitions=2 * n,
                         wall_sequence_s=t_seq, wall_batch_s=t_many, sequence_over_batch=t_seq / t_many,
                         launches_sequence_s=[r.seconds_per_iteration * 2 * n for r in singles], launch_batch_s=batch[0].batch_seconds,
                         largest_alone_s=singles[-1].seconds_per_iteration * 2 * n,
                         largest_alone_us_per_leaf=singles[-1].seconds_per_iteration * 2 * n * 1e6 / evals,
                         batch_us_per_leaf_of_largest=batch[0].batch_seconds * 1e6 / evals))
    for row in rows:
        print(json.dumps(row), flush=True)


def host_baseline(pts, wts, center, transform, n=30):
    D = pts.shape[1]
    host = pts.cpu().numpy() if hasattr(pts, "cpu") else pts
    tgt = hr.Target("logistic", host, wts, D, center, transform)
    z = np.random.RandomState(0).randn(n, D + 3)
    t0 = time.perf_counter()
    hr.run_chain(tgt, z, n, L, 0.5)
    return (time.perf_counter() - t0) / n


def main():
    import torch
    import bayesiancoresets_amd as bc
    quick = "--quick" in sys.argv
    nuts = "--kernel" in sys.argv and sys.argv[sys.argv.index("--kernel") + 1:][:1] == ["nuts"]
    rs = np.random.RandomState(0)
    D = 10
    if nuts and "--stream" in sys.argv:
        k = 4096
        pts, wts = data(k, D, rs), rs.uniform(1.0, 50.0, k)
        mu, cov = model_lr.laplace_fit(pts, wts)
        for chains in (64, 256):
            case_stream(bc, "k=%d" % k, pts, wts, chains, 50 if quick else 200, mu, np.linalg.cholesky(cov).T)
        N = 100000 if quick else 1000000
        Z = torch.from_numpy(data(N, D, rs)).cuda()
        mu, cov = model_lr.laplace_fit(Z)
        for chains in (64, 256):
            case_stream(bc, "N=%d" % N, Z, None, chains, 10 if quick else 50, mu, np.linalg.cholesky(cov).T)
        return
    adapt_metric, identity, scale = option("--adapt_metric"), "--identity" in sys.argv, float(option("--scale") or 1.0)
    if nuts and "--batch" in sys.argv:
        case_batch(bc, rs, D, 64, 100 if quick else 500, adapt_metric)
        return
    for k in (30, 300, 1000):
        pts, wts = data(k, D, rs), rs.uniform(1.0, 50.0, k)
        pts[:, :D - 1] *= scale ** (np.arange(D - 1) / (D - 2.0))
        mu, cov = model_lr.laplace_fit(pts, wts)
        W = np.linalg.cholesky(cov).T
        if identity:
            mu, W = np.zeros(D), np.eye(D)
        host = None if nuts else host_baseline(pts, wts, mu, W)
        for chains in (64, 256):
            res = case(bc, torch, "coreset k=%d" % k, pts, wts, chains, 100 if quick else 500, mu, W)
            if nuts:
                case_nuts(bc, "coreset k=%d%s%s" % (k, " identity" if identity else "", " scale %g" % scale if scale != 1.0 else ""), pts, wts,
                          chains, 100 if quick else 500, mu, W, res, adapt_metric)
        if nuts:
            continue
        print(json.dumps(dict(case="host restatement k=%d" % k, us_per_transition_per_chain=host * 1e6)), flush=True)
    if nuts:
        return
    N = 100000 if quick else 1000000
    Z = torch.from_numpy(data(N, D, rs)).cuda()
    mu, cov = model_lr.laplace_fit(Z)
    W = np.linalg.cholesky(cov).T
    case(bc, torch, "streamed N=%d" % N, Z, None, 64, 20 if quick else 100, mu, W)
    print(json.dumps(dict(case="host restatement N=%d" % N, us_per_transition_per_chain=host_baseline(Z, None, mu, W, 3) * 1e6)), flush=True)
    # the log-joint pass alone against its model: C x N evaluations of ~100 fp64 VALU operations (exp, log1p, two
    # divisions) plus 2 D multiply-adds each, on 256 CUs x 4 SIMDs x 16 fp64 lanes per clock at 2.4 GHz
    th = torch.from_numpy(mu + 0.1 * rs.randn(64, D)).cuda()
    bc.log_joint_grad("logistic", Z, None, th)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reps = 5
    for _ in range(reps):
        bc.log_joint_grad("logistic", Z, None, th)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    ops = 64.0 * N * (100 + 2 * D)
    bound = ops / (256 * 4 * 16 * 2.4e9)
    print(json.dumps(dict(case="log_joint_grad N=%d C=64" % N, us=dt * 1e6, valu_model_us=bound * 1e6, fraction_of_model=bound / dt)), flush=True)


if __name__ == "__main__":
    main()
