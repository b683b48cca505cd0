"""CPU model of the 8-bit screening tier (csrc/screen8.hip): the quantiser and its per-row bound restated in NumPy, the
survivor count per Frank-Wolfe iteration on the flagship's generator shape, and an emulation of the per-wave capture
(two slots per wave, 4 waves per workgroup, grid-stride row mapping of screen_kernel<false, 32, 1, 4>) that predicts how
often a greedy iteration overflows it.

    python tools/screen8_model.py [--rows 1000000] [--dim 512] [--iters 40] [--seed 0] [--grid 512]

Prints one JSON line.  The numbers quoted in DESIGN.md 4.1 come from the default arguments."""
import argparse
import json
import math

import numpy as np

FLT_MIN = np.float32(1.17549435e-38)


def quantise(An):
    """Rows of An (fp32, or fp16 values held exactly in fp32) -> (codes uint8 [n, ld8], scale fp32 [n], bound fp32 [n]).
    The same arithmetic as quantise_kernel: scale = fp32(double(max|a|) / 127) (at least FLT_MIN),
    code = 128 + clamp(rint(double(a) / double(scale)), -127, 127), bound = fp32 round-up of
    sqrt(sum (a - (code - 128) scale)^2) (1 + 2^-20) in fp64.  Padding bytes hold 128."""
    An = np.ascontiguousarray(An, dtype=np.float32)
    n, d = An.shape
    ld8 = (d + 15) // 16 * 16
    a64 = An.astype(np.float64)
    with np.errstate(all="ignore"):
        m = np.fmax.reduce(np.abs(An), axis=1, initial=np.float32(0)) if d else np.zeros(n, np.float32)
        sc = (m.astype(np.float64) / 127.0).astype(np.float32)
        sc = np.where(sc >= FLT_MIN, sc, FLT_MIN).astype(np.float32)
        c = np.rint(a64 / sc.astype(np.float64)[:, None])
        c = np.where(c > 127.0, 127.0, np.where(c < -127.0, -127.0, c))
        c = np.where(np.isnan(c), 0.0, c)
        r = a64 - c * sc.astype(np.float64)[:, None]
        b = np.sqrt((r * r).sum(axis=1)) * (1.0 + 2.0 ** -20)
        bf = b.astype(np.float32)
        bf = np.where(bf.astype(np.float64) < b, np.nextafter(bf, np.float32(np.inf)), bf).astype(np.float32)
        bf = np.where(np.isnan(bf), np.float32(np.inf), bf).astype(np.float32)
    codes = np.full((n, ld8), 128, dtype=np.uint8)
    codes[:, :d] = (c + 128.0).astype(np.uint8)
    return codes, sc, bf


def dequantise(codes, sc, d):
    """fp64 values the codes stand for (exact: 8-bit integer times fp32 scale)."""
    return (codes[:, :d].astype(np.float64) - 128.0) * sc.astype(np.float64)[:, None]


def kacc(d, G, CH):
    """fp32 accumulation term of screen_kernel per unit of scale and |q| (derivation at the head of screen8.hip)."""
    u = 2.0 ** -24
    lg = int(math.log2(G))
    return 1.3 * u * (511.0 * (16.0 * CH + 1.0) + 127.0 * lg) * math.sqrt(d)


def plan(d):
    ldv = (d + 15) // 16
    G = 1
    while G < 64 and G < ldv:
        G <<= 1
    CH = 1
    while CH * G < ldv:
        CH <<= 1
    return G, CH


def wave_of_row(rows, G, UR, grid):
    """The capture bin (workgroup * 4 + wave) that screen_kernel assigns a row to."""
    rpw = 64 // G
    rpb = 4 * rpw * UR
    blk = (rows // rpb) % grid
    within = rows % rpb
    wave = (within // rpw) % 4
    return blk * 4 + wave


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--trials", type=int, default=200, help="random placements of each iteration's survivors over the bins")
    args = ap.parse_args()
    rs = np.random.RandomState(args.seed)
    N, d = args.rows, args.dim
    A = rs.randn(N, d)
    nrm = np.sqrt((A * A).sum(axis=1))
    An = (A / nrm[:, None]).astype(np.float32)
    codes, sc, bound = quantise(An)
    Aq = (codes[:, :d].astype(np.float32) - 128.0) * sc[:, None]      # exact in fp32
    G, CH = plan(d)
    e_row = (bound.astype(np.float64) + sc.astype(np.float64) * kacc(d, G, CH)) * 1.000002 + 1.3 * 2.0 ** -24 * (4 * 2 + 6 + 3)
    # Frank-Wolfe (frankwolfe.py:15-40 of the reference), selection by the exact scores
    b = A.sum(axis=0)
    sigma = nrm.sum()
    xw = np.zeros(d)
    w = np.zeros(N)
    counts, overflow_real, top_ratio, spread = [], 0, [], []
    bins = wave_of_row(np.arange(N), G, 4, args.grid)
    nbins = args.grid * 4
    placed_over = 0
    for it in range(args.iters):
        q = b - xw
        qn = float(np.linalg.norm(q))
        s8 = (Aq @ q.astype(np.float32)).astype(np.float64)
        U = s8 + e_row * qn
        L = s8 - e_row * qn
        surv = np.flatnonzero(U >= L.max())
        counts.append(int(len(surv)))
        per_bin = np.bincount(bins[surv], minlength=nbins)
        overflow_real += int(per_bin.max() > 2 or len(surv) > 256)
        # the same number of survivors dropped on uniformly random rows: the rate the row mapping gives in general
        for _ in range(args.trials):
            rr = rs.randint(0, N, size=len(surv))
            placed_over += int(np.bincount(bins[rr], minlength=nbins).max() > 2)
        score = (An.astype(np.float64) @ q)
        top_ratio.append(float(score.max() / qn))
        spread.append(float(score.std() / qn))
        f = int(np.argmax(score))
        if it == 0:
            w[f] = sigma / nrm[f]
            xw = w[f] * A[f]
        else:
            v = sigma / nrm[f] * A[f] - xw
            g = float(v @ (b - xw)) / float(v @ v)
            w *= (1.0 - g)
            w[f] += g * sigma / nrm[f]
            xw = (1.0 - g) * xw + g * sigma / nrm[f] * A[f]
    out = {
        "rows": N, "dim": d, "iters": args.iters, "seed": args.seed, "grid": args.grid, "bins": nbins, "G": G, "CH": CH,
        "bound_mean": float(bound.mean()), "bound_max": float(bound.max()), "scale_mean": float(sc.mean()),
        "kacc_times_scale_mean": float(sc.mean() * kacc(d, G, CH)),
        "survivors_min": int(min(counts)), "survivors_max": int(max(counts)), "survivors_mean": float(np.mean(counts)),
        "top_score_over_qnorm": float(np.mean(top_ratio)), "score_std_over_qnorm": float(np.mean(spread)),
        "capture_overflows_at_the_real_rows": overflow_real,
        "capture_overflow_rate_random_placement": placed_over / float(args.iters * args.trials),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
