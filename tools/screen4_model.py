"""CPU model of the 4-bit front pass (csrc/screen4.hip): the 4-bit quantiser, the query's integer planes and the enclosure
e4 restated in NumPy, and a Frank-Wolfe run on the flagship's generator shape that prints, per iteration, what decides whether
the tier pays: how far the sentinel threshold Lg lies below the top score, how many rows the front pass lists for several
clipping factors c, how full the fullest per-wave list segment gets under front4_kernel's row-to-wave map, and the redos the
host's state machine (two plain 8-bit iterations after a fresh start, one after a redo, drop after 4 redos within 256 4-bit
iterations) would see with the chosen segment capacity.

    python tools/screen4_model.py [--rows 1000000] [--dim 512] [--iters 40] [--seed 0] [--case randn|lowrank]

Prints one JSON line per iteration and a summary line.  DESIGN.md 4.1b quotes the default arguments.  The 8-bit capture
behind the list (two slots per wave) is tools/screen8_model.py's subject and is not modelled again here."""
import argparse
import json
import math

import numpy as np

try:
    from tools.screen8_model import quantise as quantise8, kacc as kacc8, plan as plan8
except ImportError:      # run as a script from the repository root or from tools/
    from screen8_model import quantise as quantise8, kacc as kacc8, plan as plan8

FLT_MIN = np.float32(1.17549435e-38)
CLIP = 0.8            # BCX_S4_CLIP
QMAX = 1911.0         # BCX_S4_QMAX
SEG_CAP = 1024        # BCX_S4_SEG_CAP
SENTINELS = 64
CS = (0.7, 0.8, 0.9, 1.0)


def _round_up_f32(v):
    f = np.asarray(v, dtype=np.float64).astype(np.float32)
    f = np.where(f.astype(np.float64) < v, np.nextafter(f, np.float32(np.inf)), f).astype(np.float32)
    return f


def quantise4(An, c=CLIP):
    """Rows of An (fp32) -> (codes int8 [n, d] in [-7, 7], scale4 fp32 [n], bound4 fp32 [n]): quantise4_kernel's arithmetic.
    scale4 = fp32(double(max|a|) * c / 7) (at least FLT_MIN), code = clamp(rint(double(a) / double(scale4)), -7, 7),
    bound4 = fp32 round-up of sqrt(sum (a - code scale4)^2) (1 + 2^-20) in fp64 -- the clipped excess is inside it."""
    An = np.ascontiguousarray(An, dtype=np.float32)
    a64 = An.astype(np.float64)
    with np.errstate(all="ignore"):
        m = np.fmax.reduce(np.abs(An), axis=1, initial=np.float32(0))
        sc = (m.astype(np.float64) * c / 7.0).astype(np.float32)
        sc = np.where(sc >= FLT_MIN, sc, FLT_MIN).astype(np.float32)
        k = np.rint(a64 / sc.astype(np.float64)[:, None])
        k = np.clip(k, -7.0, 7.0)
        k = np.where(np.isnan(k), 0.0, k)
        r = a64 - k * sc.astype(np.float64)[:, None]
        b = np.sqrt((r * r).sum(axis=1)) * (1.0 + 2.0 ** -20)
        bf = _round_up_f32(b)
        bf = np.where(np.isnan(bf), np.float32(np.inf), bf).astype(np.float32)
    return k.astype(np.int8), sc, bf


def pack4(codes):
    """The stored bytes of a row: element 8 w + k in bits 4k..4k+3 of dword w as code + 8, padding nibbles 8;
    rows of ceil(d / 32) * 16 bytes."""
    n, d = codes.shape
    ld = (d + 31) // 32 * 32
    u = np.full((n, ld), 8, dtype=np.uint8)
    u[:, :d] = (codes.astype(np.int16) + 8).astype(np.uint8)
    return (u[:, 0::2] | (u[:, 1::2] << 4)).astype(np.uint8)      # little-endian dwords: low nibble first


def quantise_query(q32):
    """front4_head (a): integers x in [-1911, 1911], step = fp32(max|q| / 1911), qerr >= ||q - x step||_2 (fp32 round-up),
    and the three digit planes x = 256 h2 + 16 h1 + l, every digit in [-8, 7]."""
    q = np.asarray(q32, dtype=np.float32).astype(np.float64)
    m = np.abs(q).max() if q.size else 0.0
    step = np.float32(m / QMAX)
    if not (np.isfinite(m) and step >= FLT_MIN):
        z = np.zeros(q.shape, dtype=np.int64)
        return z, np.float32(0), np.float32(np.inf), (z, z, z)
    x = np.clip(np.rint(q / np.float64(step)), -QMAX, QMAX)
    r = q - x * np.float64(step)
    qerr = _round_up_f32(np.sqrt((r * r).sum()) * (1.0 + 2.0 ** -20))
    xi = x.astype(np.int64)
    l = ((xi + 8) & 15) - 8
    x1 = (xi - l) >> 4
    h1 = ((x1 + 8) & 15) - 8
    h2 = (x1 - h1) >> 4
    return xi, step, np.float32(qerr), (l, h1, h2)


def e4_coefficients(qscale32, qerr32, err_coef):
    """(eA, eB) of the head front4_head computes: e4 = bound4 eA + eB + 5e-7 |score4| (derivation: head of screen4.hip)."""
    qs, qe = float(np.float32(qscale32)), float(qerr32)
    eA = _round_up_f32((qs * 1.000002 + qe) * 1.000004)
    eB = _round_up_f32((err_coef * qs + 1.001 * qe) * 1.000004 + 1e-37)
    return np.float32(eA), np.float32(eB)


def score4(codes, sc, x, step):
    """front4_kernel's score: exact integer sum, then fp32( fp32(scale4 * step) * fp32(sum) ).  The sum is taken per digit
    plane of x as the kernel does: there an fp32 matrix product is exact (|sum| <= 4096 * 7 * 8 < 2^24)."""
    xi = np.asarray(x, dtype=np.int64)
    l = ((xi + 8) & 15) - 8
    x1 = (xi - l) >> 4
    h1 = ((x1 + 8) & 15) - 8
    h2 = (x1 - h1) >> 4
    cf = codes if codes.dtype == np.float32 else codes.astype(np.float32)
    t = (cf @ np.stack([l, h1, h2], axis=1).astype(np.float32)).astype(np.int64)
    tot = (t[:, 2] * 16 + t[:, 1]) * 16 + t[:, 0]
    return ((sc * np.float32(step)).astype(np.float32) * tot.astype(np.float32)).astype(np.float32)


def e4_of(s4, bound4, eA, eB):
    with np.errstate(all="ignore"):
        return ((bound4.astype(np.float32) * eA + eB).astype(np.float32) + (np.abs(s4) * np.float32(5e-7)).astype(np.float32)).astype(np.float32)


def upper4(s4, bound4, eA, eB):
    with np.errstate(all="ignore"):
        return (s4 + e4_of(s4, bound4, eA, eB)).astype(np.float32)


def err_coef_f32(d):
    """bcx_scan_plan's storage term for fp32 rows, as tools/screen8_model.py takes it."""
    return 1.3 * 2.0 ** -24 * (4 * 2 + 6 + 3)


def plan4(d):
    ldv = (d + 31) // 32
    G = 1
    while G < 64 and G < ldv:
        G <<= 1
    CH = 1
    while CH * G < ldv:
        CH <<= 1
    return G, CH


def wave_of_row4(n, d):
    """(segment of every row, number of segments) under front4_kernel's grid-stride map (bcx_launch_screen4)."""
    G, CH = plan4(d)
    ur = 8 if CH == 1 else 4
    rpw = 64 // G
    rpb = 4 * rpw * ur
    cap = 512
    grid = max(1, min(cap, (n + rpb - 1) // rpb))
    rows = np.arange(n)
    blk = (rows // rpb) % grid
    wave = ((rows % rpb) // rpw) % 4
    return blk * 4 + wave, grid * 4


def pick_sentinels(U, rows, bins, nbins):
    """refine_kernel's selection on the partials a tier iteration leaves: per segment the two largest upper bounds among `rows`
    (two candidates of partial p), then the 4 largest of each sixteenth of the candidates, partial p being held by wave
    (p mod 1024) // 64 of the refine kernel."""
    order = rows[np.lexsort((rows, -U[rows]))]               # by U descending, row ascending
    b = bins[order]
    first = np.zeros(len(order), dtype=bool)
    _, i1 = np.unique(b, return_index=True)
    first[i1] = True
    rest = order[~first]
    _, i2 = np.unique(bins[rest], return_index=True)
    cand_row = np.full(2 * nbins, -1, dtype=np.int64)
    cand_row[2 * bins[order[i1]]] = order[i1]
    cand_row[2 * bins[rest[i2]] + 1] = rest[i2]
    out = []
    holder = (np.arange(nbins) % 1024) // 64
    for w in range(16):
        c = cand_row.reshape(nbins, 2)[holder == w].ravel()
        c = c[c >= 0]
        out.extend(c[np.argsort(-U[c], kind="stable")[: SENTINELS // 16]].tolist())
    return np.array(out, dtype=np.int64)


def make_rows(case, rs, N, d):
    if case == "lowrank":
        return rs.randn(N, 100) @ rs.randn(100, d)
    return rs.randn(N, d)


def run(N, d, iters, seed, case="randn", cs=CS, verbose=True, seg_cap=SEG_CAP):
    rs = np.random.RandomState(seed)
    A = make_rows(case, rs, N, d)
    nrm = np.sqrt((A * A).sum(axis=1))
    An = (A / nrm[:, None]).astype(np.float32)
    c8, s8c, b8 = quantise8(An)
    A8 = (c8[:, :d].astype(np.float32) - 128.0) * s8c[:, None]
    G8, CH8 = plan8(d)
    ec = err_coef_f32(d)
    e8 = (b8.astype(np.float64) + s8c.astype(np.float64) * kacc8(d, G8, CH8)) * 1.000002 + ec
    shadows = {}
    for c in cs:
        k4, sc4, b4 = quantise4(An, c)
        shadows[c] = (k4.astype(np.float32), sc4, b4)
    bins, nbins = wave_of_row4(N, d)
    b = A.sum(axis=0)
    sigma = nrm.sum()
    xw = np.zeros(d)
    w = np.zeros(N)
    warm, halts, stamps, dropped, iters4, redos = 2, 0, [], False, 0, 0
    sentinels = None
    lines, listed_frac, fullest_all = [], [], []
    for it in range(iters):
        q = b - xw
        q32 = q.astype(np.float32)
        qn = float(np.linalg.norm(q32.astype(np.float64)))
        score = An.astype(np.float64) @ q
        s8 = (A8 @ q32).astype(np.float64)
        U8 = s8 + e8 * qn + np.abs(s8) * 2e-7
        L8 = s8 - e8 * qn - np.abs(s8) * 2e-7
        line = {"it": it, "top_over_q": float(score.max() / qn)}
        four = (not dropped) and warm == 0
        considered = np.arange(N)
        if sentinels is not None:
            Lg = float(L8[sentinels].max())
            line["top_minus_Lg_over_q"] = float((score.max() - Lg) / qn)
            x, step, qerr, _ = quantise_query(q32)
            eA, eB = e4_coefficients(np.float32(qn), qerr, ec)
            for c in cs:
                k4, sc4, b4 = shadows[c]
                U4 = upper4(score4(k4, sc4, x, step), b4, eA, eB)
                lst = np.flatnonzero(~(U4 < np.float32(Lg)))
                full = int(np.bincount(bins[lst], minlength=nbins).max())
                line["listed_c%.1f" % c] = int(len(lst))
                line["fullest_c%.1f" % c] = full
                if c == CLIP:
                    assert score.argmax() in lst
                    if four:
                        iters4 += 1
                        listed_frac.append(len(lst) / float(N))
                        fullest_all.append(full)
                        if full > seg_cap:
                            redos += 1
                            halts += 1
                            stamps = [iters4] + stamps[:3]
                            if halts >= 4 and stamps[0] - stamps[3] < 256:
                                dropped = True
                            warm = 1
                            considered = None          # redone by the storage-precision scan: no tier partials
                        else:
                            considered = lst
        line["tier"] = "4-bit" if four else "8-bit"
        line["redos"] = redos
        line["dropped"] = dropped
        if considered is not None:
            if not four and warm > 0:
                warm -= 1
            sentinels = pick_sentinels(U8, considered, bins, nbins)
        lines.append(line)
        if verbose:
            print(json.dumps(line))
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
    out = {"case": case, "rows": N, "dim": d, "iters": iters, "seed": seed, "segments": int(nbins), "segment_capacity": seg_cap,
           "clip": CLIP, "bound8_mean": float(b8.mean()),
           "bound4_mean": {"%.1f" % c: float(shadows[c][2].mean()) for c in cs},
           "bound4_max": {"%.1f" % c: float(shadows[c][2].max()) for c in cs},
           "iterations_4bit": iters4, "redos": redos, "dropped": dropped,
           "listed_fraction_mean": float(np.mean(listed_frac)) if listed_frac else None,
           "listed_fraction_max": float(np.max(listed_frac)) if listed_frac else None,
           "fullest_segment_max": int(max(fullest_all)) if fullest_all else None}
    if verbose:
        print(json.dumps(out))
    return out, lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--case", default="both", choices=["randn", "lowrank", "both"])
    a = ap.parse_args()
    for case in (("randn", "lowrank") if a.case == "both" else (a.case,)):
        run(a.rows, a.dim, a.iters, a.seed, case)


if __name__ == "__main__":
    main()
