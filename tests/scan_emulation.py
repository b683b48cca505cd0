"""Pure-NumPy companion of the correlation scan (csrc/scan.hip, screen8.hip): what the stored rows and the fp32 query give
as a score, the exact score in long double, a restatement of the launch plan, and the adversarial inputs of
tests/test_gpu_scan_enclosure.py with the host-side checks that they ARE adversarial (tests/test_scale_host.py runs those
without a GPU).  Nothing here touches the device."""
import numpy as np

STORAGES = ("float32", "float16", "float64")
RESOLUTION = {"float32": 2.0 ** -24, "float16": 2.0 ** -11, "float64": 2.0 ** -53}   # unit roundoff of the stored rows
EPL = {"float32": 4, "float16": 8, "float64": 2}                                    # elements per 16-byte piece
MAX_CAND = 64             # BCX_MAX_CAND (csrc/bcx_internal.h): rows resolve re-scores in fp64 before it asks for the exact scan
# Row lengths of tests/test_gpu_scan_enclosure.py and the plan (G, CH, UR, ragged R, deep D, long rows L) each reaches per
# storage type, read from bcx_scan_plan (scan_plan below restates it; tests/test_scale_host.py checks the coverage):
#      d   float32          float16          float64      |      d   float32          float16          float64
#      1   1,1,4            1,1,4            1,1,4        |    300   64,2,4 R         64,1,8 RD        64,4,4 D
#      3   1,1,4            1,1,4            2,1,4        |    513   64,4,4 D         64,2,8 RD        64,8,2 D
#      4   1,1,4            1,1,4            2,1,4        |   1000   64,4,2           64,2,4           64,8,1
#      5   2,1,4            1,1,4            4,1,4        |   1024   64,4,2           64,2,4           64,8,1
#      8   2,1,4            1,1,4            4,1,4        |   1025   64,8,2 D         64,4,4 D         64,16,1
#      9   4,1,4            2,1,4            8,1,4        |   2048   64,8,1           64,4,2           64,16,1
#     31   8,1,4            4,1,4            16,1,4       |   2049   64,16,1          64,8,2 D         L
#     33   16,1,4           8,1,4            32,1,8 RD    |   4096   64,16,1          64,8,1           L
#     64   16,1,4           8,1,4            32,1,4       |   4097   L                64,16,1          L
#    100   32,1,8 RD        16,1,4           64,1,8 RD    |   5000   L                64,16,1          L
#    127   32,1,4           16,1,4           64,1,4       |   8200   L                L                L
#    129   64,1,8 RD        32,1,8 RD        64,2,8 RD    |
#    256   64,1,4           32,1,4           64,2,4       |
#    257   64,2,8 RD        64,1,8 RD        64,4,4 D     |
D_LIST = (1, 3, 4, 5, 8, 9, 31, 33, 64, 100, 127, 129, 256, 257, 300, 513, 1000, 1024, 1025, 2048, 2049, 4096, 4097, 5000, 8200)
SCREEN_MAX_SURV = 256     # BCX_SCREEN_MAX_SURV: rows the 8-bit tier passes on before it asks for the storage-precision scan


# ---- arithmetic ------------------------------------------------------------------------------------------------------
def exact_scores(X, q):
    """(row . q) / ||row|| in long double on the raw fp64 rows."""
    Xl, ql = np.asarray(X, dtype=np.longdouble), np.asarray(q, dtype=np.longdouble)
    if Xl.shape[1] == 1:      # x q / |x| = sign(x) q exactly: rows of one element tie exactly, as An = +-1 does in the reference
        return np.sign(Xl[:, 0]) * ql[0]
    return Xl.dot(ql) / np.sqrt((Xl * Xl).sum(axis=1))


def first_argmax(s):
    """ndarray.argmax: the first maximum."""
    return int(np.argmax(np.asarray(s)))


def query_exponent(q):
    """E of csrc/apply_common.h: the fp32 query holds q * 2^-E, E the exponent of |q| (0 for a zero / non-finite norm)."""
    q = np.asarray(q, dtype=np.float64)
    m = float(np.max(np.abs(q))) if q.size else 0.0
    if not (m > 0.0 and np.isfinite(m)):
        return 0
    e0 = int(np.floor(np.log2(m)))
    n = float(np.sqrt((np.ldexp(q, -e0) ** 2).sum()))
    return e0 + int(np.floor(np.log2(n)))


def stored_rows(X, storage):
    """The normalised rows as the device stores them: A / ||A|| in fp64, then one rounding to the storage type."""
    X = np.asarray(X, dtype=np.float64)
    An = X / np.sqrt((X * X).sum(axis=1))[:, None]
    return An.astype(storage)


def stored_scores(X, q, storage):
    """Score of the stored rows against the stored query, products and sum carried in fp64 (the roundings of the storage
    only: what any summation order of the scan approximates), returned in the caller's scale."""
    q = np.asarray(q, dtype=np.float64)
    if storage == "float64":
        qs, E = q, 0
    else:
        E = query_exponent(q)
        qs = np.ldexp(q, -E).astype(np.float32).astype(np.float64)
    return np.ldexp(stored_rows(X, storage).astype(np.float64).dot(qs), E)


def gap_floor(d, q):
    """64 (d + 2) 2^-53 |q|: well above the rounding of the fp64 re-score of a unit row against q."""
    return 64.0 * (d + 2) * 2.0 ** -53 * float(np.sqrt((np.asarray(q, dtype=np.float64) ** 2).sum()))


# ---- the launch plan (bcx_scan_plan, csrc/scan.hip; bcx_launch_screen, csrc/screen8.hip) ----------------------------------
def scan_plan(d, storage):
    epl = EPL[storage]
    nvec = (d + epl - 1) // epl
    G = 1
    while G < 64 and G < nvec:
        G <<= 1
    CH = 1
    while CH < (nvec + G - 1) // G:
        CH <<= 1
    ur = 1 if CH >= 8 else min(4, 8 // CH)
    util = nvec / float(G * CH)
    ragged = util < 0.85 and G >= 32 and CH <= 2
    if ragged:
        deep = CH * ur * util < 4.5
    else:
        deep = CH < 16 and G == 64 and CH >= 2 and util < 0.80
    if deep:
        ur *= 2
    long_rows = nvec > 64 * 16
    rpb = 4 if long_rows else 4 * (64 // G) * ur        # rows a workgroup takes per trip (long rows: one per wave)
    return {"G": G, "CH": CH, "UR": ur, "ragged": ragged, "deep": deep, "long_rows": long_rows, "rpb": rpb}


def screen_rpb(d):
    """Rows per workgroup and trip of the 8-bit screen kernel (16 codes per piece, 4 row steps), None beyond its reach."""
    if d > 4096:
        return None
    ldv = (d + 15) // 16
    G = 1
    while G < 64 and G < ldv:
        G <<= 1
    return 4 * (64 // G) * 4


def edge_rows(d, storage, N):
    """Row indices on both sides of the first row-block edges of the storage scan and of the 8-bit screen, inside [0, N)."""
    out = []
    for rpb in (scan_plan(d, storage)["rpb"], screen_rpb(d)):
        if rpb:
            out += [rpb - 1, rpb, rpb + 1, 2 * rpb - 1, 2 * rpb]
    seen, res = set(), []
    for r in out:
        if 0 <= r < N and r not in seen:
            seen.add(r)
            res.append(r)
    return res


# ---- adversarial inputs ------------------------------------------------------------------------------------------------
def _fp32_query(rs, d):
    """A query that fp32 holds exactly: the storage rounding of the ROWS is what each case is about."""
    return rs.randn(d).astype(np.float32).astype(np.float64)


def _positions(d, storage, N, winner, count):
    """`count` distinct rows for a cluster: the winner's row first, then block edges, then evenly spread rows."""
    pos = [winner]
    for r in edge_rows(d, storage, N) + [0, N - 1]:
        if len(pos) < count and r not in pos:
            pos.append(r)
    step = max(1, N // (count + 1))
    r = step // 2
    while len(pos) < count:
        if r % N not in pos:
            pos.append(r % N)
        r += step if step > 1 else 1
    return pos[:count]


def cluster_case(d, storage, N, M, winner, seed, duplicate=False):
    """Rows u + eps_m v_m (u = q / |q|, v_m unit and orthogonal to u): exact scores |q| / sqrt(1 + eps_m^2), separated by a
    gap g with  gap_floor <= g |q|  and  M g < resolution of the storage: the whole cluster sits inside one rounding of
    the stored score of its winner.  The other rows are randn.  Returns X, q and the facts the precondition reads."""
    assert d >= 2
    rs = np.random.RandomState(seed)
    q = _fp32_query(rs, d)
    qn = float(np.sqrt((q * q).sum()))
    u = q / qn
    M = min(M, N)
    res = RESOLUTION["float32" if storage == "float64" else storage]
    g = max(2.0 * gap_floor(d, q) / qn, res / (4.0 * max(M, 4)))
    X = rs.randn(N, d)
    pos = _positions(d, storage, N, winner, M)
    for m, r in enumerate(pos):
        v = rs.randn(d)
        v -= v.dot(u) * u
        v /= np.sqrt((v * v).sum())
        X[r] = (u + np.sqrt(2.0 * g * (m + 0.25)) * v) * (0.5 + rs.rand())
    dup = None
    if duplicate:
        free = [r for r in range(N - 1, winner, -1) if r not in pos]
        if free:
            dup = free[0]
            X[dup] = X[winner]
    return X, q, {"winner": winner, "cluster": pos, "M": M, "gap": g * qn, "dup": dup}


def check_cluster(X, q, storage, info):
    """The precondition of a cluster case (a violated one is a broken test): see cluster_case."""
    d = X.shape[1]
    ex = exact_scores(X, q)
    qn = float(np.sqrt((q * q).sum()))
    w = info["winner"]
    assert first_argmax(ex) == w, (first_argmax(ex), w)
    others = np.delete(ex, [w] + ([info["dup"]] if info["dup"] is not None else []))
    if others.size:
        gap = float(ex[w] - others.max())
        assert gap >= gap_floor(d, q), (gap, gap_floor(d, q))
        if storage != "float64":
            assert gap < RESOLUTION[storage] * qn, (gap, RESOLUTION[storage] * qn)
    if storage != "float64":
        near = int((ex >= ex[w] - RESOLUTION[storage] * qn).sum())
        assert near >= min(info["M"], X.shape[0]), (near, info["M"])
    if info["dup"] is not None:
        assert info["dup"] > w and ex[info["dup"]] == ex[w]


def _grid_cell(x, storage):
    """For x > 0: the storage-grid values lo <= x < hi around it and the grid value below lo."""
    t = np.dtype(storage).type
    g = t(x)
    lo = g if float(g) <= x else np.nextafter(g, t(0))
    hi = np.nextafter(lo, t(np.inf))
    lo2 = np.nextafter(lo, t(0))
    return float(lo2), float(lo), float(hi)


def aligned_case(d, storage, N, winner, seed):
    """Storage rounding lined up with the query.  Every element of the winner sits just BELOW a midpoint of the storage grid
    (in magnitude, sign of q_i), so all of them round against its score; every element of the runner-up sits just ABOVE one.
    On the coordinates A the two rows straddle the SAME midpoint (equal to 2^-15 of a grid step; the runner-up stores
    one step higher); on the few coordinates B the runner-up sits one whole step lower and both store the same value.  So the
    exact order (winner ahead by the B steps) is inverted in storage by the A steps: nearly the full resolution times |q|.
    The last coordinate carries no query weight and brings both rows to unit norm, so the normalisation does not move
    anything off its place."""
    assert d >= 3 and storage != "float64"
    rs = np.random.RandomState(seed)
    q = _fp32_query(rs, d)
    q[np.abs(q) < 0.0625] = 0.0625           # (no element so small that its grid step is negligible; fp32 holds it exactly)
    q[d - 1] = 0.0
    qn = float(np.sqrt((q * q).sum()))
    u = 0.9 * q / qn
    nB = max(1, (d - 1) // 8)
    # (short rows: the B coordinates are the ones of least query weight, so that their steps stay below the resolution)
    B = set((np.argsort(np.abs(q[:d - 1]), kind="stable") if d < 16 else rs.permutation(d - 1))[:nB].tolist())
    w, r = np.zeros(d), np.zeros(d)
    for i in range(d - 1):
        lo2, lo, hi = _grid_cell(abs(u[i]), storage)
        mid, t = 0.5 * (lo + hi), (hi - lo) * 2.0 ** -16
        sg = 1.0 if q[i] > 0 else -1.0
        w[i] = sg * (mid - t)
        r[i] = sg * ((0.5 * (lo2 + lo) + (lo - lo2) * 2.0 ** -16) if i in B else (mid + t))
    w[d - 1] = np.sqrt(1.0 - (w[:-1] ** 2).sum())
    r[d - 1] = np.sqrt(1.0 - (r[:-1] ** 2).sum())
    X = rs.randn(N, d)
    X[X.dot(q) > 0] *= -1.0                      # (the pair scores 0.9 |q|: no other row of a short length may come near)
    X[winner] = w
    runner = None
    if N > 1:
        runner = 0 if winner != 0 else 1         # below the winner where there is room: a tie would go wrong too
        X[runner] = r
    return X, q, {"winner": winner, "runner": runner}


def check_aligned(X, q, storage, info):
    d = X.shape[1]
    ex, st = exact_scores(X, q), stored_scores(X, q, storage)
    qn = float(np.sqrt((q * q).sum()))
    w, r = info["winner"], info["runner"]
    assert first_argmax(ex) == w
    if r is None:
        return
    gap = float(ex[w] - np.delete(ex, w).max())
    assert gap >= gap_floor(d, q) and gap < RESOLUTION[storage] * qn, (gap, gap_floor(d, q), RESOLUTION[storage] * qn)
    assert first_argmax(st) != w and st[r] > st[w], (first_argmax(st), st[r] - st[w])     # the stored order is inverted


def subnormal_case(d, N, winner, seed):
    """fp16 storage, rows of one element 1 and d - 1 elements inside fp16's subnormal range (spacing 2^-24: the absolute
    2^-25 per element of the bound); the query's weight is on the small coordinates.  The winner's small elements sit just
    below 2^-25 and all store as 0; the competitor's sit just above it on three quarters of the coordinates (stored 2^-24)
    and at 2^-26 on the others: ahead in storage, behind exactly.  The other rows have small elements of the opposite sign."""
    assert d >= 5
    rs = np.random.RandomState(seed)
    q = np.abs(_fp32_query(rs, d)) + 0.25
    q[0] = 0.0
    h = 2.0 ** -25
    X = np.empty((N, d))
    X[:, 0] = 1.0
    X[:, 1:] = -np.exp(rs.uniform(np.log(2.0 ** -26), np.log(2.0 ** -15), size=(N, d - 1)))
    X[winner, 1:] = 0.98 * h
    comp = None
    if N > 1:
        comp = 0 if winner != 0 else 1
        c = np.full(d - 1, 1.02 * h)
        c[rs.permutation(d - 1)[:max(1, (d - 1) // 4)]] = 0.5 * h
        X[comp, 1:] = c
    return X, q, {"winner": winner, "comp": comp}


def check_subnormal(X, q, info):
    d = X.shape[1]
    ex, st = exact_scores(X, q), stored_scores(X, q, "float16")
    qn = float(np.sqrt((q * q).sum()))
    w, c = info["winner"], info["comp"]
    assert first_argmax(ex) == w
    An = np.abs(X[w] / np.sqrt((X[w] ** 2).sum()))
    err_w = abs(float(st[w] - ex[w]))
    # the relative part of the fp16 rounding model alone (2^-11 |a_i| per element) does not cover the winner's stored score:
    # the absolute 2^-25 per element does
    assert err_w > 2.0 ** -11 * float(An.dot(np.abs(q))), (err_w, 2.0 ** -11 * float(An.dot(np.abs(q))))
    assert err_w <= 2.0 ** -25 * np.sqrt(d) * qn * (1 + 1e-6)
    if c is not None:
        gap = float(ex[w] - np.delete(ex, w).max())
        assert gap >= gap_floor(d, q) and gap < RESOLUTION["float16"] * qn
        assert st[c] > st[w] and first_argmax(st) == c


def negative_case(d, N, seed):
    """Every score is negative: the maximum is the least negative one."""
    rs = np.random.RandomState(seed)
    q = _fp32_query(rs, d)
    if not np.any(q):
        q[0] = 1.0
    X = rs.randn(N, d)
    s = X.dot(q)
    X[s > 0] *= -1.0
    X[s == 0] = -q
    return X, q


def padzero_case(d, storage, N, seed):
    """The query is zero on the elements of the last 16-byte piece of a row (all of it for rows of one piece but for the
    first element)."""
    rs = np.random.RandomState(seed)
    q = _fp32_query(rs, d)
    epl = EPL[storage]
    first = ((d + epl - 1) // epl - 1) * epl
    q[max(first, 1):] = 0.0
    if not np.any(q):
        q[0] = 1.0
    return rs.randn(N, d), q
