"""Host side of tests/test_gpu_front4_exact.py: what the 4-bit front pass (csrc/screen4.hip) must list, worked out without a
GPU and without the product.  Built on tools/screen4_model.py and tools/screen8_model.py (the quantisers, the query's integer
planes, e4, the row -> wave map); added here are the exact scores in long double, the threshold Lg restated from an 8-bit
shadow, the per-row upper bound U4 restated from a 4-bit shadow, the predicates the GPU test applies to a probe's list and
to its settled partials, and the adversarial inputs with the checks that they ARE adversarial (tests/
test_front4_restatement_host.py runs those on the model's own shadows; the GPU test runs them on the shadows read back, before
it probes).

Sharpness of the aligned cases, measured on the model (`python -m tests.front4_restatement`: seed 0, target row 0, rpt + 1
rows, fp32 storage), not on the kernel.  `tight` is (exact - score4) / e4 of the target row; `flip` is the largest factor on eA
at which that row is still excluded, (Lg - score4 - eB - 5e-7 |score4|) / (bound4 eA): a front pass whose eA is shorter than
that factor fails soundness on the case.  randn rows flip above 0.9 at every d; dominant (clipped) rows have a wide 8-bit
interval, Lg lies further below the exact score, and from d = 256 on they flip at or below 0.9:
      d          16     24     40    100    256    512    520   1000   2048   4096
  randn tight   0.997  0.995  0.994  0.992  0.991  0.992  0.992  0.991  0.991  0.992
  randn flip    0.969  0.948  0.941  0.929  0.934  0.926  0.926  0.930  0.923  0.923
  dominant tight 0.996 0.996  0.995  0.995  0.996  0.995  0.994  0.994  0.995  0.996
  dominant flip 0.955  0.944  0.936  0.913  0.896  0.904  0.874  0.847  0.865  0.863
"""
import math

import numpy as np

from tools import screen4_model as m4
from tools import screen8_model as m8
from tests import scan_emulation as emu
from tests.screen4_fused_cases import rows_per_trip

D_LIST = (16, 24, 40, 100, 256, 512, 520, 1000, 2048, 4096)      # one per pair of lane geometry (screen4_fused_cases.GEOMETRY)
D_SHADOW_ONLY = (1, 31, 33)
STORAGES = ("float32", "float16")
SEG_CAP = m4.SEG_CAP
EMPTY = 0x7fffffff


def row_counts(d):
    rpt = rows_per_trip(d)
    return (max(5, rpt - 1), rpt + 1, 3 * rpt + 5)


def multi_trip_rows(d):
    """More rows than 512 workgroups take in two trips: a workgroup goes round its stream loop three times."""
    rpt = rows_per_trip(d)
    return 2 * 512 * rpt + rpt + 1


# ---- arithmetic ------------------------------------------------------------------------------------------------------------
def err_coef(d, storage):
    """bcx_scan_plan's storage term (csrc/scan.hip), as the front pass receives it in fp32."""
    p = emu.scan_plan(d, storage)
    lg = int(math.log2(p["G"]))
    coef = 1.3 * 2.0 ** -24 * (emu.EPL[storage] * p["CH"] + lg + 3.0)
    if storage == "float16":
        coef += 1.02 * (2.0 ** -11 + 2.0 ** -25 * math.sqrt(d))
    return float(np.float32(coef))


def scaled_query(q):
    """(q 2^-E in fp64, the fp32 query, qscale as the kernel reads it, E): the units of apply_common.h store_query, as
    bcx_argmax_correlation sets them."""
    q = np.asarray(q, dtype=np.float64)
    m = float(np.max(np.abs(q)))
    if not (m > 0.0 and np.isfinite(m)):
        return q, q.astype(np.float32), np.float32(math.sqrt(float(np.cumsum(q * q)[-1]))), 0
    e0 = math.frexp(m)[1] - 1                                                # ilogb
    t = np.ldexp(q, -e0)
    n0 = math.sqrt(float(np.cumsum(t * t)[-1]))                              # summed in index order, as the host does
    e1 = math.frexp(n0)[1] - 1
    E = e0 + e1
    qs = np.ldexp(q, -E)
    qn = math.ldexp(n0, -e1)
    return qs, qs.astype(np.float32), np.float32(qn), E


def unpack4(raw, d):
    """Stored bytes of the 4-bit shadow -> (codes int8 [n, d], padding nibbles uint8 [n, ld - d]); the inverse of m4.pack4."""
    raw = np.asarray(raw, dtype=np.uint8)
    nib = np.empty((raw.shape[0], raw.shape[1] * 2), dtype=np.uint8)
    nib[:, 0::2] = raw & 15
    nib[:, 1::2] = raw >> 4
    return (nib[:, :d].astype(np.int16) - 8).astype(np.int8), nib[:, d:]


def interval8(s0, sc, bound, kacc, ec, qscale):
    """screen_interval (csrc/screen_core.h) in fp32."""
    f = np.float32
    with np.errstate(all="ignore"):
        e = ((sc * f(kacc) + bound).astype(f) * f(1.000002) + f(ec)).astype(f) * f(qscale)
        ee = (e + np.abs(s0) * f(2e-7)).astype(f)
        return (s0 + ee).astype(f), (s0 - ee).astype(f)


class Model(object):
    """Rows (raw fp64), their stored form and the two shadows: the model's own (from_host) or the device's (from_device)."""

    def __init__(self, X, storage, stored, shadow4, shadow8):
        self.X = np.asarray(X, dtype=np.float64)
        self.n, self.d = self.X.shape
        self.storage = storage
        self.stored = np.asarray(stored).astype(np.float32)                  # fp16 values are exact in fp32
        self.codes4, self.sc4, self.b4 = shadow4
        self.codes8, self.sc8, self.b8 = shadow8
        self.ec = err_coef(self.d, storage)
        G8, CH8 = m8.plan(self.d)
        self.kacc = float(np.float32(m8.kacc(self.d, G8, CH8)))
        self.bins, self.nbins = m4.wave_of_row4(self.n, self.d)
        self._c4f = None

    @classmethod
    def from_host(cls, X, storage):
        stored = emu.stored_rows(X, storage).astype(np.float32)
        return cls(X, storage, stored, m4.quantise4(stored), m8.quantise(stored))

    @classmethod
    def from_device(cls, X, storage, stored, raw4, shadow8):
        codes, pad = unpack4(raw4[0], X.shape[1])
        assert (pad == 8).all()
        return cls(X, storage, stored, (codes, raw4[1], raw4[2]), shadow8)

    def codes4_f32(self):
        if self._c4f is None:
            self._c4f = self.codes4.astype(np.float32)
        return self._c4f

    def residual4(self, i):
        return self.stored[i].astype(np.float64) - self.codes4[i].astype(np.float64) * float(self.sc4[i])


class Scored(object):
    """Everything the predicates need about one (query, sentinels) pair on one Model."""


def score(model, q, sentinels, eA_factor=1.0):
    """Exact scores (long double, raw rows, scaled units), Lg restated from the 8-bit shadow, U4 restated from the 4-bit one,
    and the 8-bit interval of every row.  eA_factor: the break a reviewer would make in front4_head, on the model."""
    o = Scored()
    o.q = np.asarray(q, dtype=np.float64)
    o.qs64, o.q32, o.qscale, o.E = scaled_query(o.q)
    o.sentinels = np.asarray(sentinels, dtype=np.int64)
    o.exact = emu.exact_scores(model.X, o.qs64)
    q64 = o.q32.astype(np.float64)
    d = model.d
    # 8-bit tier: integer codes times the fp32 query, summed in fp64; one rounding with the scale
    tot = (model.codes8[:, :d].astype(np.float64) - 128.0) @ q64
    o.s8 = (model.sc8.astype(np.float64) * tot).astype(np.float32)
    o.U8, o.L8 = interval8(o.s8, model.sc8, model.b8, model.kacc, model.ec, o.qscale)
    valid = o.sentinels[o.sentinels >= 0]
    x, step, qerr, _ = m4.quantise_query(o.q32)
    o.x, o.step, o.qerr = x, step, qerr
    o.qok = bool(np.isfinite(qerr))
    L = o.L8[valid]
    L = L[~np.isnan(L)]
    o.Lg = float(L.max()) if (len(L) and o.qok) else -np.inf
    eA, eB = m4.e4_coefficients(o.qscale, qerr if o.qok else np.float32(0), model.ec)
    o.eA, o.eB = np.float32(np.float32(eA_factor) * eA), eB
    o.s4 = m4.score4(model.codes4_f32(), model.sc4, x, step)
    o.e4 = m4.e4_of(o.s4, model.b4, o.eA, o.eB)
    o.U4 = m4.upper4(o.s4, model.b4, o.eA, o.eB)
    return o


def model_list(model, o, seg_cap=SEG_CAP, stride=None):
    """The probe's answer as the model gives it: counts per wave and the segments, rows in order, -1 behind them."""
    with np.errstate(invalid="ignore"):
        want = ~(o.U4 < np.float32(o.Lg))
    counts = np.bincount(model.bins[want], minlength=model.nbins).astype(np.int32)
    stride = stride or max(1, min(seg_cap, int(counts.max())))
    lst = np.full((model.nbins, stride), -1, dtype=np.int32)
    for b in np.flatnonzero(counts):
        rows = np.flatnonzero(want & (model.bins == b))[:min(seg_cap, stride)]
        lst[b, :len(rows)] = rows
    return counts, lst


def tightness(o):
    """(rows the list may hold, rows it must hold) by the front pass's own formula: U4 (1 + 4e-6) + 1e-37 >= Lg (1 - 4e-7) and
    U4 (1 - 4e-6) > Lg (1 + 4e-7).  The factors are margins on the magnitudes -- one fp32 ulp of Lg each way, the coefficients'
    roundings on U4 -- so for a negative U4 or Lg they are applied to |U4| and |Lg| (as bare factors they would narrow the
    predicates there, and the model's own list would fail them)."""
    U = o.U4.astype(np.float64)
    aU, aL = 4e-6 * np.abs(U), 4e-7 * abs(o.Lg) if np.isfinite(o.Lg) else 0.0
    may = U + aU + 1e-37 >= o.Lg - aL
    must = U - aU > o.Lg + aL
    return may, must


def undecided(o):
    """Rows between the two tightness predicates: the list may hold them or not."""
    with np.errstate(invalid="ignore"):
        may, must = tightness(o)
    return may & ~must


def band_cap(n):
    return max(2, n // 1000)


# ---- predicates on a probe ---------------------------------------------------------------------------------------------------
def segments_of(model, counts, lst, seg_cap=SEG_CAP):
    """Structure of a probe's list; returns the listed rows as a mask."""
    counts, lst = np.asarray(counts), np.asarray(lst)
    assert len(counts) == model.nbins == lst.shape[0], (len(counts), model.nbins)
    listed = np.zeros(model.n, dtype=bool)
    per_wave = np.bincount(model.bins, minlength=model.nbins)
    for b in range(model.nbins):
        c = int(counts[b])
        assert 0 <= c <= per_wave[b] and c <= seg_cap, ("count", b, c)
        seg = lst[b, :c]
        assert len(seg) == c and (lst[b, c:] == -1).all(), ("entries returned", b)
        if c == 0:
            continue
        assert (seg >= 0).all() and (seg < model.n).all(), ("range", b, seg)
        assert (np.diff(seg) > 0).all(), ("order", b, seg)
        assert (model.bins[seg] == b).all(), ("wave", b, seg)
        listed[seg] = True
    return listed


def check_list(model, o, counts, lst):
    """Section (b): structure, soundness against exact arithmetic, tightness against the front pass's own formula."""
    listed = segments_of(model, counts, lst)
    with np.errstate(invalid="ignore"):
        must_exact = np.asarray(o.exact >= np.longdouble(o.Lg + 4e-7 * abs(o.Lg) + 1e-37))
        may, must = tightness(o)
    missing = np.flatnonzero(must_exact & ~listed)
    assert len(missing) == 0, ("soundness: rows at or above Lg are not listed", missing[:8], o.Lg)
    extra = np.flatnonzero(listed & ~may)
    assert len(extra) == 0, ("tightness: listed rows whose U4 is below Lg", extra[:8], o.U4[extra[:8]], o.Lg)
    short = np.flatnonzero(must & ~listed)
    assert len(short) == 0, ("tightness: rows whose U4 is above Lg are not listed", short[:8], o.U4[short[:8]], o.Lg)
    return listed


def check_all_listed(model, counts, lst):
    """Section (c): no threshold, every row listed, the segments are the rows of each wave in order."""
    listed = segments_of(model, counts, lst)
    assert listed.all() and np.array_equal(counts, np.bincount(model.bins, minlength=model.nbins))
    return listed


def same_shadow8(model, a, b):
    return bool(model.sc8[a] == model.sc8[b] and model.b8[a] == model.b8[b] and np.array_equal(model.codes8[a], model.codes8[b]))


def check_settle(model, o, counts, lst, P, seg_cap=SEG_CAP):
    """Section (d): the per-wave partials against the 8-bit restatement of the listed rows.  Returns the number of waves whose
    order of i1 / i2 the accumulation order leaves open."""
    opened = 0
    slack_all = 2.0 * model.sc8.astype(np.float64) * model.kacc * float(o.qscale)
    U8 = o.U8.astype(np.float64)
    for b in range(model.nbins):
        c = int(counts[b])
        got = [float(P[k][b]) for k in ("U1", "U2", "U3", "L")] + [int(P["i1"][b]), int(P["i2"][b])]
        if c > seg_cap:
            assert got == [-np.inf, -np.inf, np.inf, -np.inf, EMPTY, EMPTY], ("overflow partial", b, got)
            continue
        if c == 0:
            assert got == [-np.inf, -np.inf, -np.inf, -np.inf, EMPTY, EMPTY], ("empty segment", b, got)
            continue
        rows = np.asarray(lst[b, :c], dtype=np.int64)
        U1, U2, U3, L, i1, i2 = got
        ex = o.exact[rows]
        top = ex.max()
        assert U1 >= top and L <= top, ("U1 / L", b, U1, L, float(top))
        order = rows[np.lexsort((rows, -U8[rows]))]
        assert i1 in rows, ("i1", b, i1)
        assert abs(U1 - U8[i1]) <= slack_all[i1] + 1e-6 * abs(U1), ("U1 restated", b, U1, U8[i1])
        if c == 1:
            assert U2 == -np.inf and U3 == -np.inf and i2 == EMPTY and i1 == rows[0], ("one row", b, got)
            continue
        assert i2 in rows and i2 != i1, ("i2", b, i2)
        assert U2 >= o.exact[i2], ("U2", b)
        rest = rows[(rows != i1) & (rows != i2)]
        if c == 2:
            assert U3 == -np.inf, ("two rows", b, got)
        else:
            assert np.isfinite(U3) and U3 >= o.exact[rest].max(), ("U3", b, U3)
        if (i1, i2) != (order[0], order[1]):
            # open only between rows whose restated bounds are closer than the accumulation-order term 2 scale kacc qs (of the
            # row with the larger scale); rows that are bit-identical in the shadow get bit-identical bounds from the kernel,
            # so between them the lower index must win
            close = lambda a, r: abs(U8[a] - U8[r]) <= max(slack_all[a], slack_all[r])
            assert close(i1, order[0]) and close(i2, order[1]), ("i1 / i2", b, (i1, i2), order[:3], U8[order[:3]])
            for pick, allowed in ((i1, ()), (i2, (i1,))):
                for p in rows[rows < pick]:
                    if p not in allowed and same_shadow8(model, p, pick):
                        raise AssertionError(("tie: the higher of two identical rows was ranked first", b, int(p), pick))
            opened += 1
    return opened


# ---- rows ----------------------------------------------------------------------------------------------------------------------
def make_rows(kind, rs, n, d):
    if kind == "randn":
        return rs.randn(n, d)
    if kind == "dominant":            # one element far above the rest: clipping at 0.8 max|a| is active
        X = rs.randn(n, d)
        X[np.arange(n), rs.randint(0, d, size=n)] = 40.0 * (1 + rs.rand(n))
        return X
    if kind == "constant":
        return np.outer(rs.uniform(0.5, 2.0, size=n) * rs.choice([-1.0, 1.0], size=n), np.ones(d))
    if kind == "onehot":
        X = np.zeros((n, d))
        X[np.arange(n), rs.randint(0, d, size=n)] = rs.uniform(0.5, 2.0, size=n) * rs.choice([-1.0, 1.0], size=n)
        return X
    raise AssertionError(kind)


def check_dominant(model, rows):
    """Clipping is active: the largest element lies beyond 7 scale4."""
    assert (np.abs(model.stored[rows]).max(axis=1) > 7.0 * model.sc4[rows]).all()


def shadow_rows(storage, d, seed=0):
    """Rows of test (a): every kind, N no multiple of 4."""
    rs = np.random.RandomState(seed + d)
    parts = [("randn", make_rows("randn", rs, 9, d)), ("dominant", make_rows("dominant", rs, 6, d)),
             ("constant", make_rows("constant", rs, 3, d)), ("onehot", make_rows("onehot", rs, 3, d)),
             ("big", np.ldexp(rs.randn(3, d), 100)), ("small", np.ldexp(rs.randn(3, d), -100))]
    if storage == "float16":
        # normalised elements in fp16's subnormal range (below 2^-14): one element carries the norm
        S = rs.randn(3, d) * 2.0 ** -18
        S[:, 0] = 1.0
        parts.append(("subnormal", S))
    kinds = np.concatenate([[k] * len(x) for k, x in parts])
    X = np.concatenate([x for _, x in parts])
    assert len(X) % 4 != 0
    return X, kinds


def duplicate_rows(X, src, copy, doubled):
    X[copy] = X[src]
    X[doubled] = 2.0 * X[src]
    return X


# ---- cases: (query, sentinels) -----------------------------------------------------------------------------------------------
def aligned_case(model, target):
    """The query along the target row's own 4-bit residual a~ - deq4, that row the only sentinel: Cauchy-Schwarz in term (3) of
    the enclosure is an equality, so the exact score sits at the top of [score4 - e4, score4 + e4].  The largest factor on eA
    at which the row is still excluded, per d, for randn and for dominant rows: the table at the head of this file."""
    r = model.residual4(target)
    q = 1.37 * r / np.sqrt((r * r).sum())      # (not a unit vector: its exponent must not hang on the last bit of its norm)
    sent = np.full(64, -1, dtype=np.int32)
    sent[0] = target
    return q, sent


def flip_factor(o, model, t):
    """Largest factor on eA at which row t is still excluded: (Lg - score4 - eB - 5e-7 |score4|) / (bound4 eA)."""
    return (o.Lg - float(o.s4[t]) - float(o.eB) - 5e-7 * abs(float(o.s4[t]))) / (float(model.b4[t]) * float(o.eA))


def check_aligned(model, o, target, randn):
    t = target
    tight = (float(o.exact[t]) - float(o.s4[t])) / float(o.e4[t])
    assert tight >= 0.95, ("aligned: the exact score is not at the edge of e4", tight)
    assert float(o.exact[t]) >= o.Lg, ("aligned: the target is below its own threshold", float(o.exact[t]), o.Lg)
    f = flip_factor(o, model, t)
    if randn:
        assert f > 0.9, ("aligned: the row would still be listed with 0.9 eA", f)
        short = score(model, o.q, o.sentinels, eA_factor=0.9)
        assert short.U4[t] < np.float32(short.Lg)
    return tight, f


def query_tail_case(d, rs):
    """Term (2), qerr: the last query element is 2^13 times the others, which therefore all quantise to zero, and a row
    supported on those others with their signs (the first one positive).  score4 of the row is exactly zero, its exact score is
    close to ||q_small|| = qerr: all of it must come out of e4's qerr terms and the row's bound.  Returns (query, row)."""
    q = rs.uniform(1.0, 2.0, size=d) * rs.choice([-1.0, 1.0], size=d)
    q[0] = abs(q[0])
    q[d - 1] = 2.0 ** 13 * 1.5
    row = np.sign(q) * rs.uniform(0.5, 1.0, size=d)
    row[d - 1] = 0.0
    return q, row


def check_query_tail(model, o, target):
    t = target
    support = model.X[t] != 0
    assert (o.x[support] == 0).all() and float(o.s4[t]) == 0.0, "query tail: the small elements do not quantise to zero"
    assert float(o.exact[t]) > 0 and float(o.exact[t]) >= o.Lg
    assert float(o.qerr) > 0 and float(o.exact[t]) >= 0.8 * float(o.qerr), ("query tail: the row is not along the rounding error",
                                                                           float(o.exact[t]), float(o.qerr))


def random_query(rs, d):
    return rs.randn(d)


def random_sentinels(rs, n):
    return rs.randint(0, n, size=64).astype(np.int32)


def one_sentinel(row, copies=1):
    s = np.full(64, -1, dtype=np.int32)
    s[64 - copies:] = row
    return s


def picked_sentinels(model, other):
    """The rows refine_kernel would leave after an iteration with query `other` (m4.pick_sentinels on its 8-bit upper bounds)."""
    o = score(model, other, np.full(64, -1))
    rows = m4.pick_sentinels(o.U8.astype(np.float64), np.arange(model.n), model.bins, model.nbins)
    s = np.full(64, -1, dtype=np.int32)
    s[:len(rows)] = rows[:64]
    return s


def positive_first_column(X):
    """Rows whose first element is positive, so that the query -e_0 scores every row below zero."""
    X[:, 0] = np.abs(X[:, 0]) + 0.5
    return X


def negative_query(model):
    q = np.zeros(model.d)
    q[0] = -1.0
    return q


def check_negative(o):
    assert (o.exact < 0).all(), "negative query: a row scores at or above zero"


def edge_targets(model):
    """First row, last row, and the rows either side of the first trip edge."""
    rpt = rows_per_trip(model.d)
    t = [0, model.n - 1]
    if model.n > rpt:
        t += [rpt - 1, rpt]
    return t


def check_band(model, o):
    k = int(undecided(o).sum())
    assert k <= band_cap(model.n), ("undecided band", k, band_cap(model.n))
    return k


# ---- the rows and the probes of one shape ----------------------------------------------------------------------------------------
def list_rows(d, n, seed):
    """Rows of tests (b) to (d) at one shape: randn rows with a positive first element; the first row, the last row and the rows
    either side of the first trip edge stay randn (aligned targets), their inner neighbours are dominant rows (aligned targets of
    the clipped kind), one row is rewritten for the query-tail case, and three rows are a row, its copy and its double."""
    assert n >= 15
    rs = np.random.RandomState(seed)
    X = positive_first_column(rs.randn(n, d))
    rpt = rows_per_trip(d)
    info = {"randn": [0, n - 1], "dominant": [1, n - 2]}
    if n > rpt + 2:
        info["randn"] += [rpt - 1, rpt]
        info["dominant"] += [rpt - 2, rpt + 1]
    X[info["dominant"]] = positive_first_column(make_rows("dominant", rs, len(info["dominant"]), d))
    taken = set(info["randn"] + info["dominant"])
    free = [i for i in range(n) if i not in taken]
    tail, src, copy, doubled = free[0], free[1], free[len(free) // 2], free[-1]
    tq, X[tail] = query_tail_case(d, rs)
    duplicate_rows(X, src, copy, doubled)
    info.update({"tail": tail, "tail_query": tq, "duplicates": (src, copy, doubled), "seed": seed})
    return X, info


def build_probes(model, info):
    """[(name, Scored)] of one shape, every precondition and the cap of the undecided band asserted.  `same_as` in a Scored names
    the probe whose list this one must repeat."""
    rs = np.random.RandomState(info["seed"] + 1)
    n, d = model.n, model.d
    out = []

    def add(name, q, sent, same_as=None):
        o = score(model, q, sent)
        o.name, o.same_as = name, same_as
        o.band = check_band(model, o)
        out.append((name, o))
        return o

    q0, q1 = random_query(rs, d), random_query(rs, d)
    s0 = random_sentinels(rs, n)
    add("random0/random64", q0, s0)
    add("random1/picked", q1, picked_sentinels(model, q0))
    add("random0*2^300", np.ldexp(q0, 300), s0, same_as="random0/random64")
    add("random0*2^-300", np.ldexp(q0, -300), s0, same_as="random0/random64")
    add("random1/one", q1, one_sentinel(int(rs.randint(0, n))))
    add("random1/same64", q1, one_sentinel(int(rs.randint(0, n)), copies=64))
    for kind in ("randn", "dominant"):
        if kind == "dominant":
            check_dominant(model, info["dominant"])
        for t in info[kind]:
            q, sent = aligned_case(model, t)
            o = add("aligned_%s/%d" % (kind, t), q, sent)
            o.tight, o.flip = check_aligned(model, o, t, kind == "randn")
    sent = one_sentinel(info["tail"])
    check_query_tail(model, add("query_tail", info["tail_query"], sent), info["tail"])
    check_negative(add("negative/random64", negative_query(model), random_sentinels(rs, n)))
    return out


def multi_trip_probes(model):
    """[(name, Scored)] of a multi-trip shape (list_rows(d, multi_trip_rows(d), 3 d)): one random query with picked sentinels and
    the aligned query of the first row of the second trip, preconditions and band cap asserted."""
    d = model.d
    assert model.n == multi_trip_rows(d) and model.nbins == 2048
    rs = np.random.RandomState(d)
    q = rs.randn(d)
    out = [("random", score(model, q, picked_sentinels(model, rs.randn(d))))]
    t = 512 * rows_per_trip(d)
    qa, sa = aligned_case(model, t)
    oa = score(model, qa, sa)
    oa.tight, oa.flip = check_aligned(model, oa, t, True)
    out.append(("aligned", oa))
    for _, o in out:
        o.band = check_band(model, o)
    return out


def check_duplicates(info, listed):
    src, copy, doubled = info["duplicates"]
    assert listed[src] == listed[copy] == listed[doubled], ("duplicates", listed[[src, copy, doubled]])


if __name__ == "__main__":
    for kind in ("randn", "dominant"):
        out = []
        for d in D_LIST:
            rs = np.random.RandomState(0)
            mod = Model.from_host(make_rows(kind, rs, row_counts(d)[1], d), "float32")
            q, sent = aligned_case(mod, 0)
            o = score(mod, q, sent)
            out.append("%d: tight %.3f flip %.3f" % ((d,) + check_aligned(mod, o, 0, False)))
        print(kind, "  ".join(out))
