"""GPU: the 4-bit front pass itself (csrc/screen4.hip: quantise4_kernel, front4_kernel with front4_head and settle8) against
exact arithmetic, kernel by kernel, through the two diagnostic entries bcx_screen4_read and bcx_screen4_probe.  The host side
is tests/front4_restatement.py (its preconditions run without a GPU in tests/test_front4_restatement_host.py); here they are
asserted once more on the shadows read back from the device before the kernel is asked anything.

(a) the shadow equals tools/screen4_model.py's quantiser on the stored rows, byte for byte, padding included, and bound4 covers
    the long-double residual;  (b) the list holds every row whose exact score reaches the restated threshold and no row the
front pass's own formula excludes;  (c) without a threshold every row is listed;  (d) the partials the second stage writes
enclose the exact scores of the listed rows and name the rows the 8-bit restatement names;  (e) a probe leaves no trace in a
build.

Run time on one MI355X: the whole file (125 tests) 13 s.  The slowest are the two multi-trip cases, 2.9 s (d = 16, 2 099 201
rows) and 3.7 s (d = 4096, 16 401 rows), nearly all of it the long-double restatement on the host, so both are kept; the shared
probes of one (handle, d) take 0.1 to 0.2 s, every other test less.
"""
import os

import numpy as np
import pytest

from tests import front4_restatement as fr
from tools import screen4_model as m4
from tools import screen8_model as m8

pytestmark = pytest.mark.gpu

HANDLES = (("fw", "float32"), ("omp", "float16"), ("fw", "float16"), ("omp", "float32"))


@pytest.fixture(scope="module")
def bc():
    import bayesiancoresets_amd as bc
    return bc


def _solver(bc, X, alg, dtype):
    cls = {"fw": bc.snnls.FrankWolfe, "omp": bc.snnls.OrthoPursuit}[alg]
    s = cls(X.T, X.sum(axis=0), dtype=dtype)
    assert os.environ.get("BCX_SCREEN4") is None and s._eng.screen_stats()["front4_active"]
    return s


def _device_model(s, X, dtype):
    eng = s._eng
    return fr.Model.from_device(X, dtype, eng.stored_rows().astype(np.float32), eng.screen4_read(), eng.screen_read())


def _probe(eng, model, o_or_q, sentinels=None):
    q = o_or_q.q if sentinels is None else o_or_q
    sent = o_or_q.sentinels if sentinels is None else sentinels
    stride = min(fr.SEG_CAP, int(np.bincount(model.bins).max()))
    return eng.screen4_probe(q, np.asarray(sent, dtype=np.int32), list_stride=stride)


# ---- (a) the shadow ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", fr.STORAGES)
@pytest.mark.parametrize("d", fr.D_LIST + fr.D_SHADOW_ONLY)
def test_shadow_equals_the_model_quantiser(bc, d, dtype):
    X, kinds = fr.shadow_rows(dtype, d)
    s = _solver(bc, X, "fw", dtype)
    raw, sc, bd = s._eng.screen4_read()
    stored = s._eng.stored_rows()
    if dtype == "float16" and d > 1:
        sub = np.abs(stored[kinds == "subnormal"][:, 1:].astype(np.float64))
        assert ((sub < 2.0 ** -14) & (sub > 0)).any()           # elements in the subnormal range of the stored type
    stored = stored.astype(np.float32)
    c2, s2, b2 = m4.quantise4(stored)
    assert raw.shape == (len(X), (d + 31) // 32 * 16)
    assert np.array_equal(raw, m4.pack4(c2)), "codes or padding nibbles"
    assert np.array_equal(sc.view(np.uint32), s2.view(np.uint32)), "scale4"
    if d > 1:
        dom = np.flatnonzero(kinds == "dominant")
        assert (np.abs(stored[dom]).max(axis=1) > 7.0 * s2[dom]).all()      # clipping is active
    res = np.sqrt(((stored.astype(np.longdouble) - c2.astype(np.longdouble) * s2.astype(np.longdouble)[:, None]) ** 2).sum(axis=1))
    print(d, dtype, "bound4 / residual - 1: max %.3g" % float(np.max(bd / np.maximum(res, np.longdouble(1e-300)) - 1)))
    assert (bd.astype(np.longdouble) >= res).all()
    assert (bd.astype(np.longdouble) <= res * (1 + 4e-6) + 1e-37).all()
    # a sub-range reads the same rows
    r2, sc2, bd2 = s._eng.screen4_read(3, 5)
    assert np.array_equal(r2, raw[3:8]) and np.array_equal(sc2, sc[3:8]) and np.array_equal(bd2, bd[3:8])


# ---- (b) and (d): one set of probes per shape, shared ---------------------------------------------------------------------------
_shapes = {}


def _shape(bc, alg, dtype, d):
    key = (alg, dtype, d)
    if key not in _shapes:
        runs = []
        for k, n in enumerate(fr.row_counts(d)):
            X, info = fr.list_rows(d, n, 100 * d + k)
            s = _solver(bc, X, alg, dtype)
            model = _device_model(s, X, dtype)
            probes = fr.build_probes(model, info)                 # preconditions, on the shadows as read back
            runs.append((model, info, [(name, o, _probe(s._eng, model, o)) for name, o in probes]))
        _shapes[key] = runs
    return _shapes[key]


@pytest.mark.parametrize("alg,dtype", HANDLES)
@pytest.mark.parametrize("d", fr.D_LIST)
def test_list_is_sound_and_tight(bc, d, alg, dtype):
    for model, info, probes in _shape(bc, alg, dtype, d):
        by_name = {}
        for name, o, P in probes:
            listed = fr.check_list(model, o, P["counts"], P["list"])
            fr.check_duplicates(info, listed)
            by_name[name] = P
            if o.same_as:
                assert np.array_equal(P["counts"], by_name[o.same_as]["counts"]) and np.array_equal(P["list"], by_name[o.same_as]["list"]), name
            if hasattr(o, "tight"):
                print(d, dtype, model.n, name, "tight %.3f flip %.3f listed %d" % (o.tight, o.flip, listed.sum()))


@pytest.mark.parametrize("alg,dtype", HANDLES)
@pytest.mark.parametrize("d", fr.D_LIST)
def test_settled_partials_enclose_the_listed_rows(bc, d, alg, dtype):
    for model, info, probes in _shape(bc, alg, dtype, d):
        total = 0
        for name, o, P in probes:
            opened = fr.check_settle(model, o, P["counts"], P["list"], P)
            assert opened <= fr.band_cap(model.n), (name, opened)
            total += opened
        print(d, dtype, model.n, "waves whose i1 / i2 order was open, over %d probes:" % len(probes), total)


def test_special_segments_were_met(bc):
    """Empty, one-row, two-row and three-row segments all occur among the probes (check_settle holds each to its partial)."""
    sizes = set()
    for d in (16, 4096):
        for model, info, probes in _shape(bc, "fw", "float32", d):
            for name, o, P in probes:
                fr.check_settle(model, o, P["counts"], P["list"], P)
                sizes.update(int(c) for c in np.unique(P["counts"]))
    assert {0, 1, 2, 3} <= sizes, sorted(sizes)[:8]


# ---- (c) no threshold -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", fr.D_LIST)
def test_nothing_is_excluded_without_a_threshold(bc, d):
    from bayesiancoresets_amd import _native
    n = fr.row_counts(d)[1]
    X, info = fr.list_rows(d, n, 5 * d)
    s = _solver(bc, X, "fw" if d % 16 else "omp", "float32")
    model = _device_model(s, X, "float32")
    rs = np.random.RandomState(d)
    q = rs.randn(d)
    some = fr.random_sentinels(rs, n)
    nan_q, inf_q = q.copy(), q.copy()
    nan_q[d // 2] = np.nan
    inf_q[d - 1] = -np.inf
    for name, qq, sent in (("no sentinels", q, np.full(64, -1)), ("zero query", np.zeros(d), some), ("NaN", nan_q, some),
                           ("Inf", inf_q, some)):
        P = _probe(s._eng, model, qq, sent)
        fr.check_all_listed(model, P["counts"], P["list"])
    before = _probe(s._eng, model, q, some)
    for bad in (n, -2, 2 ** 31 - 1):
        sent = some.copy()
        sent[17] = bad
        with pytest.raises(_native.EngineError) as e:
            _probe(s._eng, model, q, sent)
        assert e.value.code == _native.ERR_ARG
    after = _probe(s._eng, model, q, some)
    for k in before:
        assert np.array_equal(before[k], after[k], equal_nan=True), k


# ---- (d) overflow -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", (16, 512, 4096))
def test_overflowing_segments_write_the_overflow_partial(bc, d):
    n = fr.row_counts(d)[2]
    X, info = fr.list_rows(d, n, 9 * d)
    os.environ["BCX_SCREEN4_SEGCAP"] = "3"
    try:
        s = _solver(bc, X, "fw", "float32")
    finally:
        os.environ.pop("BCX_SCREEN4_SEGCAP", None)
    model = _device_model(s, X, "float32")
    q = np.random.RandomState(d).randn(d)
    P = _probe(s._eng, model, q, np.full(64, -1))
    per_wave = np.bincount(model.bins, minlength=model.nbins)
    assert np.array_equal(P["counts"], per_wave) and (per_wave > 3).any()
    o = fr.score(model, q, np.full(64, -1))
    for b in range(model.nbins):
        rows = np.flatnonzero(model.bins == b)
        assert np.array_equal(P["list"][b, :3], rows[:3]) if len(rows) >= 3 else np.array_equal(P["list"][b, :len(rows)], rows)
        assert (P["list"][b, 3:] == -1).all()
    fr.check_settle(model, o, P["counts"], P["list"], P, seg_cap=3)


# ---- multi-trip: a workgroup goes round its stream loop more than once ----------------------------------------------------------
@pytest.mark.parametrize("d", (16, 4096))
def test_more_than_one_trip(bc, d):
    n = fr.multi_trip_rows(d)
    assert n > 2 * 512 * fr.rows_per_trip(d)
    X, info = fr.list_rows(d, n, 3 * d)
    s = _solver(bc, X, "fw", "float32")
    model = _device_model(s, X, "float32")
    assert model.nbins == 2048
    for name, o in fr.multi_trip_probes(model):                    # preconditions, on the shadows as read back
        P = _probe(s._eng, model, o)
        listed = fr.check_list(model, o, P["counts"], P["list"])
        opened = fr.check_settle(model, o, P["counts"], P["list"], P)
        print(d, n, name, "listed", int(listed.sum()), "open", opened)
        assert opened <= fr.band_cap(n)


# ---- (e) the probe leaves no trace ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ("fw", "omp"))
def test_probe_leaves_no_trace(bc, alg):
    from bayesiancoresets_amd import _native
    rs = np.random.RandomState(12)
    X = rs.randn(9001, 256)
    q = rs.randn(256)
    sent = fr.random_sentinels(rs, 9001)

    def run(probing):
        s = _solver(bc, X, alg, "float32")
        out = []
        if probing:
            s._eng.screen4_probe(q, sent, list_stride=64)
        for k in range(2):
            s.build(8)
            out += [np.array(x) for x in s.last_trace]
            if probing and k == 0:
                s._eng.screen4_probe(q, sent, list_stride=64)
        return out + [np.array(s.weights()), np.array(s.error())], s._eng.screen_stats()

    plain, st0 = run(False)
    probed, st1 = run(True)
    for a, b in zip(plain, probed):
        assert np.array_equal(a, b)
    st0.pop("build_us"), st1.pop("build_us")
    assert st0 == st1 and st0["front4_iterations"] > 0
    # with iterations enqueued and not polled the probe refuses
    s = _solver(bc, X, alg, "float32")
    assert not s._eng.build_begin(4, 0.0)
    s._eng.enqueue(4)
    with pytest.raises(_native.EngineError) as e:
        s._eng.screen4_probe(q, sent, list_stride=64)
    assert e.value.code == _native.ERR_STATE
    s._eng.poll()
    s._eng.screen4_probe(q, sent, list_stride=64)
    # so does a reset in place of the poll
    assert not s._eng.build_begin(4, 0.0)
    s._eng.enqueue(4)
    s._eng.reset()
    s._eng.screen4_probe(q, sent, list_stride=64)


def test_entries_refuse_where_the_front_pass_does_not_apply(bc):
    from bayesiancoresets_amd import _native
    X = np.random.RandomState(1).randn(200, 40)
    for make in (lambda: bc.snnls.GIGA(X.T, X.sum(axis=0), dtype="float32"), lambda: bc.snnls.FrankWolfe(X.T, X.sum(axis=0), dtype="float64")):
        s = make()
        for call in (lambda: s._eng.screen4_read(), lambda: s._eng.screen4_probe(np.ones(40), np.full(64, -1))):
            with pytest.raises(_native.EngineError) as e:
                call()
            assert e.value.code == _native.ERR_STATE
