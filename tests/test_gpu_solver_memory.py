"""GPU: a solver gives back every byte of device memory it took.

csrc/dev_buf.hip counts the bytes that the solver's buffers (DevBuf, csrc/dev_buf.h) hold; the count is exact and belongs to
this process, so it needs no tolerance and other jobs on the card cannot disturb it.  Every case runs three times, and after
each close() the count has to be what it was before the first run.  The cases walk the buffers that come and go on demand: both
screening tiers (built, then rebuilt in place after a reload), the upload staging buffer, the slots and the Gram system growing
256 -> 512, the scratch of optimize() and its warm start, the trace, and a handle that never saw a row.
"""
import ctypes
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bc():
    import bayesiancoresets_amd as bc
    return bc


@pytest.fixture(scope="module")
def live_bytes(bc):
    from bayesiancoresets_amd import _native
    lib = _native.load()
    fn = lib.bcx_debug_live_device_bytes      # an unlisted debug entry point: bound here, not in _native.SYMBOLS
    fn.restype, fn.argtypes = ctypes.c_int64, []
    return fn


@pytest.fixture(scope="module")
def rows():
    """The small shapes of tests/screen4_cases.py (the 4-bit front pass runs on them), and one with d = 512 for OMP."""
    return {"fw": np.random.RandomState(5).randn(65536, 128), "giga": np.random.RandomState(9).randn(30000, 64),
            "omp": np.random.RandomState(11).randn(4000, 512)}


def _fw_both_tiers(bc, rows):
    X = rows["fw"]
    b = X.sum(axis=0)
    s = bc.snnls.FrankWolfe(X.T, b, dtype="float32", keep_exact_rows=True)
    s.build(30)
    st = s._eng.screen_stats()
    assert st["front4_iterations"] > 0, st
    s._eng.load_host_rows(X)                  # a reload from row 0: both shadows are rebuilt where they are
    assert s._eng.finalize(b) == 0
    s.build(30)
    assert s._eng.screen_stats()["front4_iterations"] > st["front4_iterations"]
    s.reset()
    s._eng.close()


def _fw_staged_upload(bc, rows):
    X = rows["fw"]
    s = bc.snnls.FrankWolfe(X.T, X.sum(axis=0), keep_exact_rows=False)     # host rows without a resident fp64 copy: staged
    s.build(10)
    s._eng.close()


def _omp_growth_and_optimize(bc, rows):
    X = rows["omp"]
    s = bc.snnls.OrthoPursuit(X.T, X.sum(axis=0))
    s.build(200)
    s.build(200)                              # room for 400 slots is asked for: the slot arrays and the Gram system grow 256 -> 512
    s.optimize()
    s._eng.close()


def _giga_no_reset(bc, rows):
    X = rows["giga"]
    s = bc.snnls.GIGA(X.T, X.sum(axis=0))
    s.build(20)
    assert np.isfinite(s.error())
    s._eng.close()


def _never_loaded(bc, rows):
    from bayesiancoresets_amd import _native
    _native.Engine(_native.ALG_FW, 5000, 64).close()


@pytest.mark.parametrize("case", (_fw_both_tiers, _fw_staged_upload, _omp_growth_and_optimize, _giga_no_reset, _never_loaded),
                         ids=lambda f: f.__name__.lstrip("_"))
def test_close_returns_every_byte(bc, live_bytes, rows, case):
    gc.collect()                              # solvers that earlier tests dropped go now, not in the middle of the count
    before = live_bytes()
    from bayesiancoresets_amd import _native
    held = _native.Engine(_native.ALG_FW, 5000, 64)
    assert live_bytes() >= before + 5000 * 64 * 4      # the count moves: a solver that lives holds at least its rows
    held.close()
    assert live_bytes() == before
    for run in range(3):
        case(bc, rows)
        after = live_bytes()
        print(case.__name__, "run", run, "live bytes before", before, "after", after)
        assert after == before, (run, before, after)
