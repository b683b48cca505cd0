"""CPU-only: the host side of bcx_nuts_batch (csrc/nuts.hip) -- the size of the problem table, the binding, and
every refusal that needs no device, each with BCX_ERR_ARG and a message of its own.  (tests/test_abi.py holds the header, the
exports and the binding list to one another.)"""
import ctypes
import inspect

import pytest


def test_table_bytes():
    from bayesiancoresets_amd import _native
    tb = _native.load().bcx_nuts_batch_table_bytes
    assert tb.restype is ctypes.c_int64
    record = ctypes.sizeof(_native.NutsProblem)
    assert record == 56 and _native.NutsProblem.k.offset == 48 and _native.NutsProblem.index.offset == 52
    for bad in (0, -1, -2 ** 31):
        assert tb(bad) == -1
    for P in (1, 2, 7, 1000, 2 ** 31 - 1):
        assert tb(P) == P * record


def test_binding():
    from bayesiancoresets_amd import _native
    lib = _native.load()
    vp, i32, i64, dbl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    single = list(lib.bcx_nuts_adapt.argtypes)
    # bcx_nuts_adapt's arguments with the problem's own (k, weights, rows, frame) in the records (their array: an address, as every
    # pointer of the header) and no fixed_eps
    assert list(lib.bcx_nuts_batch.argtypes) == [vp, i32, i32, vp, vp, i32] + single[10:15] + single[16:]
    assert single[15] is dbl and single[2] is i32 and single[6] is i64
    assert lib.bcx_nuts_batch.restype is ctypes.c_int


def test_bad_arguments_are_refused_before_any_launch():
    from bayesiancoresets_amd import _native
    lib = _native.load()
    one, D, C, J, P = ctypes.c_void_p(8), 4, 8, 3, 3             # (never dereferenced: the checks come first)
    R = D + 3 * J + 2 * (2 ** J - 1)

    def records(**kw):
        rec = (_native.NutsProblem * P)()
        for p in range(P):
            rec[p].w_dev, rec[p].pts_dev, rec[p].ldp, rec[p].mu_dev, rec[p].W_dev, rec[p].ldw, rec[p].k = 8, 8, D, 8, 8, D, 5 + p
        for name, value in kw.items():
            setattr(rec[1], name, value)
        return rec

    names = ("stream", "family", "P", "problems", "table", "D", "chains", "n_warmup", "n_samples", "max_depth", "eps0", "noise", "noise_ld",
             "ld", "samples", "xi", "prop", "diag", "accept", "eps", "status", "metric", "frames", "metric_out")
    good = dict(stream=None, family=0, P=P, problems=records(), table=one, D=D, chains=C, n_warmup=2, n_samples=2, max_depth=J, eps0=0.5,
                noise=one, noise_ld=R, ld=D, samples=one, xi=None, prop=None, diag=one, accept=one, eps=one, status=one, metric=0,
                frames=None, metric_out=None)
    whole = (dict(family=2), dict(D=0), dict(D=33, ld=33), dict(ld=D - 1), dict(ld=33), dict(chains=0), dict(n_warmup=0, n_samples=0),
             dict(n_warmup=-1), dict(eps0=0.0), dict(noise=None), dict(samples=None), dict(diag=None), dict(accept=None), dict(eps=None),
             dict(status=None), dict(P=0), dict(P=-1), dict(P=2 ** 30, chains=4), dict(problems=None), dict(table=None), dict(max_depth=0),
             dict(max_depth=11), dict(noise_ld=R - 1), dict(metric=3), dict(metric=-1), dict(metric=1), dict(metric=2, frames=one),
             dict(metric=1, metric_out=one), dict(frames=one), dict(metric_out=one))
    for kw in whole:
        args = [dict(good, **kw)[n] for n in names]
        assert lib.bcx_nuts_batch(*args) == _native.ERR_ARG, kw
        text = lib.bcx_project_last_error()
        assert text.startswith(b"bcx_nuts_batch: bad arguments") and len(text) > 60, kw
    # one problem's own: named by its place in the caller's array, the others' are fine
    for family, kw in ((0, dict(k=-1)), (0, dict(ldp=D - 1)), (1, dict(ldp=D)), (0, dict(ldw=D - 1)), (0, dict(pts_dev=None))):
        args = [dict(good, family=family, problems=records(**kw))[n] for n in names]
        if family == 1:
            for p in (0, 2):
                args[3][p].ldp = D + 1
        assert lib.bcx_nuts_batch(*args) == _native.ERR_ARG, kw
        assert lib.bcx_project_last_error().startswith(b"bcx_nuts_batch: problem 1: bad arguments"), kw
    # k = 0 needs no rows; a NULL frame is the identity: with good arguments the refusal is the device's (there is none here), and it
    # is a problem's -- the table was not touched, nothing was launched
    import torch
    if not torch.cuda.is_available():
        args = [dict(good, problems=records(k=0, pts_dev=None, W_dev=None, ldw=0))[n] for n in names]
        assert lib.bcx_nuts_batch(*args) == _native.ERR_ARG
        assert lib.bcx_project_last_error().startswith(b"bcx_nuts_batch: problem 0: 5 points of 4 parameters are outside bcx_nuts_coreset_ok")
        args = [dict(good, metric=2, frames=one, metric_out=one)[n] for n in names]
        assert lib.bcx_nuts_batch(*args) == _native.ERR_ARG
        assert b"outside bcx_nuts_adapt_ok" in lib.bcx_project_last_error()


def test_method_signature_needs_no_gpu():
    import bayesiancoresets_amd as bc
    p = inspect.signature(bc.DeviceHMC.sample_many).parameters
    assert list(p) == ["self", "problems", "n_samples", "n_warmup", "seeds", "keep_trace"]
    assert p["n_warmup"].default is None and p["seeds"].default is None and p["keep_trace"].default is False
    assert p["seeds"].kind is inspect.Parameter.KEYWORD_ONLY and p["keep_trace"].kind is inspect.Parameter.KEYWORD_ONLY
