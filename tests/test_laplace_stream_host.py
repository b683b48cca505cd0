"""CPU-only: the ABI, the constructor keyword and the compiled resources of the streamed Laplace fit (csrc/laplace_stream.hip)."""
import ctypes
import inspect
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from bayesiancoresets_amd import _native
    return _native.load()


def test_abi_symbols_and_signatures(lib):
    from bayesiancoresets_amd import _native
    assert "bcx_laplace_sampler_stream" in _native.SYMBOLS and "bcx_laplace_stream_scratch_bytes" in _native.SYMBOLS
    vp, i32, i64, dbl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    fn = lib.bcx_laplace_sampler_stream
    # bcx_laplace_sampler's arguments, then the scratch buffer and its size
    assert list(fn.argtypes) == [vp, i32, i32, i32, vp, vp, i64, vp, i32, dbl, i32, vp, vp, i32, i32, vp, vp, vp, vp, i64]
    assert list(fn.argtypes[:18]) == list(lib.bcx_laplace_sampler.argtypes) and fn.restype is ctypes.c_int
    sb = lib.bcx_laplace_stream_scratch_bytes
    assert list(sb.argtypes) == [i32, i32] and sb.restype is ctypes.c_int64
    header = open(os.path.join(ROOT, "include", "bcx.h")).read()
    assert "int64_t bcx_laplace_stream_scratch_bytes(int32_t k, int32_t D);" in header
    assert "int bcx_laplace_sampler_stream(void* stream, int32_t family, int32_t k, int32_t D," in header


def test_scratch_bytes(lib):
    sb = lib.bcx_laplace_stream_scratch_bytes
    assert sb(100, 0) == -1 and sb(100, 33) == -1 and sb(-1, 4) == -1
    for D in (1, 10, 32):
        sizes = [sb(k, D) for k in (0, 1, 127, 128, 129, 1000, 4096, 32768, 1000000, (1 << 31) - 1)]
        assert sizes[0] > 0 and all(b >= a for a, b in zip(sizes, sizes[1:])), (D, sizes)
        assert sizes[-1] <= 4 << 20                  # (bounded: a record per workgroup, not per tile)
    assert sb(1000, 32) > sb(1000, 10) > sb(1000, 1)


def test_bad_arguments_are_refused_before_any_launch(lib):
    from bayesiancoresets_amd import _native
    one = ctypes.c_void_p(8)                         # (never dereferenced: the checks come first)
    args = lambda **kw: [kw.get(n, d) for n, d in (("stream", None), ("family", 0), ("k", 0), ("D", 4), ("w", None), ("pts", None), ("ldp", 4),
                                                   ("mu", one), ("warm", 0), ("tol", 1e-10), ("max_iter", 10), ("R", one), ("Rbar", one),
                                                   ("S", 4), ("ld", 4), ("theta", one), ("tbar", one), ("status", one), ("work", one),
                                                   ("work_bytes", 0))]
    for kw in (dict(D=0), dict(D=33), dict(family=2), dict(S=0), dict(ld=3), dict(max_iter=0), dict(tol=0.0), dict(work=None),
               dict(work_bytes=0), dict(k=5, work_bytes=1 << 20), dict(k=5, w=one, pts=one, ldp=3, work_bytes=1 << 20),
               dict(k=5, family=1, w=one, pts=one, ldp=4, work_bytes=1 << 20)):
        assert lib.bcx_laplace_sampler_stream(*args(**kw)) == _native.ERR_ARG, kw
        assert b"bcx_laplace_sampler_stream" in lib.bcx_project_last_error()


def test_constructor_keywords():
    import bayesiancoresets_amd as bc
    p = inspect.signature(bc.LaplacePosteriorSampler.__init__).parameters
    assert p["stream"].kind is inspect.Parameter.KEYWORD_ONLY and p["stream"].default is False
    p = inspect.signature(bc.DeviceHMC.__init__).parameters
    assert p["device_frame"].kind is inspect.Parameter.KEYWORD_ONLY and p["device_frame"].default is False


def test_no_spills_no_scratch():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"),
                          os.path.join(ROOT, "bayesian-coresets_amd", "csrc", "laplace_stream.hip")], capture_output=True, text=True,
                         timeout=1200, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    last = out.stdout.strip().splitlines()[-1]
    assert last == "kernels with spills or scratch: 0", out.stdout[-3000:]
    assert "laplace_stream_kernel" in out.stdout
