"""ctypes binding of libbcx.so (the C ABI in include/bcx.h) and the host-side driver of one
row shard.  There is NO CPU fallback: if the library is missing or no GPU is usable every
solver constructor raises."""
import ctypes
import os

import numpy as np

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# a source checkout builds the library in-tree (make -C bayesian-coresets_amd); an installed package carries it inside (setup.py)
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libbcx.so")
if not os.path.exists(LIB_PATH) and os.path.exists(os.path.join(_HERE, "_lib", "libbcx.so")):
    LIB_PATH = os.path.join(_HERE, "_lib", "libbcx.so")

# the header's enums and integer #defines under their names less the BCX_ prefix: ALG_*, F32 / F64 / F16, OK, ERR_*, IT_*,
# MAX_ROW_LENGTH, LOAD_CENTER_ROWS, SCREEN4_MAX_WAVES, ...; REC_HDR and CHUNK_ROWS are csrc/bcx_internal.h's, not the boundary's
globals().update((name[4:], value) for name, value in _abi.CONSTANTS.items())
REC_HDR = 4
CHUNK_ROWS = 1024
SYMBOLS = tuple(_abi.PROTOTYPES)      # every symbol include/bcx.h declares
Config, NutsProblem = _abi.STRUCTS["bcx_config"], _abi.STRUCTS["bcx_nuts_problem"]

_lib = None


def ensure_ipc_mode():
    """The ONE place that sets the IPC mode: multi-process GPU work on this platform (RCCL, the peer mailbox's
    hipIpcGetMemHandle) needs dmabuf IPC, i.e. HSA_ENABLE_IPC_MODE_LEGACY=0 in the environment BEFORE the HSA runtime
    initialises.  Called by load(), tests/conftest.py, bench.py and __graft_entry__.py.  A different value chosen by the
    user is respected (BCX_KEEP_IPC_MODE=1) and a setting that can no longer take effect is reported."""
    import logging
    cur = os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY")
    if cur == "0":
        return True
    if os.environ.get("BCX_KEEP_IPC_MODE"):
        return False
    initialised = False
    try:
        import sys
        t = sys.modules.get("torch")
        initialised = bool(t is not None and t.cuda.is_initialized())
    except Exception:
        pass
    os.environ["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    if initialised:
        logging.getLogger().warning("bayesiancoresets_amd: the HIP runtime was initialised before HSA_ENABLE_IPC_MODE_LEGACY=0 "
                                    "could be set (it was %r); peer mailboxes / RCCL between processes may fail -- export it "
                                    "before the first GPU call", cur)
    return not initialised


def load():
    """Load libbcx.so once; raise (never fall back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libbcx.so not found at %s -- build it with `make -C bayesian-coresets_amd` "
            "(or python -c 'import __graft_entry__ as g; g.build()'). There is no CPU fallback." % LIB_PATH)
    ensure_ipc_mode()
    # PyTorch-ROCm bundles its own HIP / HSA runtime; libbcx.so must bind to THAT copy (same SONAME, already loaded),
    # not pull the system one in next to it -- two HIP runtimes in one process fight over the device ("No HIP GPUs are
    # available" in whichever initialises second).  So torch is imported before the library is opened
    # (BCX_NO_TORCH_PRELOAD=1 skips this for embedders without torch).
    if not os.environ.get("BCX_NO_TORCH_PRELOAD"):
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in _abi.PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


class EngineError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("bcx error %d: %s" % (code, msg))
        self.code = code


def check(rc):
    """The status of an entry point that takes no handle: raise with bcx_project_last_error()'s text unless it is 0."""
    if rc != 0:
        raise EngineError(rc, load().bcx_project_last_error().decode())
    return rc


def stream_ptr(device):
    """The HIP stream torch is issuing work on for `device`, as the entry points take it."""
    import torch
    return int(torch.cuda.current_stream(device).cuda_stream)


def _current_stream_ptr():
    """Stream torch is currently issuing work on (so torch.distributed collectives and
    torch.cuda events order correctly with the engine's kernels); NULL stream without torch."""
    try:
        import torch
        if torch.cuda.is_available():
            return int(torch.cuda.current_stream().cuda_stream)
    except Exception:
        pass
    return 0


class Engine(object):
    """One row shard of the device solver.  Thin: every method is one or two ABI calls."""

    def __init__(self, alg, n_local, d, n_global=None, row_offset=0, rank=0, world_size=1, device=0,
                 store_dtype=F32, keep_exact_rows=True, refresh_every=0):
        self.lib = load()
        self.h = ctypes.c_void_p()
        self.cfg = Config(alg=alg, store_dtype=store_dtype, keep_exact_rows=int(bool(keep_exact_rows)),
                          device=device, d=d, world_size=world_size, rank=rank, refresh_every=refresh_every,
                          n_local=n_local, n_global=n_local if n_global is None else n_global,
                          row_offset=row_offset)
        rc = self.lib.bcx_create(ctypes.byref(self.cfg), ctypes.byref(self.h))
        if rc != OK:
            msg = self.lib.bcx_last_error(None).decode()
            self.h = ctypes.c_void_p()
            raise EngineError(rc, msg)
        self.d, self.n_local = d, n_local
        self.rec_len = d + REC_HDR
        self.use_current_stream()

    # -- plumbing ---------------------------------------------------------
    def _check(self, rc):
        if rc != OK:
            raise EngineError(rc, self.lib.bcx_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.lib.bcx_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def use_current_stream(self):
        self._check(self.lib.bcx_set_stream(self.h, ctypes.c_void_p(_current_stream_ptr())))

    # -- ingest -----------------------------------------------------------
    def load_host_rows(self, rows, row_begin=0, center=False):
        """rows: C-contiguous (n, >=d) float32/float64 ndarray view (row stride in elements = ld).
        center: the rows are raw log-likelihoods, subtract each row's mean during the pass (projector.py:21)."""
        assert rows.ndim == 2 and rows.strides[1] == rows.itemsize
        dt = F64 if rows.dtype == np.float64 else F32
        ld = rows.strides[0] // rows.itemsize
        self._check(self.lib.bcx_load_rows_flags(self.h, ctypes.c_void_p(rows.ctypes.data), 0, dt, row_begin,
                                                 rows.shape[0], ld, LOAD_CENTER_ROWS if center else 0))

    def load_device_rows(self, ptr, n, ld, is_f64, row_begin=0, center=False):
        self._check(self.lib.bcx_load_rows_flags(self.h, ctypes.c_void_p(ptr), 1, F64 if is_f64 else F32, row_begin, n, ld,
                                                 LOAD_CENTER_ROWS if center else 0))

    def chunk_sums_info(self):
        p, n, r = ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int64()
        self._check(self.lib.bcx_chunk_sums(self.h, ctypes.byref(p), ctypes.byref(n), ctypes.byref(r)))
        return p.value, n.value, r.value

    def export_chunk_sums(self, dst_ptr, cap_chunks):
        self._check(self.lib.bcx_export_chunk_sums(self.h, ctypes.c_void_p(dst_ptr), cap_chunks))

    def finalize(self, b=None, gathered_ptr=None, n_gathered=0):
        bp = None
        if b is not None:
            b = np.ascontiguousarray(b, dtype=np.float64)
            assert b.shape == (self.d,)
            bp = ctypes.c_void_p(b.ctypes.data)
        rc = self.lib.bcx_finalize(self.h, bp, ctypes.c_void_p(gathered_ptr) if gathered_ptr else None, n_gathered)
        return rc

    # -- tensor-level protocol used by sharded.ShardedSolver -----------------
    def tensor_device(self):
        import torch
        return torch.device("cuda", self.cfg.device)

    def load_rows_any(self, rows, row_begin=0, center=False):
        try:
            import torch
            if isinstance(rows, torch.Tensor):
                if rows.device.type == "cuda":
                    assert rows.stride(1) == 1
                    self.load_device_rows(rows.data_ptr(), rows.shape[0], rows.stride(0),
                                          rows.element_size() == 8, row_begin, center)
                    return
                rows = rows.numpy()
        except ImportError:
            pass
        self.load_host_rows(np.ascontiguousarray(rows), row_begin, center)

    def export_chunk_sums_tensor(self, t, cap_chunks):
        self.export_chunk_sums(t.data_ptr(), cap_chunks)

    def finalize_any(self, b, gathered, n_gathered):
        return self.finalize(b, gathered.data_ptr() if gathered is not None else None, n_gathered)

    def step_scan_tensor(self, send, exact=False):
        self.step_scan(send.data_ptr(), exact)

    def step_apply_tensor(self, recv):
        self.step_apply(recv.data_ptr())

    # -- build ------------------------------------------------------------
    def build_begin(self, itrs, tol):
        skip = ctypes.c_int32()
        self._check(self.lib.bcx_build_begin(self.h, itrs, tol, ctypes.byref(skip)))
        return bool(skip.value)

    def step_scan(self, send_ptr=None, exact=False):
        fn = self.lib.bcx_step_scan_exact if exact else self.lib.bcx_step_scan
        self._check(fn(self.h, ctypes.c_void_p(send_ptr) if send_ptr else None))

    def step_apply(self, recv_ptr=None):
        self._check(self.lib.bcx_step_apply(self.h, ctypes.c_void_p(recv_ptr) if recv_ptr else None))

    def enqueue(self, itrs):
        self._check(self.lib.bcx_build_enqueue(self.h, itrs))

    def enqueue_exact(self):
        self._check(self.lib.bcx_build_enqueue_exact(self.h))

    # -- peer mailbox (device-side record exchange between row shards) -------
    IPC_HANDLE_BYTES = 64

    def exchange_export(self):
        buf = ctypes.create_string_buffer(self.IPC_HANDLE_BYTES)
        self._check(self.lib.bcx_exchange_export(self.h, buf, self.IPC_HANDLE_BYTES))
        return buf.raw

    def exchange_attach(self, handles, timeout_s=0.0):
        blob = b"".join(handles)
        assert len(blob) == self.IPC_HANDLE_BYTES * len(handles)
        self._check(self.lib.bcx_exchange_attach(self.h, blob, self.IPC_HANDLE_BYTES, float(timeout_s)))

    def exchange_probe(self):
        res = ctypes.c_int32()
        self._check(self.lib.bcx_exchange_probe(self.h, ctypes.byref(res)))
        return res.value

    def exchange_set_timeout(self, timeout_s):
        self._check(self.lib.bcx_exchange_set_timeout(self.h, float(timeout_s)))

    def exchange_stats(self, reset=False):
        """Device-side timing of the record exchanges since the last reset (microseconds)."""
        n = ctypes.c_int64()
        v = [ctypes.c_double() for _ in range(4)]
        self._check(self.lib.bcx_exchange_stats(self.h, ctypes.byref(n), *[ctypes.byref(x) for x in v], int(bool(reset))))
        return {"exchanges": n.value, "wait_us_mean": v[0].value, "wait_us_max": v[1].value,
                "total_us_mean": v[2].value, "total_us_max": v[3].value}

    def exchange_disable(self):
        self._check(self.lib.bcx_exchange_disable(self.h))

    def poll(self):
        n, ne, lim = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int32()
        self._check(self.lib.bcx_build_poll(self.h, ctypes.byref(n), ctypes.byref(ne), ctypes.byref(lim)))
        return n.value, bool(ne.value), bool(lim.value)

    def trace(self, cap):
        sel = np.empty(cap, dtype=np.int64)
        err = np.empty(cap, dtype=np.float64)
        status = np.empty(cap, dtype=np.int32)
        n = ctypes.c_int64()
        self._check(self.lib.bcx_build_trace(self.h, sel.ctypes.data, err.ctypes.data, status.ctypes.data, cap,
                                             ctypes.byref(n)))
        return sel[:n.value], err[:n.value], status[:n.value]

    def run_build(self, itrs, tol):
        """Single-shard build(): enqueue everything, fall back to the exact scan for the rare
        iterations whose candidate window overflowed.  Returns (sel, err, status) of this call."""
        if self.build_begin(itrs, tol):
            return None
        self.enqueue(itrs)
        while True:
            done, need_exact, limit = self.poll()
            if not need_exact:
                break
            self.step_scan(exact=True)
            self.step_apply()
            done, need_exact, limit = self.poll()
            if need_exact:
                raise EngineError(ERR_STATE, "exact scan did not resolve the iteration")
            if done < itrs and not limit:
                self.enqueue(itrs - done)
        return self.trace(itrs)

    # -- read-out ---------------------------------------------------------
    def sparse_weights(self):
        k = ctypes.c_int64()
        self._check(self.lib.bcx_active_count(self.h, ctypes.byref(k)))
        idx = np.empty(k.value, dtype=np.int64)
        w = np.empty(k.value, dtype=np.float64)
        if k.value:
            self._check(self.lib.bcx_get_weights(self.h, idx.ctypes.data, w.ctypes.data, k.value, ctypes.byref(k)))
        return idx, w

    def error(self):
        e = ctypes.c_double()
        self._check(self.lib.bcx_error(self.h, ctypes.byref(e)))
        return e.value

    def optimize(self, tol):
        acc = ctypes.c_int32()
        self._check(self.lib.bcx_optimize(self.h, tol, ctypes.byref(acc)))
        return bool(acc.value)

    def reset(self):
        self._check(self.lib.bcx_reset(self.h))

    def set_check_monotone(self, on):
        self._check(self.lib.bcx_set_check_monotone(self.h, int(bool(on))))

    def reached_numeric_limit(self):
        v = ctypes.c_int32()
        self._check(self.lib.bcx_reached_numeric_limit(self.h, ctypes.byref(v)))
        return bool(v.value)

    def vector(self, which):
        out = np.empty(self.d, dtype=np.float64)
        self._check(self.lib.bcx_get_vector(self.h, which, out.ctypes.data))
        return out

    def norms(self, begin=0, count=None):
        count = self.n_local - begin if count is None else count
        out = np.empty(count, dtype=np.float64)
        if count:
            self._check(self.lib.bcx_get_norms(self.h, begin, count, out.ctypes.data))
        return out

    def stored_rows(self, begin=0, count=None):
        """The normalised rows as stored on the device ([count, d] in the storage type)."""
        count = self.n_local - begin if count is None else count
        ld = ctypes.c_int32()
        self._check(self.lib.bcx_get_stored_rows(self.h, begin, 0, None, ctypes.byref(ld)))
        dt = {F64: np.float64, F16: np.float16}.get(self.cfg.store_dtype, np.float32)
        out = np.empty((count, ld.value), dtype=dt)
        if count:
            self._check(self.lib.bcx_get_stored_rows(self.h, begin, count, out.ctypes.data, ctypes.byref(ld)))
        return out[:, :self.d]

    def argmax_correlation(self, query):
        q = np.ascontiguousarray(query, dtype=np.float64)
        assert q.shape == (self.d,)
        idx, score = ctypes.c_int64(), ctypes.c_double()
        self._check(self.lib.bcx_argmax_correlation(self.h, ctypes.c_void_p(q.ctypes.data), ctypes.byref(idx),
                                                    ctypes.byref(score)))
        return idx.value, score.value

    # -- measurement ------------------------------------------------------
    def time_scan(self, reps=20, exact=False):
        ms, by = ctypes.c_double(), ctypes.c_double()
        self._check(self.lib.bcx_time_scan(self.h, reps, int(exact), ctypes.byref(ms), ctypes.byref(by)))
        return ms.value, by.value

    def stats(self):
        a, b, c = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        self._check(self.lib.bcx_stats(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return {"exact_fallbacks": a.value, "candidates": b.value, "resolves": c.value}

    SCREEN_DROP = {0: "in use", 1: "dropped by the overflow rule until reset()", 2: "no device memory for the shadow",
                   3: "switched off or not applicable"}

    SCREEN4_STATE = {0: "in use", 1: "dropped to 8-bit", 2: "no device memory for the second shadow",
                     3: "switched off or not applicable"}

    def screen_stats(self):
        """The 8-bit screening tier: iterations screened, rows that survived it (re-scored from the stored rows), capture
        overflows and iterations redone with the storage-precision scan (not exact fallbacks; 8-bit and 4-bit iterations
        alike, the 4-bit ones alone are front4_redos), its state and footprint."""
        out = (ctypes.c_int64 * 8)()
        self._check(self.lib.bcx_screen_stats(self.h, out))
        o4 = (ctypes.c_int64 * 8)()
        self._check(self.lib.bcx_screen4_stats(self.h, o4))
        return {"active": bool(out[0]), "screened": out[1], "survivors": out[2], "overflows": out[3], "storage_redos": out[4],
                "state": self.SCREEN_DROP.get(int(out[5]), "?"), "device_bytes": out[6], "build_us": out[7],
                # the 4-bit front pass in front of the tier (csrc/screen4.hip)
                "front4_active": bool(o4[0]), "front4_iterations": o4[1], "front4_listed": o4[2], "front4_overflows": o4[3],
                "front4_redos": o4[4], "front4_state": self.SCREEN4_STATE.get(int(o4[5]), "?"), "front4_device_bytes": o4[6],
                "front4_drops": o4[7]}

    def screen_read(self, begin=0, count=None):
        """(codes uint8 [count, ld8], scales fp32 [count], bounds fp32 [count]) of the tier's shadow rows."""
        count = self.n_local - begin if count is None else count
        ld8 = (self.d + 15) // 16 * 16
        codes = np.empty((count, ld8), dtype=np.uint8)
        sc = np.empty(count, dtype=np.float32)
        bd = np.empty(count, dtype=np.float32)
        got = ctypes.c_int32()
        self._check(self.lib.bcx_screen_read(self.h, begin, count, codes.ctypes.data, sc.ctypes.data, bd.ctypes.data,
                                             ctypes.byref(got)))
        assert got.value == ld8
        return codes, sc, bd

    def screen4_read(self, begin=0, count=None):
        """(codes uint8 [count, ld4], scale4 fp32 [count], bound4 fp32 [count]) of the 4-bit front pass's shadow rows: two codes
        per byte as code + 8, the element with the even index in the low nibble, padding nibbles 8."""
        count = self.n_local - begin if count is None else count
        ld4 = (self.d + 31) // 32 * 16
        codes = np.empty((count, ld4), dtype=np.uint8)
        sc = np.empty(count, dtype=np.float32)
        bd = np.empty(count, dtype=np.float32)
        got = ctypes.c_int32()
        self._check(self.lib.bcx_screen4_read(self.h, begin, count, codes.ctypes.data, sc.ctypes.data, bd.ctypes.data,
                                              ctypes.byref(got)))
        assert got.value == ld4
        return codes, sc, bd

    SCREEN4_MAX_WAVES = SCREEN4_MAX_WAVES

    def screen4_probe(self, query, sentinels, list_stride=1024):
        """One launch of the front pass kernel alone against `query` ([d]) and 64 sentinel rows (-1: none).  Returns a dict:
        counts int32 [n_waves] (rows each wave wanted to list), list int32 [n_waves, list_stride] (the listed rows of a wave first,
        -1 behind them), and the partials its second stage wrote: U1, U2, U3, L float64 [n_waves], i1, i2 int32 [n_waves]."""
        q = np.ascontiguousarray(query, dtype=np.float64)
        sent = np.ascontiguousarray(sentinels, dtype=np.int32)
        assert q.shape == (self.d,) and sent.shape == (64,)
        cap = self.SCREEN4_MAX_WAVES
        nw = ctypes.c_int32()
        counts = np.zeros(cap, dtype=np.int32)
        lst = np.full((cap, list_stride), -1, dtype=np.int32)
        raw = np.zeros(cap * 40, dtype=np.uint8)
        self._check(self.lib.bcx_screen4_probe(self.h, q.ctypes.data, sent.ctypes.data, ctypes.byref(nw), counts.ctypes.data,
                                               lst.ctypes.data, list_stride, raw.ctypes.data))
        n = nw.value
        dbl = raw[:32 * n].view(np.float64).reshape(4, n)
        idx = raw[32 * n:40 * n].view(np.int32).reshape(2, n)
        return {"counts": counts[:n].copy(), "list": lst[:n].copy(), "U1": dbl[0].copy(), "U2": dbl[1].copy(), "U3": dbl[2].copy(),
                "L": dbl[3].copy(), "i1": idx[0].copy(), "i2": idx[1].copy()}

    def omp_stats(self):
        out = (ctypes.c_int64 * 4)()
        self._check(self.lib.bcx_omp_stats(self.h, out))
        return {"steps": out[0], "columns_left": out[1], "resolves": out[2], "extra_entered": out[3]}

    def profile(self, on):
        self._check(self.lib.bcx_profile_scan(self.h, int(on)))

    def profile_read(self):
        ms, n = ctypes.c_double(), ctypes.c_int64()
        self._check(self.lib.bcx_profile_read(self.h, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value


def device_row_sumsq(rows):
    """Sum of squares of every row of a device tensor (N x S fp64, unit column stride) as an ndarray: csrc/proj.hip
    row_sumsq_kernel (hilbert.py:19-22 drops the rows where it is zero)."""
    import torch
    lib = load()
    if rows.dtype != torch.float64 or rows.stride(1) != 1:
        rows = rows.to(torch.float64).contiguous()
    out = torch.empty(rows.shape[0], dtype=torch.float64, device=rows.device)
    with torch.cuda.device(rows.device):
        check(lib.bcx_row_sumsq(stream_ptr(rows.device), rows.data_ptr(), rows.shape[0], rows.shape[1], rows.stride(0), out.data_ptr()))
    return out.cpu().numpy()


def device_centred_copy(rows):
    """rows - rows.mean(axis=1)[:, None] for a device tensor (N x S fp64) as a NEW tensor: a device copy, then csrc/proj.hip
    center_kernel in place (projector.py:21)."""
    import torch
    lib = load()
    out = rows.to(torch.float64).contiguous().clone()
    with torch.cuda.device(out.device):
        check(lib.bcx_center_rows(stream_ptr(out.device), out.data_ptr(), out.shape[0], out.shape[1], out.stride(0)))
    return out
