"""GPU: the 8-bit screening tier (csrc/screen8.hip) changes no result.  Every case runs the same build with the tier on (the
default) and off (dev switch BCX_SCREEN8=0, read when a solver is created) and compares traces and weights bit for bit."""
import os
import socket
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bc():
    import bayesiancoresets_amd as bc
    return bc


@pytest.fixture(autouse=True)
def _restore_switch():
    old = os.environ.get("BCX_SCREEN8")
    yield
    if old is None:
        os.environ.pop("BCX_SCREEN8", None)
    else:
        os.environ["BCX_SCREEN8"] = old


def _cls(bc, alg):
    return {"giga": bc.snnls.GIGA, "fw": bc.snnls.FrankWolfe, "omp": bc.snnls.OrthoPursuit}[alg]


def _make(bc, X, alg, tier, **kw):
    os.environ["BCX_SCREEN8"] = "1" if tier else "0"
    s = _cls(bc, alg)(X.T, X.sum(axis=0), **kw)
    assert s._eng.screen_stats()["active"] == bool(tier)
    return s


def _same(a, b):
    for x, y in zip(a.last_trace, b.last_trace):
        assert np.array_equal(x, y)
    assert np.array_equal(a.weights(), b.weights())
    assert a.error() == b.error()


FIXTURES = {"F9": (7, 3000, 64, "F9_input_sha256", 60), "F2": (1, 10000, 100, "F2_input_sha256", 100),
            "F3": (1, 10000, 100, "F3_t1_input_sha256", 300)}


@pytest.mark.parametrize("dtype", ("float32", "float16"))
@pytest.mark.parametrize("alg", ("giga", "fw", "omp"))
@pytest.mark.parametrize("fx", ("F9", "F2", "F3"))
def test_tier_on_equals_tier_off(bc, normal_inputs, fx, alg, dtype):
    seed, N, d, key, itrs = FIXTURES[fx]
    X = normal_inputs(seed, N, d, key)
    on, off = _make(bc, X, alg, True, dtype=dtype), _make(bc, X, alg, False, dtype=dtype)
    on.build(itrs)
    off.build(itrs)
    _same(on, off)
    st, so = on._eng.screen_stats(), on._eng.stats()
    print(fx, alg, dtype, st, so, off._eng.stats())
    assert st["screened"] > 0 and off._eng.screen_stats()["screened"] == 0
    assert so["exact_fallbacks"] == off._eng.stats()["exact_fallbacks"]


@pytest.mark.parametrize("alg", ("giga", "fw", "omp"))
def test_all_rows_tie(bc, alg):
    """X = eye(N): every score ties on every iteration; the tier overflows, the storage-precision redo overflows, the exact
    scan decides -- as without the tier -- and the overflow rule drops the tier."""
    X = np.eye(100)
    on, off = _make(bc, X, alg, True), _make(bc, X, alg, False)
    on.build(40)
    off.build(40)
    _same(on, off)
    assert list(on.last_trace[0][:12]) == list(range(12))
    assert on._eng.stats()["exact_fallbacks"] == off._eng.stats()["exact_fallbacks"]


@pytest.mark.parametrize("alg", ("giga", "fw", "omp"))
def test_incremental_build_and_reset(bc, normal_inputs, alg):
    X = normal_inputs(7, 3000, 64, "F9_input_sha256")
    on, off = _make(bc, X, alg, True), _make(bc, X, alg, False)
    for n in (1, 7, 20, 3):
        on.build(n)
        off.build(n)
        _same(on, off)
    on.reset()
    off.reset()
    on.build(25)
    off.build(25)
    _same(on, off)
    one = _make(bc, X, alg, True)
    one.build(25)
    _same(on, one)


def test_shadow_matches_the_numpy_restatement(bc):
    """Codes and scales equal the restatement of tools/screen8_model.py applied to the stored rows; every bound covers the
    true residual norm."""
    from tools.screen8_model import dequantise, quantise
    rs = np.random.RandomState(11)
    X = rs.randn(5000, 100)
    X[:50] *= 10.0 ** rs.uniform(-8, 8, size=(50, 100))       # rows with elements over many decades
    X[50] = 0.0
    X[50, 3] = 2.5                                             # one-hot
    X[51] = 1.0                                                # constant
    for dtype in ("float32", "float16"):
        s = _make(bc, X, "fw", True, dtype=dtype)
        codes, sc, bd = s._eng.screen_read()
        # the rows as the device stores them (its norms are summed in another order than NumPy's: a host-side
        # A / |A| differs from them in the last bit now and then), held to the host's normalisation
        stored = s._eng.stored_rows().astype(np.float32)
        An = X / np.linalg.norm(X, axis=1)[:, None]
        np.testing.assert_allclose(stored, An, rtol=1e-3 if dtype == "float16" else 1e-6, atol=1e-7 if dtype == "float16" else 1e-30)
        c2, s2, b2 = quantise(stored)
        assert np.array_equal(codes, c2) and np.array_equal(sc, s2)
        res = np.sqrt(((stored.astype(np.float64) - dequantise(c2, s2, 100)) ** 2).sum(axis=1))
        assert (bd.astype(np.float64) >= res).all()
        assert (bd.astype(np.float64) <= res * (1 + 4e-6) + 1e-44).all()
        assert s._eng.screen_stats()["device_bytes"] >= 5000 * (112 + 8)


def test_capture_overflow_is_bounded_and_drops_the_tier(bc):
    """Every row equals one of 50 vectors plus noise far below the 8-bit step: the 8-bit screen cannot separate the ~400 rows
    of the leading cluster, its capture overflows, each such iteration is redone with the storage-precision scan (never the
    exact scan), and after the 4th redo within 256 screened iterations the tier is dropped until reset()."""
    rs = np.random.RandomState(2)
    N, d = 20000, 128
    bases = rs.randn(50, d)
    X = 3.0 * bases[np.arange(N) % 50] + 5e-3 * rs.randn(N, d)     # 8-bit step of these rows: ~0.06
    on, off = _make(bc, X, "fw", True), _make(bc, X, "fw", False)
    on.build(30)
    off.build(30)
    _same(on, off)
    # the fp64 reference's row for the first pick
    An = X / np.linalg.norm(X, axis=1)[:, None]
    assert int(on.last_trace[0][0]) == int(np.argmax(An @ X.sum(axis=0)))
    st = on._eng.screen_stats()
    print(st, on._eng.stats(), off._eng.stats())
    assert st["overflows"] > 0 and st["storage_redos"] >= 4
    assert on._eng.stats()["exact_fallbacks"] == 0
    assert st["state"].startswith("dropped") and not st["active"]
    assert st["screened"] <= 8                     # bounded cost: nothing was screened after the drop
    on.reset()
    assert on._eng.screen_stats()["active"]        # the drop lasts until reset()


def test_c2_shape_giga_past_d_keeps_the_fp64_stage_narrow(bc):
    """GIGA at the c2 row length to M > d: rows re-scored in fp64 stay within 2 per resolve pass, as without the tier."""
    X = np.random.RandomState(1).randn(200000, 256)
    on, off = _make(bc, X, "giga", True), _make(bc, X, "giga", False)
    on.build(400)
    off.build(400)
    _same(on, off)
    st = on._eng.stats()
    print(on._eng.screen_stats(), st)
    assert st["candidates"] <= 2 * st["resolves"]


# ---- 1 / 2 / 4 ranks sharing the GPU ------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, alg, itrs, N, d, tier, out_dir):
    os.environ["BCX_EXCHANGE"] = "mailbox"
    os.environ["BCX_DEV"] = "1"
    os.environ["BCX_SCREEN8"] = "1" if tier else "0"
    for p in (ROOT, os.path.join(ROOT, "bayesian-coresets_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from bayesiancoresets_amd.sharded import ShardedSolver
    X = np.random.RandomState(21).randn(N, d)
    s = ShardedSolver(alg, N, d, device=0)
    s.load_local(torch.from_numpy(X[s.row_begin:s.row_end]).cuda())
    torch.cuda.synchronize()
    assert s.finalize(None) == 0
    tr = s.build(itrs)
    idx, w = s.sparse_weights()
    st = s.engine.screen_stats()
    np.savez(os.path.join(out_dir, "t%d_w%d_r%d.npz" % (tier, world, rank)), sel=tr[0], err=tr[1], status=tr[2], idx=idx, w=w,
             screened=st["screened"], exchange=np.array(s.exchange if world > 1 else "one"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("alg", (0, 1, 2))
def test_one_two_four_ranks(tmp_path, alg):
    import torch.multiprocessing as mp
    N, d, itrs = 12000, 48, 50
    mp.spawn(_worker, args=(1, _free_port(), alg, itrs, N, d, 0, str(tmp_path)), nprocs=1, join=True)
    ref = np.load(tmp_path / "t0_w1_r0.npz")
    for world in (1, 2, 4):
        mp.spawn(_worker, args=(world, _free_port(), alg, itrs, N, d, 1, str(tmp_path)), nprocs=world, join=True)
        for rank in range(world):
            r = np.load(tmp_path / ("t1_w%d_r%d.npz" % (world, rank)))
            for k in ("sel", "err", "status", "idx", "w"):
                assert np.array_equal(ref[k], r[k]), (world, rank, k)
            if world == 1 or str(r["exchange"]) == "mailbox":
                assert int(r["screened"]) > 0, (world, rank)
