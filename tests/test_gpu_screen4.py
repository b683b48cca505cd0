"""GPU: the 4-bit front pass (csrc/screen4.hip) changes no result.  Every case of tests/screen4_cases.py is built here with
the default path and, once for the whole module, in a child process started with BCX_DEV=1 BCX_SCREEN4=0 (the parent's
behaviour: the 8-bit tier alone); traces (selections, errors, status), weights and the final error are compared bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import screen4_cases as cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bc():
    import bayesiancoresets_amd as bc
    return bc


@pytest.fixture(scope="module")
def switched_off(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("screen4") / "off.npz")
    env = dict(os.environ, BCX_DEV="1", BCX_SCREEN4="0")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "screen4_cases.py"), path], check=True, env=env, cwd=ROOT,
                   timeout=600)
    return np.load(path)


_done = {}


def _default(bc, name):
    if name not in _done:
        assert os.environ.get("BCX_SCREEN4") is None
        _done[name] = cases.run_case(bc, name)
    return _done[name]


def _same(name, out, off):
    keys = sorted(k for k in off.files if k.startswith(name + "/"))
    assert keys and len(keys) == len(out)
    for k in keys:
        assert np.array_equal(out[k.split("/", 1)[1]], off[k]), k


# Redos the CPU model predicts for these rows: tools/screen4_model.py's row-to-wave map gives 65 536 rows 512 segments of 128
# rows, below the segment capacity whatever is listed -- 0 for every seed; the 8-bit capture behind the list may still halt an
# iteration now and then as it does without the front pass (tools/screen8_model.py), hence the + 1 the bound allows.
MODEL_REDOS = 0


@pytest.mark.parametrize("name", ("randn_fw_f32", "randn_fw_f16", "randn_omp_f32", "randn_omp_f16"))
def test_randn_builds_equal_the_switch_off_builds(bc, switched_off, name):
    out, st, _ = _default(bc, name)
    print(name, st)
    _same(name, out, switched_off)
    assert st["front4_iterations"] > 0 and st["front4_state"] == "in use"
    assert st["front4_redos"] <= MODEL_REDOS + 1
    assert 0 < st["front4_listed"] < st["front4_iterations"] * 65536
    assert st["front4_device_bytes"] >= 65536 * (64 + 8)


@pytest.mark.parametrize("name", ("ragged", "long"))
def test_ragged_and_long_rows(bc, switched_off, name):
    out, st, _ = _default(bc, name)
    print(name, st)
    _same(name, out, switched_off)
    assert st["front4_iterations"] > 0


def test_repeated_rows_drop_to_the_8_bit_tier(bc, switched_off):
    """20 000 rows that are 200 distinct rows, each 100 times: every copy of the leading row is listed and the capture behind
    the list cannot hold them, so 4-bit iterations halt, are redone, and the tier's own rule drops it -- to the 8-bit tier."""
    out, st, _ = _default(bc, "repeated")
    print(st)
    _same("repeated", out, switched_off)
    assert st["front4_redos"] >= 4 and st["front4_drops"] == 1
    assert st["front4_state"] == "dropped to 8-bit" and not st["front4_active"]


def test_reset_and_incremental_builds(bc, switched_off):
    out, st, _ = _default(bc, "reset")
    _same("reset", out, switched_off)
    assert st["front4_iterations"] > 0
    inc, st_inc, _ = _default(bc, "incremental")
    whole, _, _ = _default(bc, "incremental_whole")
    _same("incremental", inc, switched_off)
    _same("incremental_whole", whole, switched_off)
    # sentinel rows stay valid from one build() call to the next: only the first call starts with plain 8-bit iterations
    assert st_inc["front4_iterations"] >= 30 - 2 - 2 * st_inc["front4_redos"] - 2 * st_inc["storage_redos"]
    for k in ("sel", "err", "status"):
        assert np.array_equal(np.concatenate([inc[k + "0"], inc[k + "1"], inc[k + "2"]]), whole[k + "0"])
    assert np.array_equal(inc["w"], whole["w"])


def test_giga_keeps_the_8_bit_tier(bc, switched_off):
    out, st, _ = _default(bc, "giga")
    _same("giga", out, switched_off)
    assert st["screened"] > 0
    assert st["front4_iterations"] == 0 and st["front4_listed"] == 0 and not st["front4_active"]
    assert st["front4_state"] == "switched off or not applicable"


def test_full_list_segments_halt_redo_and_drop(bc, switched_off):
    """The list-overflow path itself: with the dev switch BCX_SCREEN4_SEGCAP=2 a segment holds two rows, the d = 4096 case
    lists nearly all of its four rows per wave, so the front pass stops storing at the capacity, the second stage writes the
    overflow partial, refine_kernel halts the iteration, it is redone, and the fourth redo drops the tier to 8 bits.  The
    trace is the switch-off trace."""
    os.environ["BCX_SCREEN4_SEGCAP"] = "2"
    try:
        out, st, _ = cases.run_case(bc, "long")
    finally:
        os.environ.pop("BCX_SCREEN4_SEGCAP", None)
    print(st)
    _same("long", out, switched_off)
    assert st["front4_overflows"] > 0
    assert st["front4_redos"] == 4 and st["front4_iterations"] == 4 and st["front4_drops"] == 1
    assert st["storage_redos"] >= 4
    assert st["front4_state"] == "dropped to 8-bit" and not st["front4_active"]
    assert st["front4_listed"] <= 2 * 512 * 4          # never more than the capacity of the 512 segments per iteration


# ---- two ranks sharing the GPU: row shards keep the 8-bit tier ----------------------------------------------------------------
def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, alg, itrs, N, d, front4, out_dir):
    os.environ["BCX_EXCHANGE"] = "mailbox"
    os.environ["BCX_DEV"] = "1"
    if front4:
        os.environ.pop("BCX_SCREEN4", None)
    else:
        os.environ["BCX_SCREEN4"] = "0"
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
    np.savez(os.path.join(out_dir, "f%d_r%d.npz" % (front4, rank)), sel=tr[0], err=tr[1], status=tr[2], idx=idx, w=w,
             screened=st["screened"], f4_iterations=st["front4_iterations"], f4_listed=st["front4_listed"],
             f4_active=st["front4_active"], f4_state=np.array(st["front4_state"]),
             exchange=np.array(s.exchange if world > 1 else "one"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("alg", (1, 2))
def test_two_rank_row_shards_keep_the_8_bit_tier(tmp_path, alg):
    import torch.multiprocessing as mp
    N, d, itrs = 12000, 48, 50
    for front4 in (0, 1):
        mp.spawn(_worker, args=(2, _free_port(), alg, itrs, N, d, front4, str(tmp_path)), nprocs=2, join=True)
    for rank in range(2):
        off, on = np.load(tmp_path / ("f0_r%d.npz" % rank)), np.load(tmp_path / ("f1_r%d.npz" % rank))
        for k in ("sel", "err", "status", "idx", "w"):
            assert np.array_equal(off[k], on[k]), (rank, k)
        assert int(on["f4_iterations"]) == 0 and int(on["f4_listed"]) == 0 and not bool(on["f4_active"])
        assert str(on["f4_state"]) == "switched off or not applicable"
        if str(on["exchange"]) == "mailbox":
            assert int(on["screened"]) > 0
