"""CPU-only: bench.py's launcher contract (no GPU needed for these paths): `--gpus N` never degrades to fewer ranks."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _clean_env(**extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT",
                                                           "BENCH_SHARE_GPU")}
    env.update(extra)
    return env


def test_more_ranks_than_devices_is_refused_without_a_line():
    import torch
    have = torch.cuda.device_count() if torch.cuda.is_available() else 0
    out = subprocess.run([sys.executable, BENCH, "--gpus", str(have + 3), "--steps", "2"], capture_output=True, text=True,
                         timeout=300, env=_clean_env(), cwd=ROOT)
    assert out.returncode == 2 and "refusing" in out.stderr
    assert not [l for l in out.stdout.splitlines() if l.startswith("{")]


def test_world_size_that_contradicts_gpus_is_an_error():
    out = subprocess.run([sys.executable, BENCH, "--gpus", "4", "--steps", "2"], capture_output=True, text=True, timeout=300,
                         env=_clean_env(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"), cwd=ROOT)
    assert out.returncode != 0 and "does not match WORLD_SIZE" in out.stderr
    assert not [l for l in out.stdout.splitlines() if l.startswith("{")]


def test_zero_gpus_is_an_error():
    out = subprocess.run([sys.executable, BENCH, "--gpus", "0"], capture_output=True, text=True, timeout=300, env=_clean_env(), cwd=ROOT)
    assert out.returncode != 0


def test_plain_run_leaves_every_leg_beside_the_headline_to_full(monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    legs = ("no_cpu_baseline", "no_exact_mode", "no_f16_leg", "no_side_legs", "no_one_rank_leg")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert all(getattr(a, k) for k in legs) and (a.steps, a.warmup, a.dump_outputs) == (7, 2, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-f16-leg", "--dump-outputs", "out"])
    a = bench.parse()
    assert not any(getattr(a, k) for k in legs if k != "no_f16_leg") and a.no_f16_leg and a.dump_outputs == "out"


def test_dump_outputs_writes_float64_within_the_size_cap(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import numpy as np
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 2 * 800)
    big = np.arange(300, dtype=np.int64)
    bench.dump_outputs(str(tmp_path / "d"), {"small": np.arange(5, dtype=np.int32), "big": big})
    small, cut = np.load(tmp_path / "d" / "small.npy"), np.load(tmp_path / "d" / "big.npy")
    assert small.dtype == cut.dtype == np.float64 and np.array_equal(small, np.arange(5))
    assert cut.nbytes <= 800 and len(cut) == 100 and np.all(np.diff(cut) > 0)       # a sample of the rows, in order
    bench.dump_outputs(str(tmp_path / "e"), {"small": np.zeros(5), "big": big})
    assert np.array_equal(np.load(tmp_path / "e" / "big.npy"), cut)                  # the same sample every run
