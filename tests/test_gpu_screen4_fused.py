"""GPU: the front pass that computes its own threshold (csrc/screen4.hip: front4_head, from the sentinel rows the previous
iteration's refine_kernel left) changes no result.  Every case of tests/screen4_fused_cases.py is built here with the default
path and, once for the whole module, in a child process started with BCX_DEV=1 BCX_SCREEN4=0 (the 8-bit tier alone); traces
(selections, errors, status), weights and the final error are compared bit for bit.

Every case also asserts that the front pass really ran: front4_iterations >= iterations - 2 per fresh start - 2 per redone
iteration (the warm-up rule of api.hip), and front4_redos <= 1.  tools/screen4_model.py's redos come from full list segments
alone; with the default capacity of 1024 no segment of these shapes can fill (the fullest holds rows / segments < 1024 rows),
so it predicts 0 for every seed, and the one redo allowed is the 8-bit capture behind the list halting an iteration as it does
without the front pass (tests/test_gpu_screen4.py).  The case with a capacity of 3 has rows and a seed for which the model,
run with that capacity, predicts exactly one full segment in one iteration."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import screen4_fused_cases as cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

@pytest.fixture(scope="module")
def bc():
    import bayesiancoresets_amd as bc
    return bc


@pytest.fixture(scope="module")
def switched_off(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("screen4f") / "off.npz")
    env = dict(os.environ, BCX_DEV="1", BCX_SCREEN4="0")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "screen4_fused_cases.py"), path], check=True, env=env, cwd=ROOT,
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


def _ran(name, st):
    calls = cases.CASES[name][4]
    iterations = sum(c for c in calls if c != "reset")
    starts = 1 + sum(1 for c in calls if c == "reset")
    print(name, st)
    assert st["front4_iterations"] >= iterations - 2 * starts - 2 * (st["front4_redos"] + st["storage_redos"])
    assert st["front4_redos"] <= 1


@pytest.mark.parametrize("d", sorted(cases.GEOMETRY))
def test_every_geometry_pair_equals_the_switch_off_build(bc, switched_off, d):
    name = "geom_d%d" % d
    assert cases.GEOMETRY[d] % cases.rows_per_trip(d) != 0
    out, st = _default(bc, name)
    _ran(name, st)
    _same(name, out, switched_off)
    assert st["front4_state"] == "in use" and 0 < st["front4_listed"]


def test_waves_that_list_nothing_and_single_rows(bc, switched_off):
    """9 001 rows of d = 512 in 284 list segments of about 32 rows: the model lists about a fifth of the rows at this size, so
    in every iteration a few waves list nothing at all and hand the second stage an empty segment, others a single row."""
    out, st = _default(bc, "remainder")
    _ran("remainder", st)
    _same("remainder", out, switched_off)
    assert 0 < st["front4_listed"] < 9001 * st["front4_iterations"]


def test_one_row_past_a_trip(bc, switched_off):
    n, d = cases.CASES["ragged_one"][2:4]
    assert n % cases.rows_per_trip(d) == 1
    out, st = _default(bc, "ragged_one")
    _ran("ragged_one", st)
    _same("ragged_one", out, switched_off)
    assert 0 < st["front4_listed"] <= n * st["front4_iterations"]      # the clamped copies of row n - 1 are not listed


@pytest.mark.parametrize("name", ("tiny_fw", "tiny_omp"))
def test_fewer_rows_than_a_trip_and_than_sentinels(bc, switched_off, name):
    n, d = cases.CASES[name][2:4]
    assert n < 64 and n < cases.rows_per_trip(d) and 2 * cases.segments(n, d) < 64      # candidates < sentinels: -1 entries
    out, st = _default(bc, name)
    _ran(name, st)
    _same(name, out, switched_off)
    assert 0 < st["front4_listed"] <= n * st["front4_iterations"]


def test_segment_capacity_of_three(bc, switched_off):
    """BCX_SCREEN4_SEGCAP=3 on d = 4096, N = 2048 (four rows per wave, rank-100 rows): one wave lists all four of its rows in
    one iteration, so the capacity is hit between two 8-bit slot groups; that iteration halts and is redone, the others stay
    on the 4-bit path, and the trace is the switch-off trace."""
    os.environ["BCX_SCREEN4_SEGCAP"] = "3"
    try:
        out, st = cases.run_case(bc, "segcap3")
    finally:
        os.environ.pop("BCX_SCREEN4_SEGCAP", None)
    _ran("segcap3", st)
    _same("segcap3", out, switched_off)
    assert st["front4_overflows"] > 0 and st["front4_state"] == "in use"
    assert st["front4_listed"] <= 3 * cases.segments(2048, 4096) * st["front4_iterations"]


def test_consecutive_builds_and_reset(bc, switched_off):
    """Three calls of 8 iterations against one of 24: the first 4-bit iteration of a later call uses the sentinels the previous
    call's last refine left, so only the first call warms up.  Then a reset and a rebuild, which warms up again."""
    inc, st_inc = _default(bc, "calls_3x8")
    whole, st_whole = _default(bc, "calls_24")
    _ran("calls_3x8", st_inc)
    _ran("calls_24", st_whole)
    _same("calls_3x8", inc, switched_off)
    _same("calls_24", whole, switched_off)
    for k in ("sel", "err", "status"):
        assert np.array_equal(np.concatenate([inc[k + "0"], inc[k + "1"], inc[k + "2"]]), whole[k + "0"])
    assert np.array_equal(inc["w"], whole["w"])
    assert st_inc["front4_iterations"] == st_whole["front4_iterations"] and st_inc["front4_listed"] == st_whole["front4_listed"]
    out, st = _default(bc, "reset_rebuild")
    _ran("reset_rebuild", st)
    _same("reset_rebuild", out, switched_off)
    assert np.array_equal(out["sel0"], out["sel2"]) and np.array_equal(out["err0"], out["err2"])
