"""CPU-only (hipcc cross-compiles without a GPU): the pair-statistic kernels of csrc/pairstat.hip (both kinds of
pair_tiles_kernel and pair_total_kernel) are compiled, and no kernel of the file spills registers or uses scratch memory --
tools/kernel_resources.py."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pairstat_kernels_no_spills_no_scratch():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"),
                          os.path.join(ROOT, "bayesian-coresets_amd", "csrc", "pairstat.hip")], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    assert lines[-1] == "kernels with spills or scratch: 0", out.stdout[-3000:]
    assert len(lines) == 4, out.stdout[-3000:]                                  # (three kernels and the summary: none unnamed)
    for name in ("pair_tiles_kernel<0>", "pair_tiles_kernel<1>", "pair_total_kernel"):
        mine = [ln for ln in lines if name in ln]
        assert len(mine) == 1, (name, out.stdout[-3000:])
        assert re.search(r"spill\s+0 scratch\s+0 B", mine[0]), mine[0]
