"""CPU-only (hipcc cross-compiles without a GPU): the Coreset MCMC kernels of csrc/hmc.hip (cmc_advance_kernel, the chains'
launch, and cmc_centre_kernel) are compiled, and no kernel of the file spills registers or uses scratch memory --
tools/kernel_resources.py."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cmc_kernels_no_spills_no_scratch():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"),
                          os.path.join(ROOT, "bayesian-coresets_amd", "csrc", "hmc.hip")], capture_output=True, text=True, timeout=1200, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    assert lines[-1] == "kernels with spills or scratch: 0", out.stdout[-3000:]
    for name in ("cmc_advance_kernel", "cmc_centre_kernel"):
        mine = [ln for ln in lines if name in ln]
        assert len(mine) == 1, (name, out.stdout[-3000:])
        assert re.search(r"spill\s+0 scratch\s+0 B", mine[0]), mine[0]
