"""CPU-only: the four NUTS kernels of csrc/nuts.hip -- nuts_coreset_kernel and nuts_batch_kernel, each plain and adapting (DESIGN.md
4.18) -- compile for gfx950 without a spilled register and without scratch, by tools/kernel_resources.py."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_no_spill_no_scratch_in_any_instantiation():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"),
                          os.path.join(ROOT, "bayesian-coresets_amd", "csrc", "nuts.hip")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    print(out.stdout)
    assert lines[-1] == "kernels with spills or scratch: 0"
    for kernel in ("nuts_coreset_kernel", "nuts_batch_kernel"):
        rows = [ln for ln in lines if kernel + "<" in ln]
        assert len(rows) == 2, (kernel, lines)                                  # (plain and adapting)
        for ln in rows:
            assert re.search(r"spill\s+0 scratch\s+0 B", ln), ln
