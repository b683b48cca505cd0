"""CPU-only (hipcc cross-compiles without a GPU): the streamed NUTS kernel of csrc/nuts_stream.hip may not spill registers or use
scratch memory -- tools/kernel_resources.py, the bar tests/test_laplace_stream_host.py applies to csrc/laplace_stream.hip."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_no_spills_no_scratch():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"),
                          os.path.join(ROOT, "bayesian-coresets_amd", "csrc", "nuts_stream.hip")], capture_output=True, text=True, timeout=1200,
                         cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    last = out.stdout.strip().splitlines()[-1]
    assert last == "kernels with spills or scratch: 0", out.stdout[-3000:]
    assert "nuts_stream_kernel" in out.stdout
