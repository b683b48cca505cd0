"""CPU-only: the ADAM entry of BatchPSVI's device-resident loop (csrc/psvi.hip psvi_adam_kernel, bcx_psvi_adam_step) is declared,
exported and bound, and the kernel keeps every register in registers for gfx950."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_adam_entry_is_declared_exported_and_bound():
    from bayesiancoresets_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bcx.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+bcx_psvi_adam_step\s*\(", text)
    assert "bcx_psvi_adam_step" in _native.SYMBOLS
    lib = _native.load()
    assert hasattr(lib, "bcx_psvi_adam_step")
    assert len(lib.bcx_psvi_adam_step.argtypes) == 19


def test_header_cites_the_reference_lines():
    text = open(os.path.join(ROOT, "include", "bcx.h")).read()
    at = text.index("bcx_psvi_adam_step")
    block = text[text.rindex("/*", 0, at):at]
    assert "util/opt.py:15-23" in block and "bpsvi.py:57-60" in block


def test_adam_kernel_no_spills_no_scratch():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"),
                          os.path.join(ROOT, "bayesian-coresets_amd", "csrc", "psvi.hip")], capture_output=True, text=True,
                         timeout=1200, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("psvi_adam_kernel")]
    assert len(line) == 1, out.stdout[-3000:]
    assert re.search(r"spill\s+0\s+scratch\s+0 B", line[0]), line[0]
    assert out.stdout.strip().splitlines()[-1] == "kernels with spills or scratch: 0", out.stdout[-3000:]


def test_moving_plans_are_offered_by_the_three_samplers_only():
    """``BatchPSVICoreset`` looks the plan up with getattr: the package's samplers have it, a callback has not."""
    import bayesiancoresets_amd as bc
    for cls in (bc.LinregPosteriorSampler, bc.GaussianPosteriorSampler, bc.LaplacePosteriorSampler):
        assert callable(getattr(cls, "enqueue_plan_moving", None))
        assert callable(getattr(cls, "enqueue_plan", None))
    assert bc.BatchPSVICoreset.ENQUEUE is True
    assert getattr(lambda n, w, p: None, "enqueue_plan_moving", None) is None
