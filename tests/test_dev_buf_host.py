"""Host build of csrc/dev_buf.h, the owner of the solver's device memory, over a fake allocator whose n-th allocation fails.

The paths this holds to account cannot be driven on a GPU (a shared card is not run out of memory on purpose): moves, reset,
alloc's free-before-allocate, the fills, grown plain and pitched, and a three-buffer capacity change that commits whole or not
at all under a failure at every one of its allocations.  tests/host/dev_buf_check.cpp is a program of its own, built with the
address and undefined-behaviour sanitizers; the leak checker has to be silent when it exits.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_dev_buf_under_sanitizers(tmp_path):
    exe = str(tmp_path / "dev_buf_check")
    # (the sanitizer runtimes are linked statically: the program does not depend on what else the process environment preloads)
    subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "host", "dev_buf_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "DEV_BUF OK" in r.stdout
    assert r.stderr.strip() == "", r.stderr     # no sanitizer report, no leak
