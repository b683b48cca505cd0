"""Host build of csrc/host_err.h, the one error message of the entry points that take no bcx_solver*, and the same channel
through the library.

What a failed HIP call makes of it cannot be driven on a GPU (no call is made to fail on purpose), so the grammar and the
lifetime are held here: tests/host/host_err_check.cpp is a program of its own that includes the header alone (no HIP header on
its include path), built with the address and undefined-behaviour sanitizers -- "<who>: <what>" and the code handed back, a
second failure replacing the first, the pointer valid and unchanged until the same thread's next failure, two threads each
reading their own text, an empty `what`.  The second test is the library's side of "per thread", through a refusal that needs
no device.
"""
import ctypes
import os
import shutil
import subprocess
import threading

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_host_err_under_sanitizers(tmp_path):
    exe = str(tmp_path / "host_err_check")
    # (the sanitizer runtimes are linked statically: the program does not depend on what else the process environment preloads)
    subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "host", "host_err_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "HOST_ERR OK", r.stdout
    assert r.stderr.strip() == "", r.stderr     # no sanitizer report, no leak


def test_a_failure_is_its_threads_own():
    """bcx_nuts_batch with P = 0 is refused before any device is asked for (tests/test_nuts_batch_host.py); the text it sets in one
    thread is not what another thread's bcx_project_last_error() reads."""
    from bayesiancoresets_amd import _native
    lib = _native.load()
    one = ctypes.c_void_p(8)                                      # (never dereferenced: the checks come first)
    D, J = 4, 3

    def refused(P):
        return lib.bcx_nuts_batch(None, 0, P, one, one, D, 8, 2, 2, J, 0.5, one, D + 3 * J + 2 * (2 ** J - 1), D, one, None, None, one,
                                  one, one, one, 0, None, None)

    # this thread's own text first: a refusal of another entry point
    assert lib.bcx_gram(None, None, 1, 1, 1, None, 1, None, 0) == _native.ERR_ARG
    mine = lib.bcx_project_last_error()
    assert mine == b"bcx_gram: bad arguments"
    seen = {}

    def other():
        seen["before"] = lib.bcx_project_last_error()             # a thread that has not failed reads the empty string
        seen["rc"] = refused(0)
        seen["after"] = lib.bcx_project_last_error()

    t = threading.Thread(target=other)
    t.start()
    t.join()
    assert seen["before"] == b""
    assert seen["rc"] == _native.ERR_ARG
    assert seen["after"].startswith(b"bcx_nuts_batch: bad arguments")
    assert lib.bcx_project_last_error() == mine                    # ... and did not reach this thread's
    # the other way round: a failure here does not change what a second thread set and reads again
    hold, go = threading.Event(), threading.Event()

    def holder():
        seen["held_rc"] = refused(0)
        seen["held"] = lib.bcx_project_last_error()
        hold.set()
        go.wait(60)
        seen["held_again"] = lib.bcx_project_last_error()

    t = threading.Thread(target=holder)
    t.start()
    assert hold.wait(60)
    assert lib.bcx_gram(None, None, 1, 1, 1, None, 1, None, 0) == _native.ERR_ARG
    go.set()
    t.join()
    assert seen["held_rc"] == _native.ERR_ARG
    assert seen["held"] == seen["held_again"] and seen["held"].startswith(b"bcx_nuts_batch: bad arguments")
    assert lib.bcx_project_last_error() == mine
