"""guard() and guard_device() (longbow_amd/csrc/lb_handle.h: the shell every C-ABI entry point runs its body in) as a stand-alone
host program, tests/cpp/handle_guard.cpp: a body that returns a status, and bodies that throw HipErr (out of memory, invalid
value), std::bad_alloc, CtxErr (cancelled, deadline) and an int, each on a bare HandleCore and without a handle, with a null
stream.  The status and the last_error text of each are asserted in the program; no device is needed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_guard_turns_every_exception_into_a_status_and_a_message(tmp_path):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not available")
    exe = tmp_path / "handle_guard"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function", "-x", "hip",
                        os.path.join(ROOT, "tests", "cpp", "handle_guard.cpp"), "-I" + os.path.join(ROOT, "longbow_amd", "csrc"),
                        "-lpthread", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.stdout + r.stderr)[-2000:]
