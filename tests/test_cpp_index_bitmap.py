"""Index::SearchBitmap / SearchBatchBitmap of the compiled-language host mirror (include/longbow_gpu.hpp):
tests/cpp/index_bitmap_test.cpp, built with g++ as tests/test_cpp_host.py builds its program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKIP_RC = 77


def _build(tmp_path):
    from longbow_amd import build as lb_build  # noqa: F401  (the .so must exist; built by __graft_entry__.build())
    so_dir = os.path.join(ROOT, "longbow_amd")
    if not os.path.exists(os.path.join(so_dir, "liblongbow_gpu.so")):
        pytest.skip("liblongbow_gpu.so not built")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle")], check=True)
    exe = str(tmp_path / "index_bitmap_test")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "oracle"),
           os.path.join(ROOT, "tests", "cpp", "index_bitmap_test.cpp"), "-o", exe,
           "-L", so_dir, "-llongbow_gpu", "-L", os.path.join(ROOT, "oracle"), "-llongbow_oracle",
           "-L", "/opt/rocm/lib", f"-Wl,-rpath,{so_dir}", f"-Wl,-rpath,{os.path.join(ROOT, 'oracle')}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


def test_cpp_bitmap_wrapper_compiles_warning_free_and_validates_without_a_device(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert "ok   TestIndexBitmap_NullHandle" in r.stdout, r.stdout + r.stderr
    assert r.returncode in (0, SKIP_RC), r.stdout + r.stderr
    if r.returncode == SKIP_RC:
        assert "GPU support not enabled in this build" in r.stdout


@pytest.mark.gpu
def test_cpp_bitmap_search_matches_the_oracle_on_gpu(tmp_path):
    from tests.gpu_util import gpu_or_skip
    gpu_or_skip()
    exe = _build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr
    for name in ("TestIndexBitmap_NullHandle", "TestIndexBitmap_Validation", "TestIndexBitmap_MatchesOracle"):
        assert f"ok   {name}" in r.stdout, r.stdout
