"""The six entry points that take a row bitmap with the search call on the flat index (include/longbow_gpu.h, lb_gpu_index_*:
"call bitmap") on a box without a GPU: declared, exported from both builds of the library, bound with their prototypes -- the plain
entry points' argument lists with (bitmap, nbits) behind k in all six -- and refusing a NULL handle before a device is touched,
with nothing written.  The checks behind a live handle are in tests/test_gpu_index_bitmap.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
_vp, _i, _i64 = C.c_void_p, C.c_int, C.c_int64
NEW_ARGS = [_vp, _i64]  # bitmap, nbits
AT = 4                  # behind (h, nq, queries, k)
_Q = {"": r"const float \*", "_f16": r"const uint16_t \*", "_i8": r"const int8_t \*"}
PLAIN = {}              # the entry point each one extends
for _t in _Q:
    PLAIN[f"lb_gpu_index_search{_t}_bitmap_ctx"] = f"lb_gpu_index_search{_t}_ctx"
    PLAIN[f"lb_gpu_index_search{_t}_bitmap_device_ctx"] = f"lb_gpu_index_search{_t}_device_ctx"
DECLARATIONS = [
    rf"int\s+lb_gpu_index_search{t}_bitmap_ctx\s*\(\s*lb_gpu_index \*h,\s*int64_t nq,\s*{q}queries,\s*int k,\s*"
    rf"const uint8_t \*bitmap,\s*int64_t nbits,\s*float \*dist,\s*int64_t \*labels,\s*const lb_cancel \*ctx\)"
    for t, q in _Q.items()
] + [
    rf"int\s+lb_gpu_index_search{t}_bitmap_device_ctx\s*\(\s*lb_gpu_index \*h,\s*int64_t nq,\s*{q}d_queries,\s*int k,\s*"
    rf"const uint8_t \*d_bitmap,\s*int64_t nbits,\s*float \*d_dist,\s*int64_t \*d_labels,\s*void \*stream,\s*const lb_cancel \*ctx\)"
    for t, q in _Q.items()
]


@pytest.fixture(scope="module")
def lib():
    from longbow_amd import _lib, build
    build.build()
    return _lib.load()


def _exports(path):
    return subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout


def test_symbols_declared_exported_and_bound(lib):
    from longbow_amd import _lib
    assert len(PLAIN) == 6
    header = open(os.path.join(ROOT, "include", "longbow_gpu.h")).read()
    for pat in DECLARATIONS:
        assert re.search(pat, header), pat
    bound = {s[0]: (s[1], list(s[2])) for s in _lib.SIGNATURES}
    out = _exports(_lib.SO_PATH)
    for name, plain in PLAIN.items():
        assert re.search(rf"\b{name}\b", out), f"{name} not exported"
        assert name in bound, f"{name} missing from _lib.SIGNATURES"
        res, args = bound[name]
        pres, pargs = bound[plain]
        assert res is pres is _i
        assert args == pargs[:AT] + NEW_ARGS + pargs[AT:], (name, args)   # the same place in all six
        fn = getattr(lib, name)
        assert fn.restype is _i and list(fn.argtypes) == args


def test_the_diagnostic_build_exports_them_too():
    from longbow_amd import _lib, build
    build.build(diag=True)
    out = _exports(_lib.DIAG_SO_PATH)
    for name in PLAIN:
        assert re.search(rf"\b{name}\b", out), f"{name} not exported by the diagnostic build"


def test_the_new_kernel_file_is_built_and_the_header_states_the_semantics():
    from longbow_amd import build
    assert "kernels_index_call.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "kernels_index_call.hip"))
    header = open(os.path.join(ROOT, "include", "longbow_gpu.h")).read()
    block = header[header.index("---- call bitmap: a row filter given with the search call"):header.index("int lb_gpu_index_search_bitmap_ctx")]
    for word in ("bit layout", "reading", "one bitmap", "result", "handle state", "arguments", "combining", "cancellation", "Not here"):
        assert word in block, word


@pytest.mark.parametrize("nq", [5, 0, -1])
def test_null_handle_is_refused_and_nothing_is_written(lib, nq):
    dim, k, n = 12, 3, 40
    qs = {"": np.full((5, dim), 0.5, np.float32), "_f16": np.full((5, dim), 0.5, np.float16), "_i8": np.full((5, dim), 7, np.int8)}
    bits = np.full(5, 0xA5, np.uint8)
    dist = np.full((5, k), -3.0, np.float32)
    lab = np.full((5, k), -9, np.int64)
    for t, q in qs.items():
        host = getattr(lib, f"lb_gpu_index_search{t}_bitmap_ctx")
        dev = getattr(lib, f"lb_gpu_index_search{t}_bitmap_device_ctx")
        for bm in (bits.ctypes.data, None):
            assert host(None, nq, q.ctypes.data, k, bm, n, dist.ctypes.data, lab.ctypes.data, None) == INVALID
            assert dev(None, nq, q.ctypes.data, k, bm, n, dist.ctypes.data, lab.ctypes.data, None, None) == INVALID
    assert (dist == -3.0).all() and (lab == -9).all() and (bits == 0xA5).all()
    assert (qs[""] == 0.5).all() and (qs["_f16"] == 0.5).all() and (qs["_i8"] == 7).all()


def test_python_front_end_offers_the_arguments():
    import inspect
    from longbow_amd import gpu
    for name in ("Search", "SearchBatch"):
        s = inspect.signature(getattr(gpu.Index, name)).parameters
        assert s["bitmap"].default is None and s["ctx"].default is None
        assert list(s)[-2:] == ["ctx", "bitmap"]
    d = inspect.signature(gpu.Index.search_device).parameters
    assert d["d_bitmap"].default is None and d["nbits"].default == 0
    assert callable(gpu.pack_bitmap)


def test_cpp_and_go_wrappers_name_the_entry_point():
    hpp = open(os.path.join(ROOT, "include", "longbow_gpu.hpp")).read()
    assert "Error SearchBitmap(" in hpp and "Error SearchBatchBitmap(" in hpp and "lb_gpu_index_search_bitmap_ctx(" in hpp
    go = open(os.path.join(ROOT, "go", "internal", "gpu", "hip_gpu.go")).read()
    assert "func (idx *HIPIndex) SearchWithBitmap(vector []float32, k int, bitmap []byte)" in go
    assert "C.lb_gpu_index_search_bitmap_ctx(" in go
