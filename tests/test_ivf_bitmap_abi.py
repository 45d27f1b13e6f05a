"""The four entry points that take a row bitmap with the search call (include/longbow_gpu.h, lb_gpu_ivf_*: "call bitmap") on a box
without a GPU: declared, exported from both builds of the library, bound with their prototypes -- the plain entry points' argument
lists with (bitmap, nbits, stride_bytes) behind nprobe in all four -- and refusing a NULL handle before a device is touched, with
nothing written.  The checks behind a live handle are in tests/test_gpu_ivf_bitmap.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
_vp, _i, _i64 = C.c_void_p, C.c_int, C.c_int64
NEW_ARGS = [_vp, _i64, _i64]  # bitmap, nbits, stride_bytes
AT = 5                        # behind (p, nq, queries, k, nprobe)
PLAIN = {                     # the entry point each one extends
    "lb_gpu_ivf_search_bitmap_ctx": "lb_gpu_ivf_search_ctx",
    "lb_gpu_ivf_search_bitmap_device_ctx": "lb_gpu_ivf_search_device_ctx",
    "lb_gpu_ivf_search_i8_bitmap_ctx": "lb_gpu_ivf_search_i8_ctx",
    "lb_gpu_ivf_search_i8_bitmap_device_ctx": "lb_gpu_ivf_search_i8_device_ctx",
}
_Q = {"": r"const float \*", "_i8": r"const int8_t \*"}
DECLARATIONS = [
    rf"int\s+lb_gpu_ivf_search{t}_bitmap_ctx\s*\(\s*lb_gpu_ivf \*p,\s*int64_t nq,\s*{q}queries,\s*int k,\s*int nprobe,\s*"
    rf"const uint8_t \*bitmap,\s*int64_t nbits,\s*int64_t stride_bytes,\s*float \*dist,\s*int64_t \*labels,\s*const lb_cancel \*ctx\)"
    for t, q in _Q.items()
] + [
    rf"int\s+lb_gpu_ivf_search{t}_bitmap_device_ctx\s*\(\s*lb_gpu_ivf \*p,\s*int64_t nq,\s*{q}d_queries,\s*int k,\s*int nprobe,\s*"
    rf"const uint8_t \*d_bitmap,\s*int64_t nbits,\s*int64_t stride_bytes,\s*float \*d_dist,\s*int64_t \*d_labels,\s*void \*stream,\s*"
    rf"const lb_cancel \*ctx\)"
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
        assert args == pargs[:AT] + NEW_ARGS + pargs[AT:], (name, args)   # the same place in all four
        fn = getattr(lib, name)
        assert fn.restype is _i and list(fn.argtypes) == args


def test_the_header_no_longer_lists_it_as_missing_on_this_handle():
    header = open(os.path.join(ROOT, "include", "longbow_gpu.h")).read()
    start = header.index("---- IVF-Flat: exact k-NN over the probed lists")
    block = header[start:header.index("typedef struct lb_gpu_ivf lb_gpu_ivf;")]
    assert "Not here" in block and "a filter given per search call" not in block
    flat = re.sub(r"[\s*]+", " ", header)                                   # (the sentence wraps inside the comment blocks)
    assert "a filter given per search call" in flat                        # the code handles' blocks keep what they say of it


def test_the_diagnostic_build_exports_them_too():
    from longbow_amd import _lib, build
    build.build(diag=True)
    out = _exports(_lib.DIAG_SO_PATH)
    for name in PLAIN:
        assert re.search(rf"\b{name}\b", out), f"{name} not exported by the diagnostic build"


@pytest.mark.parametrize("nq", [5, 0, -1])
def test_null_handle_is_refused_and_nothing_is_written(lib, nq):
    dim, k, n = 12, 3, 40
    qf = np.full((5, dim), 0.5, np.float32)
    q8 = np.full((5, dim), 7, np.int8)
    bits = np.full(5 * 5, 0xA5, np.uint8)
    dist = np.full((5, k), -3.0, np.float32)
    lab = np.full((5, k), -9, np.int64)
    for q, t in ((qf, ""), (q8, "_i8")):
        host = getattr(lib, f"lb_gpu_ivf_search{t}_bitmap_ctx")
        dev = getattr(lib, f"lb_gpu_ivf_search{t}_bitmap_device_ctx")
        for bm, stride in ((bits.ctypes.data, 0), (bits.ctypes.data, 5), (None, 0)):
            assert host(None, nq, q.ctypes.data, k, 2, bm, n, stride, dist.ctypes.data, lab.ctypes.data, None) == INVALID
            assert dev(None, nq, q.ctypes.data, k, 2, bm, n, stride, dist.ctypes.data, lab.ctypes.data, None, None) == INVALID
    assert (dist == -3.0).all() and (lab == -9).all() and (bits == 0xA5).all() and (qf == 0.5).all() and (q8 == 7).all()


def test_python_front_end_offers_the_arguments():
    import inspect
    from longbow_amd import ivf
    for cls in (ivf.IVFFlat, ivf.IVFFlatInt8):
        s = inspect.signature(cls.search).parameters
        assert s["bitmap"].default is None and s["bitmap_stride"].default == 0 and s["ctx"].default is None
        d = inspect.signature(cls.search_device).parameters
        assert d["d_bitmap"].default is None and d["nbits"].default == 0 and d["bitmap_stride"].default == 0
    for name in ("SearchBatch", "Search"):
        assert inspect.signature(getattr(ivf.IVFFlatIndex, name)).parameters["bitmap"].default is None
    assert callable(ivf.pack_bitmap)
