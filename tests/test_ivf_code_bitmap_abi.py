"""The four entry points that take a row bitmap with the search call on the IVF-PQ and IVF-SQ8 handles (include/longbow_gpu.h,
lb_gpu_ivfpq_search_bitmap_ctx / _bitmap_device_ctx and lb_gpu_ivfsq8_search_bitmap_ctx / _bitmap_device_ctx) on a box without a
GPU: declared with the IVF-Flat handle's argument order, exported from both builds of the library, bound with their prototypes
-- the plain entry points' argument lists with (bitmap, nbits, stride_bytes) behind nprobe -- and refusing a NULL handle before a
device is touched, with nothing written.  The checks behind a live handle are in tests/test_gpu_ivf_code_bitmap.py."""
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
HANDLES = ("ivfpq", "ivfsq8")
PLAIN = {f"lb_gpu_{h}_search_bitmap{d}_ctx": f"lb_gpu_{h}_search{d}_ctx" for h in HANDLES for d in ("", "_device")}
DECLARATIONS = [
    rf"int\s+lb_gpu_{h}_search_bitmap_ctx\s*\(\s*lb_gpu_{h} \*p,\s*int64_t nq,\s*const float \*queries,\s*int k,\s*int nprobe,\s*"
    rf"const uint8_t \*bitmap,\s*int64_t nbits,\s*int64_t stride_bytes,\s*float \*dist,\s*int64_t \*labels,\s*const lb_cancel \*ctx\)"
    for h in HANDLES
] + [
    rf"int\s+lb_gpu_{h}_search_bitmap_device_ctx\s*\(\s*lb_gpu_{h} \*p,\s*int64_t nq,\s*const float \*d_queries,\s*int k,\s*int nprobe,\s*"
    rf"const uint8_t \*d_bitmap,\s*int64_t nbits,\s*int64_t stride_bytes,\s*float \*d_dist,\s*int64_t \*d_labels,\s*void \*stream,\s*"
    rf"const lb_cancel \*ctx\)"
    for h in HANDLES
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
    assert len(PLAIN) == 4
    for name, plain in PLAIN.items():
        assert re.search(rf"\b{name}\b", out), f"{name} not exported"
        assert name in bound, f"{name} missing from _lib.SIGNATURES"
        res, args = bound[name]
        pres, pargs = bound[plain]
        assert res is pres is _i
        assert args == pargs[:AT] + NEW_ARGS + pargs[AT:], (name, args)   # the same place in all four
        assert args == bound[name.replace("ivfpq", "ivf").replace("ivfsq8", "ivf")][1]  # the IVF-Flat handle's order
        fn = getattr(lib, name)
        assert fn.restype is _i and list(fn.argtypes) == args


def test_the_ivfbq_handle_has_none():
    from longbow_amd import _lib
    assert not [s[0] for s in _lib.SIGNATURES if s[0].startswith("lb_gpu_ivfbq") and "bitmap" in s[0]]
    assert not re.search(r"lb_gpu_ivfbq_\w*bitmap", _exports(_lib.SO_PATH))


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
    bits = np.full(5 * 5, 0xA5, np.uint8)
    dist = np.full((5, k), -3.0, np.float32)
    lab = np.full((5, k), -9, np.int64)
    for h in HANDLES:
        host = getattr(lib, f"lb_gpu_{h}_search_bitmap_ctx")
        dev = getattr(lib, f"lb_gpu_{h}_search_bitmap_device_ctx")
        for bm in (bits.ctypes.data, None):
            for stride in (0, 5, 1, -1):
                assert host(None, nq, qf.ctypes.data, k, 2, bm, n, stride, dist.ctypes.data, lab.ctypes.data, None) == INVALID
                assert dev(None, nq, qf.ctypes.data, k, 2, bm, n, stride, dist.ctypes.data, lab.ctypes.data, None, None) == INVALID
    assert (dist == -3.0).all() and (lab == -9).all() and (bits == 0xA5).all() and (qf == 0.5).all()


def test_python_front_end_offers_the_arguments():
    import inspect
    from longbow_amd import ivfpq, ivfsq8
    for mod, cls in ((ivfpq, ivfpq.IVFPQ), (ivfsq8, ivfsq8.IVFSQ8)):
        s = inspect.signature(cls.search).parameters
        assert s["bitmap"].default is None and s["bitmap_stride"].default == 0 and s["ctx"].default is None
        d = inspect.signature(cls.search_device).parameters
        assert d["d_bitmap"].default is None and d["nbits"].default == 0 and d["bitmap_stride"].default == 0
        r = inspect.signature(cls.search_refine).parameters
        assert r["bitmap"].default is None and r["bitmap_stride"].default == 0
        assert "bitmap" in cls.last_timing.__doc__ and "plan" in cls.last_timing.__doc__
        from longbow_amd import _rowfilter
        assert mod.pack_bitmap is _rowfilter.pack_bitmap
