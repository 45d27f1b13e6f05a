"""The IVF-Flat removal entry points on a box without a GPU: declared, exported from both builds of the library, bound with their
prototypes, and refusing bad arguments before a device is touched (include/longbow_gpu.h: lb_gpu_ivf_remove*, _nlive, _ndeleted,
_compact)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LB_ERR_INVALID_ARG = 1
_vp, _i, _i64 = C.c_void_p, C.c_int, C.c_int64
_p64 = C.POINTER(C.c_int64)
PROTOTYPES = {
    "lb_gpu_ivf_remove": (_i, [_vp, _i64, _vp, _p64]),
    "lb_gpu_ivf_remove_device": (_i, [_vp, _i64, _vp, _p64]),
    "lb_gpu_ivf_remove_rows": (_i, [_vp, _i64, _vp, _p64]),
    "lb_gpu_ivf_nlive": (_i64, [_vp]),
    "lb_gpu_ivf_ndeleted": (_i64, [_vp]),
    "lb_gpu_ivf_compact": (_i, [_vp, _vp, _i64]),
}
DECLARATIONS = [
    r"int\s+lb_gpu_ivf_remove\s*\(\s*lb_gpu_ivf \*p,\s*int64_t n,\s*const int64_t \*labels,\s*int64_t \*n_removed\)",
    r"int\s+lb_gpu_ivf_remove_device\s*\(\s*lb_gpu_ivf \*p,\s*int64_t n,\s*const int64_t \*d_labels,\s*int64_t \*n_removed\)",
    r"int\s+lb_gpu_ivf_remove_rows\s*\(\s*lb_gpu_ivf \*p,\s*int64_t n,\s*const int64_t \*rows,\s*int64_t \*n_removed\)",
    r"int64_t\s+lb_gpu_ivf_nlive\s*\(\s*const lb_gpu_ivf \*p\)",
    r"int64_t\s+lb_gpu_ivf_ndeleted\s*\(\s*const lb_gpu_ivf \*p\)",
    r"int\s+lb_gpu_ivf_compact\s*\(\s*lb_gpu_ivf \*p,\s*int64_t \*old_rows,\s*int64_t cap\)",
]
REMOVALS = ("lb_gpu_ivf_remove", "lb_gpu_ivf_remove_device", "lb_gpu_ivf_remove_rows")


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
    bound = {s[0]: (s[1], s[2]) for s in _lib.SIGNATURES}
    out = _exports(_lib.SO_PATH)
    for name, (res, args) in PROTOTYPES.items():
        assert re.search(rf"\b{name}\b", out), f"{name} not exported"
        assert name in bound, f"{name} missing from _lib.SIGNATURES"
        assert bound[name][0] is res and list(bound[name][1]) == args, (name, bound[name])


def test_the_diagnostic_build_exports_them_too_and_one_round_hook():
    """the compaction's round walk is defined once (lb_remove.h): the one hook serves the flat index and this handle"""
    from longbow_amd import _lib, build
    build.build(diag=True)
    out = _exports(_lib.DIAG_SO_PATH)
    for name in PROTOTYPES:
        assert re.search(rf"\b{name}\b", out), f"{name} not exported by the diagnostic build"
    assert len(re.findall(r"\blb_debug_set_compact_round_rows\b", out)) == 1
    assert "lb_debug_set_compact_round_rows" not in _exports(_lib.SO_PATH)
    csrc = os.path.join(ROOT, "longbow_amd", "csrc")
    sources = [f for f in sorted(os.listdir(csrc)) if f.endswith((".h", ".hip"))]
    defs = [f for f in sources if "g_compact_round_rows{" in open(os.path.join(csrc, f)).read()]
    assert defs == ["lb_remove.h"], defs


@pytest.mark.parametrize("n", [5, 0, -1])
def test_null_handle_is_refused_and_nothing_is_written(lib, n):
    values = np.array([3, 1, 4, 1, 5], np.int64)
    before = values.copy()
    for name in REMOVALS:
        removed = C.c_int64(-77)
        assert getattr(lib, name)(None, n, values.ctypes.data, C.byref(removed)) == LB_ERR_INVALID_ARG, (name, n)
        assert removed.value == -77, name
        assert getattr(lib, name)(None, n, None, None) == LB_ERR_INVALID_ARG, (name, n)
    assert np.array_equal(values, before)
    old = np.full(5, -77, np.int64)
    assert lib.lb_gpu_ivf_compact(None, old.ctypes.data, n) == LB_ERR_INVALID_ARG
    assert lib.lb_gpu_ivf_compact(None, None, n) == LB_ERR_INVALID_ARG
    assert np.all(old == -77)


def test_counts_of_a_null_handle(lib):
    assert lib.lb_gpu_ivf_nlive(None) == 0
    assert lib.lb_gpu_ivf_ndeleted(None) == 0


def test_python_front_end_offers_the_methods():
    from longbow_amd import ivf
    for cls in (ivf.IVFFlat, ivf.IVFFlatInt8):
        for name in ("remove", "remove_rows", "remove_device", "compact", "nlive", "ndeleted"):
            assert callable(getattr(cls, name, None)), (cls.__name__, name)
    for name in ("Remove", "Compact", "nlive", "ndeleted", "Size"):
        assert callable(getattr(ivf.IVFFlatIndex, name, None)), name
