"""The removal entry points of the IVF-PQ and IVF-SQ8 handles on a box without a GPU: lb_gpu_ivfpq_* and lb_gpu_ivfsq8_*
_remove, _remove_device, _remove_rows, _nlive, _ndeleted and _compact (include/longbow_gpu.h) are declared, exported from both
builds of the library, bound with their prototypes, and refuse bad arguments before a device is touched; the Python classes offer
the methods."""
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
PREFIXES = ("lb_gpu_ivfpq", "lb_gpu_ivfsq8")
REMOVALS = ("remove", "remove_device", "remove_rows")


def _prototypes(prefix):
    out = {f"{prefix}_{name}": (_i, [_vp, _i64, _vp, _p64]) for name in REMOVALS}
    out.update({f"{prefix}_nlive": (_i64, [_vp]), f"{prefix}_ndeleted": (_i64, [_vp]), f"{prefix}_compact": (_i, [_vp, _vp, _i64])})
    return out


def _declarations(prefix):
    return [
        rf"int\s+{prefix}_remove\s*\(\s*{prefix} \*p,\s*int64_t n,\s*const int64_t \*labels,\s*int64_t \*n_removed\)",
        rf"int\s+{prefix}_remove_device\s*\(\s*{prefix} \*p,\s*int64_t n,\s*const int64_t \*d_labels,\s*int64_t \*n_removed\)",
        rf"int\s+{prefix}_remove_rows\s*\(\s*{prefix} \*p,\s*int64_t n,\s*const int64_t \*rows,\s*int64_t \*n_removed\)",
        rf"int64_t\s+{prefix}_nlive\s*\(\s*const {prefix} \*p\)",
        rf"int64_t\s+{prefix}_ndeleted\s*\(\s*const {prefix} \*p\)",
        rf"int\s+{prefix}_compact\s*\(\s*{prefix} \*p,\s*int64_t \*old_rows,\s*int64_t cap\)",
    ]


PROTOTYPES = {name: proto for prefix in PREFIXES for name, proto in _prototypes(prefix).items()}


@pytest.fixture(scope="module")
def lib():
    from longbow_amd import _lib, build
    build.build()
    return _lib.load()


def _exports(path):
    return subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout


def test_the_twelve_symbols_are_declared_exported_and_bound(lib):
    from longbow_amd import _lib
    assert len(PROTOTYPES) == 12
    header = open(os.path.join(ROOT, "include", "longbow_gpu.h")).read()
    for prefix in PREFIXES:
        for pat in _declarations(prefix):
            assert re.search(pat, header), pat
    bound = {s[0]: (s[1], s[2]) for s in _lib.SIGNATURES}
    out = _exports(_lib.SO_PATH)
    for name, (res, args) in PROTOTYPES.items():
        assert re.search(rf"\b{name}\b", out), f"{name} not exported"
        assert name in bound, f"{name} missing from _lib.SIGNATURES"
        assert bound[name][0] is res and list(bound[name][1]) == args, (name, bound[name])


def test_the_diagnostic_build_exports_them_too_and_still_one_round_hook():
    """the compaction's round walk stays defined once (lb_remove.h) and its hook exported once, by the diagnostic build alone"""
    from longbow_amd import _lib, build
    build.build(diag=True)
    out = _exports(_lib.DIAG_SO_PATH)
    for name in PROTOTYPES:
        assert re.search(rf"\b{name}\b", out), f"{name} not exported by the diagnostic build"
    assert len(re.findall(r"\blb_debug_set_compact_round_rows\b", out)) == 1
    assert "lb_debug_set_compact_round_rows" not in _exports(_lib.SO_PATH)
    csrc = os.path.join(ROOT, "longbow_amd", "csrc")
    sources = [f for f in sorted(os.listdir(csrc)) if f.endswith((".h", ".hip"))]
    hooks = [f for f in sources if re.search(r"^void lb_debug_set_compact_round_rows\(", open(os.path.join(csrc, f)).read(), re.M)]
    assert hooks == ["index_remove.hip"], hooks


@pytest.mark.parametrize("n", [5, 0, -1])
@pytest.mark.parametrize("prefix", PREFIXES)
def test_null_handle_is_refused_and_nothing_is_written(lib, prefix, n):
    values = np.array([3, 1, 4, 1, 5], np.int64)
    before = values.copy()
    for name in REMOVALS:
        fn = getattr(lib, f"{prefix}_{name}")
        removed = C.c_int64(-77)
        assert fn(None, n, values.ctypes.data, C.byref(removed)) == LB_ERR_INVALID_ARG, (name, n)
        assert removed.value == -77, name
        assert fn(None, n, None, None) == LB_ERR_INVALID_ARG, (name, n)
    assert np.array_equal(values, before)
    compact = getattr(lib, f"{prefix}_compact")
    old = np.full(5, -77, np.int64)
    assert compact(None, old.ctypes.data, n) == LB_ERR_INVALID_ARG
    assert compact(None, None, n) == LB_ERR_INVALID_ARG
    assert np.all(old == -77)


@pytest.mark.parametrize("prefix", PREFIXES)
def test_counts_of_a_null_handle(lib, prefix):
    assert getattr(lib, f"{prefix}_nlive")(None) == 0
    assert getattr(lib, f"{prefix}_ndeleted")(None) == 0


def test_python_front_end_offers_the_methods():
    from longbow_amd import ivf, ivfpq, ivfsq8
    for cls in (ivfpq.IVFPQ, ivfsq8.IVFSQ8):
        assert issubclass(cls, ivf.RemovalMixin), cls.__name__
        for name in ("remove", "remove_rows", "remove_device", "compact", "nlive", "ndeleted"):
            assert callable(getattr(cls, name, None)), (cls.__name__, name)
        assert "compact" in cls.search_refine.__doc__ and "live rows only" in cls.search_refine.__doc__, cls.__name__
