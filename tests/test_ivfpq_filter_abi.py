"""lb_gpu_ivfpq_* row filters: the calls exist with the prototypes of the IVF-Flat handle's, and without a handle they answer
before a device is touched (LB_ERR_INVALID_ARG; nvisible 0) and write nothing, as tests/test_ivf_filter_abi.py shows of that
handle.  All of this runs on a box without a GPU; the checks behind a live handle are in tests/test_gpu_ivfpq_filters.py."""
import ctypes as C

import numpy as np
import pytest

INVALID = 1
PREFIX = "lb_gpu_ivfpq"
CALLS = ("set_filter", "filter_int64", "filter_float32")


@pytest.fixture(scope="module")
def lib():
    from longbow_amd import _lib
    return _lib.load()


def test_prototypes_mirror_the_ivf_flat_handle(lib):
    from longbow_amd import _lib
    sig = {name: (res, args) for name, res, args in _lib.SIGNATURES}
    for call in CALLS + ("nvisible", "last_build_timing"):
        assert sig[f"{PREFIX}_{call}"] == sig[f"lb_gpu_ivf_{call}"], call
        fn = getattr(lib, f"{PREFIX}_{call}")
        assert fn.restype is sig[f"{PREFIX}_{call}"][0] and list(fn.argtypes) == sig[f"{PREFIX}_{call}"][1]
    assert sig[f"{PREFIX}_nvisible"] == (C.c_int64, [C.c_void_p])


def test_null_handle_is_refused_and_nothing_is_written(lib):
    n = 5
    mask = np.full(n, 0xAB, np.uint8)
    col64 = np.full(n, 77, np.int64)
    col32 = np.full(n, 9.0, np.float32)
    valid = np.full(2, 0x5A, np.uint8)
    set_filter, f64, f32 = (getattr(lib, f"{PREFIX}_{c}") for c in CALLS)
    for nn in (n, 0, -1):
        assert set_filter(None, mask.ctypes.data, nn) == INVALID
        assert set_filter(None, None, nn) == INVALID
        for op in (0, 5, -1, 6):
            for voff in (0, 3, -1):
                for combine in (0, 1):
                    assert f64(None, col64.ctypes.data, nn, 5, op, valid.ctypes.data, voff, combine) == INVALID
                    assert f32(None, col32.ctypes.data, nn, 0.25, op, None, voff, combine) == INVALID
    assert lib.lb_gpu_ivfpq_nvisible(None) == 0
    ms = C.c_float(7.0)
    assert lib.lb_gpu_ivfpq_last_build_timing(None, C.byref(ms)) == INVALID and ms.value == 7.0
    assert (mask == 0xAB).all() and (col64 == 77).all() and (col32 == 9.0).all() and (valid == 0x5A).all()


def test_python_front_end_offers_the_calls():
    from longbow_amd import _rowfilter, ivfpq
    assert issubclass(ivfpq.IVFPQ, _rowfilter.RowFilterMixin) and ivfpq.IVFPQ._prefix == PREFIX
    for name in ("set_filter", "filter_column", "nvisible", "last_build_timing"):
        assert callable(getattr(ivfpq.IVFPQ, name)), name
