"""lb_gpu_pq4_*: every argument check that needs no handle answers before a device is touched, in the order
include/longbow_gpu.h states (INVALID_ARG, UNSUPPORTED, NO_DEVICE), and a refused call leaves its outputs untouched, so all of
this runs on a box without a GPU.  (What needs a live handle is in tests/test_gpu_pq4.py.)"""
import ctypes as C
import struct

import numpy as np
import pytest

INVALID, NO_DEVICE, UNSUPPORTED = 1, 3, 6
NAMES = ["new", "free", "last_error", "m", "dims", "ntotal", "hbm_bytes", "reserve", "add_codes", "add_codes_device", "add_vectors",
         "add_vectors_device", "get_codes", "encode", "encode_device", "build_adc_table", "adc_distance_batch", "search", "search_ctx",
         "search_device_ctx"]


@pytest.fixture(scope="module")
def lib():
    from longbow_amd import _lib
    return _lib.load()


def _blob(dims=16, M=4, K=16, extra=0):
    return struct.pack("<III", dims, M, K) + bytes(M * K * (dims // M if M else 0) * 4 + extra)


def _new(lib, blob, device=0):
    """-> the status of a refused lb_gpu_pq4_new (on a GPU box `device` is moved out of range so that nothing is created)"""
    if lib.lb_gpu_device_count() > 0 and device >= 0:
        device = 1 << 20
    st = C.c_int(-1)
    assert not lib.lb_gpu_pq4_new(device, blob, len(blob) if blob is not None else 0, C.byref(st))
    return st.value


def test_every_symbol_is_bound(lib):
    from longbow_amd import _lib
    bound = {name for name, _, _ in _lib.SIGNATURES}
    for n in NAMES:
        assert "lb_gpu_pq4_" + n in bound and getattr(lib, "lb_gpu_pq4_" + n).argtypes is not None


@pytest.mark.parametrize("blob,device,want", [
    (None, 0, INVALID),
    (b"garbage", 0, INVALID),                                  # too short for the header
    (_blob(extra=4), 0, INVALID),                              # size mismatch
    (_blob(dims=18, M=4), 0, INVALID),                         # dims % M != 0
    (struct.pack("<III", 16, 0, 16), 0, INVALID),              # M == 0
    (b"garbage", -1, INVALID),                                 # INVALID_ARG before NO_DEVICE
    (_blob(K=256), 0, UNSUPPORTED),
    (_blob(K=15), 0, UNSUPPORTED),
    (_blob(dims=1025, M=1025), 0, UNSUPPORTED),
    (_blob(dims=8193, M=1), 0, UNSUPPORTED),                   # dims > LB_MAX_DIM
    (_blob(K=256), -1, UNSUPPORTED),                           # UNSUPPORTED before NO_DEVICE
    (_blob(), -1, NO_DEVICE),
    (_blob(dims=1024, M=1024), 0, NO_DEVICE),                  # the largest M parses and is supported
])
def test_new_checks_its_arguments_in_the_documented_order(lib, blob, device, want):
    assert _new(lib, blob, device) == want
    assert not lib.lb_gpu_pq4_new(device if device < 0 else 1 << 20, blob, len(blob) if blob else 0, None)  # out_status is nullable


def test_null_handle_is_refused_everywhere_and_nothing_is_written(lib):
    f32 = np.full(64, 9.0, np.float32)
    i64 = np.full(64, 77, np.int64)
    u8 = np.full(64, 0xA5, np.uint8)
    f, i, u = f32.ctypes.data, i64.ctypes.data, u8.ctypes.data
    for n in (3, 0, -1):
        assert lib.lb_gpu_pq4_reserve(None, n) == INVALID
        assert lib.lb_gpu_pq4_add_codes(None, n, u) == INVALID
        assert lib.lb_gpu_pq4_add_codes_device(None, n, u) == INVALID
        assert lib.lb_gpu_pq4_add_vectors(None, n, f) == INVALID
        assert lib.lb_gpu_pq4_add_vectors_device(None, n, f) == INVALID
        assert lib.lb_gpu_pq4_get_codes(None, 0, n, u) == INVALID
        assert lib.lb_gpu_pq4_encode(None, n, f, u) == INVALID
        assert lib.lb_gpu_pq4_encode_device(None, n, f, u, None) == INVALID
        assert lib.lb_gpu_pq4_adc_distance_batch(None, f, 0, n, f) == INVALID
        for k in (4, 0, 4097):  # INVALID_ARG comes before UNSUPPORTED
            assert lib.lb_gpu_pq4_search(None, n, f, k, f, i) == INVALID
            assert lib.lb_gpu_pq4_search_ctx(None, n, f, k, f, i, None) == INVALID
            assert lib.lb_gpu_pq4_search_device_ctx(None, n, f, k, f, i, None, None) == INVALID
    assert lib.lb_gpu_pq4_build_adc_table(None, f, f) == INVALID
    assert (f32 == 9.0).all() and (i64 == 77).all() and (u8 == 0xA5).all()
    assert lib.lb_gpu_pq4_m(None) == 0 and lib.lb_gpu_pq4_dims(None) == 0
    assert lib.lb_gpu_pq4_ntotal(None) == 0 and lib.lb_gpu_pq4_hbm_bytes(None) == 0
    assert lib.lb_gpu_pq4_last_error(None) == b"null handle"
    lib.lb_gpu_pq4_free(None)


def test_python_front_end_fails_loudly_without_a_gpu(lib):
    import longbow_amd
    from longbow_amd import _lib, pq4
    assert "pq4" in longbow_amd.__all__
    device = 1 << 20 if lib.lb_gpu_device_count() > 0 else 0
    with pytest.raises(_lib.GPUNotAvailable):
        pq4.PQ4Encoder(_blob(), device=device)
    with pytest.raises(_lib.GPUNotAvailable):
        pq4.PQ4Encoder.Train(np.zeros((64, 8), np.float32), 2, device=device)
