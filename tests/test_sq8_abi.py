"""lb_gpu_sq8_*: every argument check that needs no handle answers before a device is touched, in the order
include/longbow_gpu.h states (INVALID_ARG, UNSUPPORTED, NO_DEVICE), and a refused call leaves its output buffers untouched, so
all of this runs on a box without a GPU.  (A handle exists only where a device does: the checks behind a live handle, k above
LB_MAX_K and the untrained refusals among them, are in tests/test_gpu_sq8.py.)"""
import ctypes as C

import numpy as np
import pytest

INVALID, NO_DEVICE, UNSUPPORTED = 1, 3, 6
LB_MAX_DIM, LB_MAX_K = 8192, 2048


@pytest.fixture(scope="module")
def lib():
    from longbow_amd import _lib
    return _lib.load()


def _new(lib, dims, device=0):
    """on a GPU box `device` is moved out of range so that nothing is ever created"""
    if lib.lb_gpu_device_count() > 0 and device >= 0:
        device = 1 << 20
    st = C.c_int(-1)
    h = lib.lb_gpu_sq8_new(device, dims, C.byref(st))
    assert not h
    return st.value


def test_new_checks_its_arguments_in_the_documented_order(lib):
    assert _new(lib, 0) == INVALID
    assert _new(lib, -1) == INVALID
    assert _new(lib, -(1 << 31)) == INVALID
    assert _new(lib, 0, device=-1) == INVALID          # INVALID_ARG before NO_DEVICE
    assert _new(lib, LB_MAX_DIM + 1) == UNSUPPORTED
    assert _new(lib, 1 << 30) == UNSUPPORTED
    assert _new(lib, LB_MAX_DIM + 1, device=-1) == UNSUPPORTED  # UNSUPPORTED before NO_DEVICE
    for dims in (1, 15, 16, 17, 768, LB_MAX_DIM):
        assert _new(lib, dims) == NO_DEVICE
    assert _new(lib, 768, device=-1) == NO_DEVICE
    # out_status is nullable
    assert not lib.lb_gpu_sq8_new(-1, 768, None) and not lib.lb_gpu_sq8_new(0, 0, None)


def test_null_handle_is_refused_everywhere_and_nothing_is_written(lib):
    dims, n, k = 20, 3, 4
    codes = np.full((n, dims), 0xAB, np.uint8)
    vec = np.full((n, dims), 7.0, np.float32)
    lo = np.full(dims, -3.0, np.float32)
    hi = np.full(dims, 3.0, np.float32)
    i32 = np.full(n, 0x5A5A5A5A, np.int32)
    f32 = np.full(n * k, 9.0, np.float32)
    f32b = np.full(n * k, 9.0, np.float32)
    i64 = np.full(n * k, 77, np.int64)
    rows = np.arange(n, dtype=np.int64)
    c, v, r = codes.ctypes.data, vec.ctypes.data, rows.ctypes.data
    for kk in (k, 0, -1, LB_MAX_K, LB_MAX_K + 1):  # INVALID_ARG comes before UNSUPPORTED: no handle and k too large -> invalid
        for nn in (n, 0, -1):
            assert lib.lb_gpu_sq8_search(None, nn, v, kk, f32.ctypes.data, i64.ctypes.data) == INVALID
            assert lib.lb_gpu_sq8_search_ctx(None, nn, v, kk, f32.ctypes.data, i64.ctypes.data, None) == INVALID
            assert lib.lb_gpu_sq8_search_codes(None, nn, c, kk, f32.ctypes.data, i64.ctypes.data) == INVALID
            assert lib.lb_gpu_sq8_search_device_ctx(None, nn, v, kk, f32.ctypes.data, i64.ctypes.data, None, None) == INVALID
    for nn in (n, 0, -1):
        assert lib.lb_gpu_sq8_add_codes(None, nn, c) == INVALID
        assert lib.lb_gpu_sq8_add_codes_device(None, nn, c) == INVALID
        assert lib.lb_gpu_sq8_add_vectors(None, nn, v) == INVALID
        assert lib.lb_gpu_sq8_add_vectors_device(None, nn, v) == INVALID
        assert lib.lb_gpu_sq8_get_codes(None, 0, nn, c) == INVALID
        assert lib.lb_gpu_sq8_encode(None, nn, v, c) == INVALID
        assert lib.lb_gpu_sq8_encode_device(None, nn, v, c, None) == INVALID
        assert lib.lb_gpu_sq8_decode(None, nn, c, v) == INVALID
        assert lib.lb_gpu_sq8_train(None, nn, v) == INVALID
        assert lib.lb_gpu_sq8_train_device(None, nn, v) == INVALID
        assert lib.lb_gpu_sq8_distance_batch(None, c, 0, nn, i32.ctypes.data) == INVALID
        assert lib.lb_gpu_sq8_rerank(None, c, r, nn, i32.ctypes.data, f32b.ctypes.data) == INVALID
        assert lib.lb_gpu_sq8_rerank_device(None, c, r, nn, i32.ctypes.data, None, None) == INVALID
        assert lib.lb_gpu_sq8_reserve(None, nn) == INVALID
    assert lib.lb_gpu_sq8_set_bounds(None, lo.ctypes.data, hi.ctypes.data) == INVALID
    assert lib.lb_gpu_sq8_get_bounds(None, lo.ctypes.data, hi.ctypes.data) == INVALID
    assert (codes == 0xAB).all() and (vec == 7.0).all() and (i32 == 0x5A5A5A5A).all() and (lo == -3.0).all() and (hi == 3.0).all()
    assert (f32 == 9.0).all() and (f32b == 9.0).all() and (i64 == 77).all() and (rows == np.arange(n)).all()
    # the accessors of no handle
    assert lib.lb_gpu_sq8_dims(None) == 0 and lib.lb_gpu_sq8_ntotal(None) == 0 and lib.lb_gpu_sq8_trained(None) == 0
    assert lib.lb_gpu_sq8_last_error(None) == b"null handle"
    lib.lb_gpu_sq8_free(None)


def test_python_front_end_fails_loudly_without_a_gpu(lib):
    from longbow_amd import _lib, sq8
    import longbow_amd
    assert "sq8" in longbow_amd.__all__
    device = 1 << 20 if lib.lb_gpu_device_count() > 0 else 0  # (a device that is not there, on a GPU box too)
    with pytest.raises(_lib.GPUNotAvailable):
        sq8.SQ8Encoder(768, device=device)
    with pytest.raises(ValueError):
        sq8.SQ8Encoder(0, device=device)
    with pytest.raises(_lib.GPUNotAvailable):
        sq8.train(np.zeros((4, 8), np.float32), device=device)
    with pytest.raises(ValueError, match="no vectors"):
        sq8.train(np.zeros((0, 8), np.float32), device=device)
    with pytest.raises(ValueError, match="zero dimensions"):
        sq8.train(np.zeros((4, 0), np.float32), device=device)
