"""lb_gpu_ivfpq_*: every argument check that needs no handle answers before a device is touched, in the order
include/longbow_gpu.h states (INVALID_ARG, UNSUPPORTED, NO_DEVICE), and a refused call leaves its output buffers untouched, so
all of this runs on a box without a GPU.  (A handle exists only where a device does: the checks behind a live handle, k above
LB_MAX_K and nprobe <= 0 among them, are in tests/test_gpu_ivfpq.py.)"""
import ctypes as C
import struct

import numpy as np
import pytest

INVALID, NO_DEVICE, UNSUPPORTED = 1, 3, 6
LB_MAX_DIM, LB_MAX_K, MAX_NLIST = 8192, 2048, 65536


@pytest.fixture(scope="module")
def lib():
    from longbow_amd import _lib
    return _lib.load()


def _blob(dims=16, M=4, K=256, extra=0):
    return struct.pack("<III", dims, M, K) + bytes(M * K * (dims // M if M else 0) * 4 + extra)


def _new(lib, blob=None, order=0, nlist=4, device=0, cent=True, length=None, null_blob=False):
    """on a GPU box `device` is moved out of range so that nothing is ever created"""
    if lib.lb_gpu_device_count() > 0 and device >= 0:
        device = 1 << 20
    blob = _blob() if blob is None else blob
    c = np.zeros(64, np.float32)  # (never read: every call here is refused first)
    st = C.c_int(-1)
    h = lib.lb_gpu_ivfpq_new(device, None if null_blob else blob, len(blob) if length is None else length, order, nlist,
                             c.ctypes.data if cent else None, C.byref(st))
    assert not h
    return st.value


def test_new_checks_its_arguments_in_the_documented_order(lib):
    assert _new(lib, null_blob=True) == INVALID
    assert _new(lib, length=8) == INVALID                              # too short for the header
    assert _new(lib, _blob(extra=4)) == INVALID                        # size mismatch
    assert _new(lib, _blob()[:-4]) == INVALID
    assert _new(lib, _blob(dims=18, M=4)) == INVALID                   # dims % M != 0
    assert _new(lib, struct.pack("<III", 16, 0, 256)) == INVALID       # M == 0
    assert _new(lib, order=2) == INVALID
    assert _new(lib, order=-1) == INVALID
    assert _new(lib, nlist=0) == INVALID
    assert _new(lib, nlist=-3) == INVALID
    assert _new(lib, cent=False) == INVALID
    assert _new(lib, nlist=0, device=-1) == INVALID                    # INVALID_ARG before NO_DEVICE
    assert _new(lib, _blob(K=16), nlist=0) == INVALID                  # INVALID_ARG before UNSUPPORTED
    assert _new(lib, _blob(K=16)) == UNSUPPORTED                       # K != 256
    assert _new(lib, _blob(K=257)) == UNSUPPORTED
    assert _new(lib, _blob(dims=160, M=160)) == UNSUPPORTED            # M * 1024 B beyond LDS
    assert _new(lib, _blob(dims=LB_MAX_DIM + 1, M=1)) == UNSUPPORTED   # dims > LB_MAX_DIM
    assert _new(lib, nlist=MAX_NLIST + 1) == UNSUPPORTED
    assert _new(lib, _blob(K=16), device=-1) == UNSUPPORTED            # UNSUPPORTED before NO_DEVICE
    for dims, M in ((16, 4), (159, 159), (768, 96), (4, 1)):           # (159: the largest table that fits)
        for order in (0, 1):
            for nlist in (1, 7, MAX_NLIST):
                assert _new(lib, _blob(dims, M), order=order, nlist=nlist) == NO_DEVICE
    assert _new(lib, device=-1) == NO_DEVICE
    # out_status is nullable
    c = np.zeros(64, np.float32)
    b = _blob()
    assert not lib.lb_gpu_ivfpq_new(-1, b, len(b), 0, 4, c.ctypes.data, None)
    assert not lib.lb_gpu_ivfpq_new(0, None, 0, 0, 4, c.ctypes.data, None)


def test_null_handle_is_refused_everywhere_and_nothing_is_written(lib):
    dim, n, k = 20, 3, 4
    vec = np.full((n, dim), 7.0, np.float32)
    ids = np.full(n, 55, np.int64)
    f32 = np.full(n * k, 9.0, np.float32)
    i64 = np.full(n * k, 77, np.int64)
    i32 = np.full(n, 0x5A5A5A5A, np.int32)
    u8 = np.full(n * 8, 0xA5, np.uint8)
    sizes = np.full(8, 31, np.int64)
    stats = (C.c_int64 * 4)(5, 5, 5, 5)
    ms = (C.c_float * 5)(2, 2, 2, 2, 2)
    v = vec.ctypes.data
    for kk in (k, 0, -1, LB_MAX_K, LB_MAX_K + 1):  # INVALID_ARG comes before UNSUPPORTED: no handle and k too large -> invalid
        for nn in (n, 0, -1):
            for nprobe in (1, 0, -1):
                assert lib.lb_gpu_ivfpq_search(None, nn, v, kk, nprobe, f32.ctypes.data, i64.ctypes.data) == INVALID
                assert lib.lb_gpu_ivfpq_search_ctx(None, nn, v, kk, nprobe, f32.ctypes.data, i64.ctypes.data, None) == INVALID
                assert lib.lb_gpu_ivfpq_search_device_ctx(None, nn, v, kk, nprobe, f32.ctypes.data, i64.ctypes.data, None, None) == INVALID
    for nn in (n, 0, -1):
        assert lib.lb_gpu_ivfpq_add(None, nn, v, None) == INVALID
        assert lib.lb_gpu_ivfpq_add(None, nn, v, ids.ctypes.data) == INVALID
        assert lib.lb_gpu_ivfpq_add_device(None, nn, v, None) == INVALID
        assert lib.lb_gpu_ivfpq_assignments(None, 0, nn, i32.ctypes.data) == INVALID
        assert lib.lb_gpu_ivfpq_get_codes(None, 0, nn, u8.ctypes.data) == INVALID
        assert lib.lb_gpu_ivfpq_reserve(None, nn) == INVALID
    assert lib.lb_gpu_ivfpq_list_sizes(None, sizes.ctypes.data) == INVALID
    assert lib.lb_gpu_ivfpq_get_centroids(None, v) == INVALID
    assert lib.lb_gpu_ivfpq_last_search_stats(None, stats) == INVALID
    assert lib.lb_gpu_ivfpq_set_profiling(None, 1) == INVALID
    assert lib.lb_gpu_ivfpq_last_timing(None, ms) == INVALID
    assert (vec == 7.0).all() and (ids == 55).all() and (f32 == 9.0).all() and (i64 == 77).all() and (i32 == 0x5A5A5A5A).all()
    assert (u8 == 0xA5).all() and (sizes == 31).all() and list(stats) == [5, 5, 5, 5] and list(ms) == [2, 2, 2, 2, 2]
    # the accessors of no handle
    assert lib.lb_gpu_ivfpq_dims(None) == 0 and lib.lb_gpu_ivfpq_m(None) == 0 and lib.lb_gpu_ivfpq_order(None) == 0
    assert lib.lb_gpu_ivfpq_nlist(None) == 0 and lib.lb_gpu_ivfpq_ntotal(None) == 0 and lib.lb_gpu_ivfpq_hbm_bytes(None) == 0
    assert lib.lb_gpu_ivfpq_last_error(None) == b"null handle"
    lib.lb_gpu_ivfpq_free(None)


def test_python_front_end_fails_loudly_without_a_gpu(lib):
    from longbow_amd import _lib, ivfpq
    import longbow_amd
    assert "ivfpq" in longbow_amd.__all__
    device = 1 << 20 if lib.lb_gpu_device_count() > 0 else 0  # (a device that is not there, on a GPU box too)
    with pytest.raises(_lib.GPUNotAvailable):
        ivfpq.IVFPQ(_blob(8, 2), np.zeros((4, 8), np.float32), device=device)
    with pytest.raises(_lib.GPUNotAvailable):
        ivfpq.train(np.zeros((600, 8), np.float32), 4, 2, device=device)
    with pytest.raises(ValueError):
        ivfpq.IVFPQ(_blob(8, 2), np.zeros((0, 8), np.float32), device=device)
    with pytest.raises(ValueError, match="dimensions"):
        ivfpq.IVFPQ(_blob(8, 2), np.zeros((4, 16), np.float32), device=device)
