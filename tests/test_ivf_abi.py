"""lb_gpu_ivf_*: every argument check that needs no handle answers before a device is touched, in the order
include/longbow_gpu.h states (INVALID_ARG, UNSUPPORTED, NO_DEVICE), and a refused call leaves its output buffers untouched, so
all of this runs on a box without a GPU.  (A handle exists only where a device does: the checks behind a live handle, k above
LB_MAX_K and nprobe <= 0 among them, are in tests/test_gpu_ivf.py.)"""
import ctypes as C

import numpy as np
import pytest

INVALID, NO_DEVICE, UNSUPPORTED = 1, 3, 6
LB_MAX_DIM, LB_MAX_K, MAX_NLIST = 8192, 2048, 65536


@pytest.fixture(scope="module")
def lib():
    from longbow_amd import _lib
    return _lib.load()


def _new(lib, dim, metric=0, order=0, nlist=4, device=0, cent=True):
    """on a GPU box `device` is moved out of range so that nothing is ever created"""
    if lib.lb_gpu_device_count() > 0 and device >= 0:
        device = 1 << 20
    c = np.zeros(max(1, min(nlist, 8)) * max(1, min(dim, 8)), np.float32)  # (never read: every call here is refused first)
    st = C.c_int(-1)
    h = lib.lb_gpu_ivf_new(device, dim, metric, order, nlist, c.ctypes.data if cent else None, C.byref(st))
    assert not h
    return st.value


def test_new_checks_its_arguments_in_the_documented_order(lib):
    assert _new(lib, 0) == INVALID
    assert _new(lib, -1) == INVALID
    assert _new(lib, 16, metric=3) == INVALID
    assert _new(lib, 16, metric=-1) == INVALID
    assert _new(lib, 16, order=2) == INVALID
    assert _new(lib, 16, order=-1) == INVALID
    assert _new(lib, 16, nlist=0) == INVALID
    assert _new(lib, 16, nlist=-3) == INVALID
    assert _new(lib, 16, cent=False) == INVALID
    assert _new(lib, 0, device=-1) == INVALID                         # INVALID_ARG before NO_DEVICE
    assert _new(lib, LB_MAX_DIM + 1, nlist=0) == INVALID              # INVALID_ARG before UNSUPPORTED
    assert _new(lib, LB_MAX_DIM + 1) == UNSUPPORTED
    assert _new(lib, 16, nlist=MAX_NLIST + 1) == UNSUPPORTED
    assert _new(lib, LB_MAX_DIM + 1, device=-1) == UNSUPPORTED        # UNSUPPORTED before NO_DEVICE
    for dim, nlist in ((1, 1), (3, 7), (768, 256)):
        for metric in (0, 1, 2):
            for order in (0, 1):
                c = np.zeros((nlist, dim), np.float32)
                device = 1 << 20 if lib.lb_gpu_device_count() > 0 else 0
                st = C.c_int(-1)
                assert not lib.lb_gpu_ivf_new(device, dim, metric, order, nlist, c.ctypes.data, C.byref(st))
                assert st.value == NO_DEVICE
    c = np.zeros((4, 16), np.float32)
    st = C.c_int(-1)
    assert not lib.lb_gpu_ivf_new(-1, 16, 0, 0, 4, c.ctypes.data, C.byref(st)) and st.value == NO_DEVICE
    # out_status is nullable
    assert not lib.lb_gpu_ivf_new(-1, 16, 0, 0, 4, c.ctypes.data, None) and not lib.lb_gpu_ivf_new(0, 0, 0, 0, 4, c.ctypes.data, None)


def test_null_handle_is_refused_everywhere_and_nothing_is_written(lib):
    dim, n, k = 20, 3, 4
    vec = np.full((n, dim), 7.0, np.float32)
    ids = np.full(n, 55, np.int64)
    f32 = np.full(n * k, 9.0, np.float32)
    i64 = np.full(n * k, 77, np.int64)
    i32 = np.full(n, 0x5A5A5A5A, np.int32)
    sizes = np.full(8, 31, np.int64)
    stats = (C.c_int64 * 4)(5, 5, 5, 5)
    v = vec.ctypes.data
    for kk in (k, 0, -1, LB_MAX_K, LB_MAX_K + 1):  # INVALID_ARG comes before UNSUPPORTED: no handle and k too large -> invalid
        for nn in (n, 0, -1):
            for nprobe in (1, 0, -1):
                assert lib.lb_gpu_ivf_search(None, nn, v, kk, nprobe, f32.ctypes.data, i64.ctypes.data) == INVALID
                assert lib.lb_gpu_ivf_search_ctx(None, nn, v, kk, nprobe, f32.ctypes.data, i64.ctypes.data, None) == INVALID
                assert lib.lb_gpu_ivf_search_device_ctx(None, nn, v, kk, nprobe, f32.ctypes.data, i64.ctypes.data, None, None) == INVALID
    for nn in (n, 0, -1):
        assert lib.lb_gpu_ivf_add(None, nn, v, None) == INVALID
        assert lib.lb_gpu_ivf_add(None, nn, v, ids.ctypes.data) == INVALID
        assert lib.lb_gpu_ivf_add_device(None, nn, v, None) == INVALID
        assert lib.lb_gpu_ivf_assignments(None, 0, nn, i32.ctypes.data) == INVALID
        assert lib.lb_gpu_ivf_reserve(None, nn) == INVALID
    assert lib.lb_gpu_ivf_list_sizes(None, sizes.ctypes.data) == INVALID
    assert lib.lb_gpu_ivf_get_centroids(None, v) == INVALID
    assert lib.lb_gpu_ivf_last_search_stats(None, stats) == INVALID
    assert (vec == 7.0).all() and (ids == 55).all() and (f32 == 9.0).all() and (i64 == 77).all() and (i32 == 0x5A5A5A5A).all()
    assert (sizes == 31).all() and list(stats) == [5, 5, 5, 5]
    # the accessors of no handle
    assert lib.lb_gpu_ivf_dim(None) == 0 and lib.lb_gpu_ivf_metric(None) == 0 and lib.lb_gpu_ivf_order(None) == 0
    assert lib.lb_gpu_ivf_nlist(None) == 0 and lib.lb_gpu_ivf_ntotal(None) == 0 and lib.lb_gpu_ivf_hbm_bytes(None) == 0
    assert lib.lb_gpu_ivf_last_error(None) == b"null handle"
    lib.lb_gpu_ivf_free(None)


def test_python_front_end_fails_loudly_without_a_gpu(lib):
    from longbow_amd import _lib, ivf
    import longbow_amd
    assert "ivf" in longbow_amd.__all__
    device = 1 << 20 if lib.lb_gpu_device_count() > 0 else 0  # (a device that is not there, on a GPU box too)
    with pytest.raises(_lib.GPUNotAvailable):
        ivf.IVFFlat(np.zeros((4, 8), np.float32), device=device)
    with pytest.raises(_lib.GPUNotAvailable):
        ivf.IVFFlatIndex(8, ivf.IVFFlatConfig(NClusters=4, NProbe=2), device=device)
    with pytest.raises(_lib.GPUNotAvailable):
        ivf.train(np.zeros((16, 8), np.float32), 4, device=device)
    with pytest.raises(ValueError):
        ivf.IVFFlat(np.zeros((0, 8), np.float32), device=device)
    with pytest.raises(ValueError):
        ivf.IVFFlatIndex(0, device=device)
    with pytest.raises(ValueError, match="256"):
        ivf.train(np.zeros((600, 8), np.float32), 257, device=device)
    with pytest.raises(ValueError, match="empty"):
        ivf.train(np.zeros((0, 8), np.float32), 4, device=device)
    cfg = ivf.IVFFlatConfig()
    assert (cfg.NClusters, cfg.NProbe) == (256, 8)
