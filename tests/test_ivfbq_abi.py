"""lb_gpu_ivfbq_*: every symbol is exported, every argument check that needs no handle answers before a device is touched, in
the order include/longbow_gpu.h states (INVALID_ARG, UNSUPPORTED, NO_DEVICE), and a refused call leaves its output buffers
untouched, so all of this runs on a box without a GPU.  (A handle exists only where a device does: the checks behind a live
handle, k above LB_MAX_K and nprobe <= 0 among them, are in tests/test_gpu_ivfbq.py.)"""
import ctypes as C

import numpy as np
import pytest

INVALID, NO_DEVICE, UNSUPPORTED = 1, 3, 6
LB_MAX_DIM, LB_MAX_K, MAX_NLIST = 8192, 2048, 65536

SYMBOLS = ("new", "free", "last_error", "dims", "words", "order", "nlist", "ntotal", "hbm_bytes", "get_centroids", "reserve", "add",
           "add_device", "get_codes", "list_sizes", "assignments", "search", "search_ctx", "search_device_ctx", "set_filter",
           "filter_int64", "filter_float32", "nvisible", "last_search_stats", "set_profiling", "last_timing", "last_build_timing")


@pytest.fixture(scope="module")
def lib():
    from longbow_amd import _lib
    return _lib.load()


def test_every_symbol_is_exported(lib):
    for name in SYMBOLS:
        assert getattr(lib, "lb_gpu_ivfbq_" + name) is not None, name


def test_the_header_declares_what_the_library_exports():
    import os
    import re
    from longbow_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "longbow_gpu.h")) as f:
        declared = set(re.findall(r"\b(lb_gpu_ivfbq_\w+)\s*\(", f.read()))
    assert declared == {"lb_gpu_ivfbq_" + s for s in SYMBOLS}
    assert {name for name, _, _ in _lib.SIGNATURES if name.startswith("lb_gpu_ivfbq_")} == declared


def _new(lib, dims=16, order=0, nlist=4, device=0, null=False):
    """on a GPU box `device` is moved out of range so that nothing is ever created"""
    if lib.lb_gpu_device_count() > 0 and device >= 0:
        device = 1 << 20
    c = np.zeros(64, np.float32)  # (never read: every call here is refused first)
    st = C.c_int(-1)
    h = lib.lb_gpu_ivfbq_new(device, dims, order, nlist, None if null else c.ctypes.data, C.byref(st))
    assert not h
    return st.value


def test_new_checks_its_arguments_in_the_documented_order(lib):
    assert _new(lib, dims=0) == INVALID
    assert _new(lib, dims=-5) == INVALID
    assert _new(lib, null=True) == INVALID
    assert _new(lib, order=2) == INVALID
    assert _new(lib, order=-1) == INVALID
    assert _new(lib, nlist=0) == INVALID
    assert _new(lib, nlist=-3) == INVALID
    assert _new(lib, nlist=0, device=-1) == INVALID                   # INVALID_ARG before NO_DEVICE
    assert _new(lib, null=True, device=-1) == INVALID
    assert _new(lib, dims=LB_MAX_DIM + 1, nlist=0) == INVALID         # INVALID_ARG before UNSUPPORTED
    assert _new(lib, dims=LB_MAX_DIM + 1, null=True) == INVALID
    assert _new(lib, dims=LB_MAX_DIM + 1, order=2) == INVALID
    assert _new(lib, nlist=MAX_NLIST + 1, order=-1) == INVALID
    assert _new(lib, nlist=MAX_NLIST + 1, dims=0) == INVALID
    assert _new(lib, dims=LB_MAX_DIM + 1) == UNSUPPORTED
    assert _new(lib, nlist=MAX_NLIST + 1) == UNSUPPORTED
    assert _new(lib, dims=LB_MAX_DIM + 1, device=-1) == UNSUPPORTED   # UNSUPPORTED before NO_DEVICE
    assert _new(lib, nlist=MAX_NLIST + 1, device=-1) == UNSUPPORTED
    for dims in (1, 16, 100, 768, 1088, LB_MAX_DIM):
        for order in (0, 1):
            for nlist in (1, 7, MAX_NLIST):
                assert _new(lib, dims=dims, order=order, nlist=nlist) == NO_DEVICE   # an out-of-range device on a GPU box
    assert _new(lib, device=-1) == NO_DEVICE
    # out_status is nullable
    c = np.zeros(64, np.float32)
    assert not lib.lb_gpu_ivfbq_new(-1, 16, 0, 4, c.ctypes.data, None)
    assert not lib.lb_gpu_ivfbq_new(0, 16, 0, 4, None, None)
    assert not lib.lb_gpu_ivfbq_new(0, 0, 0, 4, c.ctypes.data, None)


def test_null_handle_is_refused_everywhere_and_nothing_is_written(lib):
    dim, n, k = 100, 3, 4
    vec = np.full((n, dim), 7.0, np.float32)
    ids = np.full(n, 55, np.int64)
    f32 = np.full(n * k, 9.0, np.float32)
    i64 = np.full(n * k, 77, np.int64)
    i32 = np.full(n, 0x5A5A5A5A, np.int32)
    u64 = np.full(n * 2, 0xA5A5A5A5A5A5A5A5, np.uint64)
    u8 = np.full(n, 0xA5, np.uint8)
    sizes = np.full(8, 31, np.int64)
    stats = (C.c_int64 * 4)(5, 5, 5, 5)
    ms = (C.c_float * 5)(2, 2, 2, 2, 2)
    one = C.c_float(2)
    v = vec.ctypes.data
    for kk in (k, 0, -1, LB_MAX_K, LB_MAX_K + 1):  # INVALID_ARG comes before UNSUPPORTED: no handle and k too large -> invalid
        for nn in (n, 0, -1):
            for nprobe in (1, 0, -1):
                assert lib.lb_gpu_ivfbq_search(None, nn, v, kk, nprobe, f32.ctypes.data, i64.ctypes.data) == INVALID
                assert lib.lb_gpu_ivfbq_search_ctx(None, nn, v, kk, nprobe, f32.ctypes.data, i64.ctypes.data, None) == INVALID
                assert lib.lb_gpu_ivfbq_search_device_ctx(None, nn, v, kk, nprobe, f32.ctypes.data, i64.ctypes.data, None, None) == INVALID
    for nn in (n, 0, -1):
        assert lib.lb_gpu_ivfbq_add(None, nn, v, None) == INVALID
        assert lib.lb_gpu_ivfbq_add(None, nn, v, ids.ctypes.data) == INVALID
        assert lib.lb_gpu_ivfbq_add_device(None, nn, v, None) == INVALID
        assert lib.lb_gpu_ivfbq_assignments(None, 0, nn, i32.ctypes.data) == INVALID
        assert lib.lb_gpu_ivfbq_get_codes(None, 0, nn, u64.ctypes.data) == INVALID
        assert lib.lb_gpu_ivfbq_reserve(None, nn) == INVALID
        assert lib.lb_gpu_ivfbq_set_filter(None, u8.ctypes.data, nn) == INVALID
        assert lib.lb_gpu_ivfbq_filter_int64(None, ids.ctypes.data, nn, 0, 0, None, 0, 0) == INVALID
        assert lib.lb_gpu_ivfbq_filter_float32(None, v, nn, 0.0, 0, None, 0, 0) == INVALID
    assert lib.lb_gpu_ivfbq_list_sizes(None, sizes.ctypes.data) == INVALID
    assert lib.lb_gpu_ivfbq_get_centroids(None, v) == INVALID
    assert lib.lb_gpu_ivfbq_last_search_stats(None, stats) == INVALID
    assert lib.lb_gpu_ivfbq_set_profiling(None, 1) == INVALID
    assert lib.lb_gpu_ivfbq_last_timing(None, ms) == INVALID
    assert lib.lb_gpu_ivfbq_last_build_timing(None, C.byref(one)) == INVALID
    # a refused search leaves its output buffers untouched, and so does every other refused call
    assert (vec == 7.0).all() and (ids == 55).all() and (f32 == 9.0).all() and (i64 == 77).all() and (i32 == 0x5A5A5A5A).all()
    assert (u64 == 0xA5A5A5A5A5A5A5A5).all() and (u8 == 0xA5).all() and (sizes == 31).all()
    assert list(stats) == [5, 5, 5, 5] and list(ms) == [2, 2, 2, 2, 2] and one.value == 2
    # the accessors of no handle
    assert lib.lb_gpu_ivfbq_dims(None) == 0 and lib.lb_gpu_ivfbq_words(None) == 0 and lib.lb_gpu_ivfbq_order(None) == 0
    assert lib.lb_gpu_ivfbq_nlist(None) == 0 and lib.lb_gpu_ivfbq_ntotal(None) == 0 and lib.lb_gpu_ivfbq_hbm_bytes(None) == 0
    assert lib.lb_gpu_ivfbq_nvisible(None) == lib.lb_gpu_ivfsq8_nvisible(None)
    assert lib.lb_gpu_ivfbq_last_error(None) == b"null handle"
    lib.lb_gpu_ivfbq_free(None)


def test_python_front_end_fails_loudly_without_a_gpu(lib):
    from longbow_amd import _lib, ivf, ivfbq
    import longbow_amd
    assert "ivfbq" in longbow_amd.__all__
    assert ivfbq.train is ivf.train
    device = 1 << 20 if lib.lb_gpu_device_count() > 0 else 0  # (a device that is not there, on a GPU box too)
    with pytest.raises(_lib.GPUNotAvailable):
        ivfbq.IVFBQ(np.zeros((4, 8), np.float32), device=device)
    with pytest.raises(ValueError):
        ivfbq.IVFBQ(np.zeros((0, 8), np.float32), device=device)
    with pytest.raises(ValueError):
        ivfbq.IVFBQ(np.zeros(8, np.float32), device=device)
