"""lb_gpu_ivfsq8_*: every symbol is exported, every argument check that needs no handle answers before a device is touched, in
the order include/longbow_gpu.h states (INVALID_ARG, UNSUPPORTED, NO_DEVICE), and a refused call leaves its output buffers
untouched, so all of this runs on a box without a GPU.  (A handle exists only where a device does: the checks behind a live
handle, k above LB_MAX_K and nprobe <= 0 among them, are in tests/test_gpu_ivfsq8.py.)"""
import ctypes as C

import numpy as np
import pytest

INVALID, NO_DEVICE, UNSUPPORTED = 1, 3, 6
LB_MAX_DIM, LB_MAX_K, MAX_NLIST = 8192, 2048, 65536

SYMBOLS = ("new", "free", "last_error", "dims", "order", "nlist", "ntotal", "hbm_bytes", "get_bounds", "get_centroids", "reserve",
           "add", "add_device", "get_codes", "list_sizes", "assignments", "search", "search_ctx", "search_device_ctx", "set_filter",
           "filter_int64", "filter_float32", "nvisible", "last_search_stats", "set_profiling", "last_timing", "last_build_timing")


@pytest.fixture(scope="module")
def lib():
    from longbow_amd import _lib
    return _lib.load()


def test_every_symbol_is_exported(lib):
    for name in SYMBOLS:
        assert getattr(lib, "lb_gpu_ivfsq8_" + name) is not None, name


def _new(lib, dims=16, order=0, nlist=4, device=0, mn=0.0, mx=1.0, null=(), bad_dim=None, bad=(1.0, 1.0)):
    """on a GPU box `device` is moved out of range so that nothing is ever created.  bad_dim: the one dimension that gets the
    bounds `bad`"""
    if lib.lb_gpu_device_count() > 0 and device >= 0:
        device = 1 << 20
    room = max(dims, 1)
    lo, hi = np.full(room, mn, np.float32), np.full(room, mx, np.float32)
    if bad_dim is not None:
        lo[bad_dim], hi[bad_dim] = bad
    c = np.zeros(64, np.float32)  # (never read: every call here is refused first)
    st = C.c_int(-1)
    h = lib.lb_gpu_ivfsq8_new(device, dims, None if "min" in null else lo.ctypes.data, None if "max" in null else hi.ctypes.data, order,
                              nlist, None if "centroids" in null else c.ctypes.data, C.byref(st))
    assert not h
    return st.value


def test_new_checks_its_arguments_in_the_documented_order(lib):
    nan = float("nan")
    assert _new(lib, dims=0) == INVALID
    assert _new(lib, dims=-5) == INVALID
    assert _new(lib, null=("min",)) == INVALID
    assert _new(lib, null=("max",)) == INVALID
    assert _new(lib, null=("centroids",)) == INVALID
    assert _new(lib, order=2) == INVALID
    assert _new(lib, order=-1) == INVALID
    assert _new(lib, nlist=0) == INVALID
    assert _new(lib, nlist=-3) == INVALID
    for d in (0, 7, 15):                                              # min >= max in one dimension (SQ8Config.Validate)
        assert _new(lib, bad_dim=d) == INVALID                        # min == max
        assert _new(lib, bad_dim=d, bad=(2.0, 1.0)) == INVALID        # min > max
    assert _new(lib, nlist=0, device=-1) == INVALID                   # INVALID_ARG before NO_DEVICE
    assert _new(lib, bad_dim=3, device=-1) == INVALID
    assert _new(lib, dims=LB_MAX_DIM + 1, nlist=0) == INVALID         # INVALID_ARG before UNSUPPORTED
    assert _new(lib, dims=LB_MAX_DIM + 1, bad_dim=LB_MAX_DIM) == INVALID
    assert _new(lib, nlist=MAX_NLIST + 1, bad_dim=0) == INVALID
    assert _new(lib, dims=LB_MAX_DIM + 1) == UNSUPPORTED
    assert _new(lib, nlist=MAX_NLIST + 1) == UNSUPPORTED
    assert _new(lib, dims=LB_MAX_DIM + 1, device=-1) == UNSUPPORTED   # UNSUPPORTED before NO_DEVICE
    assert _new(lib, nlist=MAX_NLIST + 1, device=-1) == UNSUPPORTED
    for dims in (1, 16, 20, 768, LB_MAX_DIM):
        for order in (0, 1):
            for nlist in (1, 7, MAX_NLIST):
                assert _new(lib, dims=dims, order=order, nlist=nlist) == NO_DEVICE
    # NaN bounds pass the validation, as on lb_gpu_sq8_set_bounds: neither comparison holds
    assert _new(lib, bad_dim=2, bad=(nan, 1.0)) == NO_DEVICE
    assert _new(lib, bad_dim=2, bad=(0.0, nan)) == NO_DEVICE
    assert _new(lib, mn=nan, mx=nan) == NO_DEVICE
    assert _new(lib, device=-1) == NO_DEVICE
    # out_status is nullable
    c = np.zeros(64, np.float32)
    lo, hi = np.zeros(16, np.float32), np.ones(16, np.float32)
    assert not lib.lb_gpu_ivfsq8_new(-1, 16, lo.ctypes.data, hi.ctypes.data, 0, 4, c.ctypes.data, None)
    assert not lib.lb_gpu_ivfsq8_new(0, 16, None, hi.ctypes.data, 0, 4, c.ctypes.data, None)
    assert not lib.lb_gpu_ivfsq8_new(0, 16, hi.ctypes.data, lo.ctypes.data, 0, 4, c.ctypes.data, None)


def test_null_handle_is_refused_everywhere_and_nothing_is_written(lib):
    dim, n, k = 20, 3, 4
    vec = np.full((n, dim), 7.0, np.float32)
    ids = np.full(n, 55, np.int64)
    f32 = np.full(n * k, 9.0, np.float32)
    i64 = np.full(n * k, 77, np.int64)
    i32 = np.full(n, 0x5A5A5A5A, np.int32)
    u8 = np.full(n * dim, 0xA5, np.uint8)
    sizes = np.full(8, 31, np.int64)
    lo, hi = np.full(dim, 4.0, np.float32), np.full(dim, 6.0, np.float32)
    stats = (C.c_int64 * 4)(5, 5, 5, 5)
    ms = (C.c_float * 5)(2, 2, 2, 2, 2)
    one = C.c_float(2)
    v = vec.ctypes.data
    for kk in (k, 0, -1, LB_MAX_K, LB_MAX_K + 1):  # INVALID_ARG comes before UNSUPPORTED: no handle and k too large -> invalid
        for nn in (n, 0, -1):
            for nprobe in (1, 0, -1):
                assert lib.lb_gpu_ivfsq8_search(None, nn, v, kk, nprobe, f32.ctypes.data, i64.ctypes.data) == INVALID
                assert lib.lb_gpu_ivfsq8_search_ctx(None, nn, v, kk, nprobe, f32.ctypes.data, i64.ctypes.data, None) == INVALID
                assert lib.lb_gpu_ivfsq8_search_device_ctx(None, nn, v, kk, nprobe, f32.ctypes.data, i64.ctypes.data, None, None) == INVALID
    for nn in (n, 0, -1):
        assert lib.lb_gpu_ivfsq8_add(None, nn, v, None) == INVALID
        assert lib.lb_gpu_ivfsq8_add(None, nn, v, ids.ctypes.data) == INVALID
        assert lib.lb_gpu_ivfsq8_add_device(None, nn, v, None) == INVALID
        assert lib.lb_gpu_ivfsq8_assignments(None, 0, nn, i32.ctypes.data) == INVALID
        assert lib.lb_gpu_ivfsq8_get_codes(None, 0, nn, u8.ctypes.data) == INVALID
        assert lib.lb_gpu_ivfsq8_reserve(None, nn) == INVALID
        assert lib.lb_gpu_ivfsq8_set_filter(None, u8.ctypes.data, nn) == INVALID
        assert lib.lb_gpu_ivfsq8_filter_int64(None, ids.ctypes.data, nn, 0, 0, None, 0, 0) == INVALID
        assert lib.lb_gpu_ivfsq8_filter_float32(None, v, nn, 0.0, 0, None, 0, 0) == INVALID
    assert lib.lb_gpu_ivfsq8_list_sizes(None, sizes.ctypes.data) == INVALID
    assert lib.lb_gpu_ivfsq8_get_centroids(None, v) == INVALID
    assert lib.lb_gpu_ivfsq8_get_bounds(None, lo.ctypes.data, hi.ctypes.data) == INVALID
    assert lib.lb_gpu_ivfsq8_last_search_stats(None, stats) == INVALID
    assert lib.lb_gpu_ivfsq8_set_profiling(None, 1) == INVALID
    assert lib.lb_gpu_ivfsq8_last_timing(None, ms) == INVALID
    assert lib.lb_gpu_ivfsq8_last_build_timing(None, C.byref(one)) == INVALID
    assert (vec == 7.0).all() and (ids == 55).all() and (f32 == 9.0).all() and (i64 == 77).all() and (i32 == 0x5A5A5A5A).all()
    assert (u8 == 0xA5).all() and (sizes == 31).all() and list(stats) == [5, 5, 5, 5] and list(ms) == [2, 2, 2, 2, 2]
    assert (lo == 4.0).all() and (hi == 6.0).all() and one.value == 2
    # the accessors of no handle
    assert lib.lb_gpu_ivfsq8_dims(None) == 0 and lib.lb_gpu_ivfsq8_order(None) == 0 and lib.lb_gpu_ivfsq8_nlist(None) == 0
    assert lib.lb_gpu_ivfsq8_ntotal(None) == 0 and lib.lb_gpu_ivfsq8_hbm_bytes(None) == 0
    assert lib.lb_gpu_ivfsq8_nvisible(None) == lib.lb_gpu_ivfpq_nvisible(None)
    assert lib.lb_gpu_ivfsq8_last_error(None) == b"null handle"
    lib.lb_gpu_ivfsq8_free(None)


def test_python_front_end_fails_loudly_without_a_gpu(lib):
    from longbow_amd import _lib, ivfsq8
    import longbow_amd
    assert "ivfsq8" in longbow_amd.__all__
    device = 1 << 20 if lib.lb_gpu_device_count() > 0 else 0  # (a device that is not there, on a GPU box too)
    lo, hi = np.zeros(8, np.float32), np.ones(8, np.float32)
    with pytest.raises(_lib.GPUNotAvailable):
        ivfsq8.IVFSQ8(lo, hi, np.zeros((4, 8), np.float32), device=device)
    with pytest.raises(_lib.GPUNotAvailable):
        ivfsq8.train(np.zeros((600, 8), np.float32), 4, device=device)
    with pytest.raises(ValueError):
        ivfsq8.IVFSQ8(lo, hi, np.zeros((0, 8), np.float32), device=device)
    with pytest.raises(ValueError, match="dimensions"):
        ivfsq8.IVFSQ8(lo, hi, np.zeros((4, 16), np.float32), device=device)
    with pytest.raises(ValueError, match="same length"):
        ivfsq8.IVFSQ8(lo, hi[:7], np.zeros((4, 8), np.float32), device=device)
