"""lb_gpu_ivfpq4_* without a device, in the style of tests/test_ivfpq_abi.py: every name of the family is bound with argtypes, both
constructors refuse in the order include/longbow_gpu.h states (INVALID_ARG, UNSUPPORTED, NO_DEVICE) before a device is touched,
and calls on no handle answer INVALID_ARG, 0 or "null handle" and write nothing."""
import ctypes as C
import struct

import numpy as np
import pytest

INVALID, NO_DEVICE, UNSUPPORTED = 1, 3, 6
LB_MAX_DIM, LB_MAX_K, MAX_NLIST, PQ4_MAX_M = 8192, 2048, 65536, 1024


@pytest.fixture(scope="module")
def lib():
    from longbow_amd import _lib
    return _lib.load()


def _blob(dims=16, M=4, K=16, extra=0):
    return struct.pack("<III", dims, M, K) + bytes(M * K * (dims // M if M else 0) * 4 + extra)


def _new_both(lib, blob=None, order=0, nlist=4, device=0, cent=True, length=None, null_blob=False):
    """the status of both constructors for one refused argument set (on a GPU box `device` is moved out of range so that
    nothing is ever created); they must agree"""
    if lib.lb_gpu_device_count() > 0 and device >= 0:
        device = 1 << 20
    blob = _blob() if blob is None else blob
    c = np.zeros(64, np.float32)  # (never read: every call here is refused first)
    got = []
    for new in (lib.lb_gpu_ivfpq4_new, lib.lb_gpu_ivfpq4_new_residual):
        st = C.c_int(-1)
        h = new(device, None if null_blob else blob, len(blob) if length is None else length, order, nlist,
                c.ctypes.data if cent else None, C.byref(st))
        assert not h
        got.append(st.value)
    assert got[0] == got[1], got
    return got[1]


def test_every_name_of_the_family_is_bound_with_argtypes(lib):
    """the K = 256 family name for name, with its signatures: the library exports each and ctypes knows its arguments"""
    from longbow_amd import _lib
    bound = {name: (res, args) for name, res, args in _lib.SIGNATURES if name.startswith("lb_gpu_ivfpq4_")}
    k256 = {name.replace("ivfpq_", "ivfpq4_"): (res, args) for name, res, args in _lib.SIGNATURES if name.startswith("lb_gpu_ivfpq_")}
    assert len(bound) == 37 and bound == k256
    for name, (res, args) in bound.items():
        fn = getattr(lib, name)
        assert fn.argtypes == args and fn.restype == res, name


def test_constructors_check_their_arguments_in_the_documented_order(lib):
    assert _new_both(lib, null_blob=True) == INVALID
    assert _new_both(lib, length=8) == INVALID                              # too short for the header
    assert _new_both(lib, _blob(extra=4)) == INVALID                        # size mismatch
    assert _new_both(lib, _blob()[:-4]) == INVALID
    assert _new_both(lib, _blob(dims=18, M=4)) == INVALID                   # dims % M != 0
    assert _new_both(lib, struct.pack("<III", 16, 0, 16)) == INVALID        # M == 0
    assert _new_both(lib, order=2) == INVALID
    assert _new_both(lib, order=-1) == INVALID
    assert _new_both(lib, nlist=0) == INVALID
    assert _new_both(lib, nlist=-3) == INVALID
    assert _new_both(lib, cent=False) == INVALID
    assert _new_both(lib, nlist=0, device=-1) == INVALID                    # INVALID_ARG before NO_DEVICE
    assert _new_both(lib, _blob(K=256), nlist=0) == INVALID                 # INVALID_ARG before UNSUPPORTED
    assert _new_both(lib, _blob(K=256)) == UNSUPPORTED                      # a well-formed blob of another K
    assert _new_both(lib, _blob(K=15)) == UNSUPPORTED
    assert _new_both(lib, _blob(dims=PQ4_MAX_M + 1, M=PQ4_MAX_M + 1)) == UNSUPPORTED
    assert _new_both(lib, _blob(dims=LB_MAX_DIM + 1, M=1)) == UNSUPPORTED   # dims > LB_MAX_DIM
    assert _new_both(lib, nlist=MAX_NLIST + 1) == UNSUPPORTED
    assert _new_both(lib, _blob(K=256), device=-1) == UNSUPPORTED           # UNSUPPORTED before NO_DEVICE
    for dims, M in ((16, 4), (6, 3), (768, 96), (PQ4_MAX_M, PQ4_MAX_M), (4, 1)):
        for order in (0, 1):
            for nlist in (1, 7, MAX_NLIST):
                assert _new_both(lib, _blob(dims, M), order=order, nlist=nlist) == NO_DEVICE
    assert _new_both(lib, device=-1) == NO_DEVICE
    c = np.zeros(64, np.float32)  # out_status is nullable
    b = _blob()
    assert not lib.lb_gpu_ivfpq4_new(-1, b, len(b), 0, 4, c.ctypes.data, None)
    assert not lib.lb_gpu_ivfpq4_new_residual(0, None, 0, 0, 4, c.ctypes.data, None)


def test_null_handle_is_refused_everywhere_and_nothing_is_written(lib):
    n, k = 3, 4
    vec = np.full((n, 20), 7.0, np.float32)
    i64 = np.full(n * k, 77, np.int64)
    f32 = np.full(n * k, 9.0, np.float32)
    u8 = np.full(n * 8, 0xA5, np.uint8)
    stats = (C.c_int64 * 4)(5, 5, 5, 5)
    ms = (C.c_float * 5)(2, 2, 2, 2, 2)
    got = C.c_int64(-9)
    v, d, l, b = vec.ctypes.data, f32.ctypes.data, i64.ctypes.data, u8.ctypes.data
    L = lambda name: getattr(lib, "lb_gpu_ivfpq4_" + name)
    for kk in (k, 0, LB_MAX_K + 1):  # INVALID_ARG comes before UNSUPPORTED: no handle and k too large -> invalid
        for nprobe in (1, 0):
            assert L("search")(None, n, v, kk, nprobe, d, l) == INVALID
            assert L("search_ctx")(None, n, v, kk, nprobe, d, l, None) == INVALID
            assert L("search_device_ctx")(None, n, v, kk, nprobe, d, l, None, None) == INVALID
            assert L("search_bitmap_ctx")(None, n, v, kk, nprobe, b, n, 0, d, l, None) == INVALID
            assert L("search_bitmap_device_ctx")(None, n, v, kk, nprobe, b, n, 0, d, l, None, None) == INVALID
    for nn in (n, 0, -1):
        assert L("add")(None, nn, v, l) == INVALID and L("add_device")(None, nn, v, None) == INVALID
        assert L("assignments")(None, 0, nn, l) == INVALID and L("get_codes")(None, 0, nn, b) == INVALID
        assert L("reserve")(None, nn) == INVALID and L("set_filter")(None, b, nn) == INVALID
        assert L("filter_int64")(None, l, nn, 0, 0, None, 0, 0) == INVALID and L("filter_float32")(None, d, nn, 0.0, 0, None, 0, 0) == INVALID
        for remove in ("remove", "remove_device", "remove_rows"):
            assert L(remove)(None, nn, l, C.byref(got)) == INVALID
    assert L("list_sizes")(None, l) == INVALID and L("get_centroids")(None, v) == INVALID and L("compact")(None, l, n) == INVALID
    assert L("last_search_stats")(None, stats) == INVALID and L("set_profiling")(None, 1) == INVALID
    assert L("last_timing")(None, ms) == INVALID and L("last_build_timing")(None, ms) == INVALID
    assert (vec == 7.0).all() and (f32 == 9.0).all() and (i64 == 77).all() and (u8 == 0xA5).all()
    assert list(stats) == [5, 5, 5, 5] and list(ms) == [2, 2, 2, 2, 2] and got.value == -9
    for name in ("dims", "m", "order", "nlist", "ntotal", "hbm_bytes", "residual", "nvisible", "nlive", "ndeleted"):
        assert L(name)(None) == 0, name
    assert L("last_error")(None) == b"null handle"
    L("free")(None)


def test_python_front_end_fails_loudly_without_a_gpu(lib):
    from longbow_amd import _lib, ivfpq4
    import longbow_amd
    assert "ivfpq4" in longbow_amd.__all__
    device = 1 << 20 if lib.lb_gpu_device_count() > 0 else 0  # (a device that is not there, on a GPU box too)
    for residual in (False, True):
        with pytest.raises(_lib.GPUNotAvailable):
            ivfpq4.IVFPQ4(_blob(8, 2), np.zeros((4, 8), np.float32), device=device, residual=residual)
        with pytest.raises(_lib.GPUNotAvailable):
            ivfpq4.train(np.zeros((600, 8), np.float32), 4, 2, device=device, residual=residual)
    with pytest.raises(ValueError):
        ivfpq4.IVFPQ4(_blob(8, 2), np.zeros((0, 8), np.float32), device=device)
    with pytest.raises(ValueError, match="dimensions"):
        ivfpq4.IVFPQ4(_blob(8, 2), np.zeros((4, 16), np.float32), device=device)
