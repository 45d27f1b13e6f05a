"""lb_gpu_ivf_new_i8 / _add_i8 / _add_i8_device / _search_i8 / _search_i8_ctx / _search_i8_device_ctx: the argument checks that
need no handle answer before a device is touched, in lb_gpu_ivf_new's documented order (INVALID_ARG, UNSUPPORTED, NO_DEVICE), and
a refused call writes nothing, so all of this runs on a box without a GPU, as tests/test_ivf_f16_abi.py does for the float16 entry
points.  The checks behind a live handle are in tests/test_gpu_ivf_i8.py."""
import ctypes as C

import numpy as np
import pytest

INVALID, NO_DEVICE, UNSUPPORTED = 1, 3, 6
LB_MAX_DIM, MAX_NLIST = 8192, 65536


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
    h = lib.lb_gpu_ivf_new_i8(device, dim, metric, order, nlist, c.ctypes.data if cent else None, C.byref(st))
    assert not h
    return st.value


def test_new_i8_checks_its_arguments_in_the_documented_order(lib):
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
    assert _new(lib, 16, metric=1, nlist=0) == INVALID
    assert _new(lib, 4100, metric=2, order=2) == INVALID
    assert _new(lib, LB_MAX_DIM + 1) == UNSUPPORTED
    assert _new(lib, 16, nlist=MAX_NLIST + 1) == UNSUPPORTED
    assert _new(lib, 16, metric=1) == UNSUPPORTED                     # no int8 cosine kernel in the reference
    assert _new(lib, 4100, metric=2) == UNSUPPORTED                   # 1025 + 0 chain steps: beyond the exact dot chains
    assert _new(lib, 4099, metric=2) == UNSUPPORTED                   # 1024 + 3
    for device in (0, -1):                                            # UNSUPPORTED before NO_DEVICE
        assert _new(lib, LB_MAX_DIM + 1, device=device) == UNSUPPORTED
        assert _new(lib, 16, metric=1, device=device) == UNSUPPORTED
        assert _new(lib, 4100, metric=2, device=device) == UNSUPPORTED
    for dim, nlist in ((1, 1), (3, 7), (768, 256), (4096, 2), (4097, 2), (LB_MAX_DIM, 1)):
        for metric in (0, 2):
            if metric == 2 and dim // 4 + dim % 4 > 1024:
                continue
            for order in (0, 1):
                c = np.zeros((nlist, dim), np.float32)
                device = 1 << 20 if lib.lb_gpu_device_count() > 0 else 0
                st = C.c_int(-1)
                assert not lib.lb_gpu_ivf_new_i8(device, dim, metric, order, nlist, c.ctypes.data, C.byref(st))
                assert st.value == NO_DEVICE, (dim, nlist, metric, order)
    c = np.zeros((4, 16), np.float32)
    st = C.c_int(-1)
    assert not lib.lb_gpu_ivf_new_i8(-1, 16, 0, 0, 4, c.ctypes.data, C.byref(st)) and st.value == NO_DEVICE
    # out_status is nullable
    assert not lib.lb_gpu_ivf_new_i8(-1, 16, 0, 0, 4, c.ctypes.data, None) and not lib.lb_gpu_ivf_new_i8(0, 0, 0, 0, 4, c.ctypes.data, None)
    assert not lib.lb_gpu_ivf_new_i8(0, 16, 1, 0, 4, c.ctypes.data, None)


def test_null_handle_is_refused_and_nothing_is_written(lib):
    dim, n, k = 20, 3, 2
    vec = np.full((n, dim), 7, np.int8)
    ids = np.full(n, 55, np.int64)
    dist = np.full((n, k), -3.0, np.float32)
    lab = np.full((n, k), -9, np.int64)
    for nn in (n, 0, -1):
        assert lib.lb_gpu_ivf_add_i8(None, nn, vec.ctypes.data, None) == INVALID
        assert lib.lb_gpu_ivf_add_i8(None, nn, vec.ctypes.data, ids.ctypes.data) == INVALID
        assert lib.lb_gpu_ivf_add_i8_device(None, nn, vec.ctypes.data, None) == INVALID
        assert lib.lb_gpu_ivf_add_i8_device(None, nn, vec.ctypes.data, ids.ctypes.data) == INVALID
        assert lib.lb_gpu_ivf_search_i8(None, nn, vec.ctypes.data, k, 1, dist.ctypes.data, lab.ctypes.data) == INVALID
        assert lib.lb_gpu_ivf_search_i8_ctx(None, nn, vec.ctypes.data, k, 1, dist.ctypes.data, lab.ctypes.data, None) == INVALID
        assert lib.lb_gpu_ivf_search_i8_device_ctx(None, nn, vec.ctypes.data, k, 1, dist.ctypes.data, lab.ctypes.data, None, None) == INVALID
    assert (vec == 7).all() and (ids == 55).all() and (dist == -3.0).all() and (lab == -9).all()
    assert lib.lb_gpu_ivf_dtype(None) == 0


def test_python_front_end_fails_loudly_without_a_gpu(lib):
    from longbow_amd import _lib, ivf
    device = 1 << 20 if lib.lb_gpu_device_count() > 0 else 0  # (a device that is not there, on a GPU box too)
    cent = np.zeros((4, 8), np.float32)
    with pytest.raises(_lib.GPUNotAvailable):
        ivf.IVFFlatInt8(cent, device=device)
    with pytest.raises(_lib.GPUNotAvailable):
        ivf.IVFFlatInt8(cent, metric=2, order=1, device=device)
    with pytest.raises(ValueError):
        ivf.IVFFlatInt8(cent, metric=1, device=device)  # cosine: before the library is touched
    with pytest.raises(ValueError):
        ivf.IVFFlatInt8(np.zeros((0, 8), np.float32), device=device)
    for bad in (np.float32, np.float16, np.uint8, np.int16):
        with pytest.raises(TypeError):
            ivf.rows_i8(np.zeros((2, 8), bad), 8)
    assert ivf.rows_i8(np.zeros((2, 8), np.int8), 8).shape == (2, 8) and ivf.rows_i8(np.zeros(0, np.int8), 8).shape == (0, 8)
    with pytest.raises(ValueError):
        ivf.rows_i8(np.zeros((2, 7), np.int8), 8)
