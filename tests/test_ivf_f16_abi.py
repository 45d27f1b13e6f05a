"""lb_gpu_ivf_new_f16 / _dtype / _add_f16 / _add_f16_device: the argument checks that need no handle answer before a device is
touched, in lb_gpu_ivf_new's documented order (INVALID_ARG, UNSUPPORTED, NO_DEVICE), and a refused call writes nothing, so all
of this runs on a box without a GPU, as tests/test_ivf_abi.py does for the float32 entry points.  The checks behind a live handle
are in tests/test_gpu_ivf_f16.py."""
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
    h = lib.lb_gpu_ivf_new_f16(device, dim, metric, order, nlist, c.ctypes.data if cent else None, C.byref(st))
    assert not h
    return st.value


def test_new_f16_checks_its_arguments_in_the_documented_order(lib):
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
                assert not lib.lb_gpu_ivf_new_f16(device, dim, metric, order, nlist, c.ctypes.data, C.byref(st))
                assert st.value == NO_DEVICE
    c = np.zeros((4, 16), np.float32)
    st = C.c_int(-1)
    assert not lib.lb_gpu_ivf_new_f16(-1, 16, 0, 0, 4, c.ctypes.data, C.byref(st)) and st.value == NO_DEVICE
    # out_status is nullable
    assert not lib.lb_gpu_ivf_new_f16(-1, 16, 0, 0, 4, c.ctypes.data, None) and not lib.lb_gpu_ivf_new_f16(0, 0, 0, 0, 4, c.ctypes.data, None)


def test_null_handle_is_refused_and_nothing_is_written(lib):
    dim, n = 20, 3
    vec = np.full((n, dim), 7.0, np.float16)
    ids = np.full(n, 55, np.int64)
    for nn in (n, 0, -1):
        assert lib.lb_gpu_ivf_add_f16(None, nn, vec.ctypes.data, None) == INVALID
        assert lib.lb_gpu_ivf_add_f16(None, nn, vec.ctypes.data, ids.ctypes.data) == INVALID
        assert lib.lb_gpu_ivf_add_f16_device(None, nn, vec.ctypes.data, None) == INVALID
        assert lib.lb_gpu_ivf_add_f16_device(None, nn, vec.ctypes.data, ids.ctypes.data) == INVALID
    assert (vec == 7.0).all() and (ids == 55).all()
    assert lib.lb_gpu_ivf_dtype(None) == 0


def test_python_front_end_fails_loudly_without_a_gpu(lib):
    from longbow_amd import _lib, ivf
    from longbow_amd.gpu import DataType
    device = 1 << 20 if lib.lb_gpu_device_count() > 0 else 0  # (a device that is not there, on a GPU box too)
    cent = np.zeros((4, 8), np.float32)
    with pytest.raises(_lib.GPUNotAvailable):
        ivf.IVFFlat(cent, device=device, dtype=DataType.Float16)
    with pytest.raises(ValueError):
        ivf.IVFFlat(cent, device=device, dtype=DataType.Int8)
    with pytest.raises(ValueError):
        ivf.IVFFlat(cent, device=device, dtype=7)
    with pytest.raises(_lib.GPUNotAvailable):
        ivf.IVFFlatIndex(8, ivf.IVFFlatConfig(NClusters=4, NProbe=2), device=device, data_type=DataType.Float16)
    with pytest.raises(ValueError):
        ivf.IVFFlatIndex(8, ivf.IVFFlatConfig(NClusters=4, NProbe=2), device=device, data_type=DataType.Int8)
    with pytest.raises(TypeError):
        ivf.rows_f16(np.zeros((2, 8), np.float32), 8)
    assert ivf.rows_f16(np.zeros((2, 8), np.float16), 8).shape == (2, 8) and ivf.rows_f16(np.zeros(0, np.float16), 8).shape == (0, 8)
    with pytest.raises(ValueError):
        ivf.rows_f16(np.zeros((2, 7), np.float16), 8)
