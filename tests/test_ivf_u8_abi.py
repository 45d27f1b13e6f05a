"""lb_gpu_ivf_new_u8 and the uint8 adds and searches of the IVF-Flat handle, as far as no device is needed: the names, the order
of creation's refusals, a NULL handle, the Python front end.  Behind a live handle: tests/test_gpu_ivf_u8.py."""
import ctypes as C

import numpy as np
import pytest

INVALID, NO_DEVICE, UNSUPPORTED = 1, 3, 6
LB_MAX_DIM, MAX_NLIST = 8192, 65536
NAMES = ["lb_gpu_ivf_" + s for s in ("new_u8", "add_u8", "add_u8_device", "search_u8", "search_u8_ctx", "search_u8_device_ctx",
                                    "search_u8_bitmap_ctx", "search_u8_bitmap_device_ctx")]


@pytest.fixture(scope="module")
def lib():
    from longbow_amd import _lib
    return _lib.load()


def test_names_are_declared_exported_and_bound(lib):
    from tests.test_abi import _declared_symbols
    assert set(NAMES) <= set(_declared_symbols())
    for name in NAMES:
        assert getattr(lib, name).argtypes is not None, name  # (exported: getattr resolves the symbol; bound: a prototype is set)


def _new(lib, dim, metric=0, order=0, nlist=4, device=0, cent=True):
    if lib.lb_gpu_device_count() > 0 and device >= 0:
        device = 1 << 20  # (on a GPU box the device is moved out of range, so that nothing is ever created)
    c = np.zeros((max(1, min(nlist, 8)), max(1, min(dim, LB_MAX_DIM))), np.float32)
    st = C.c_int(-1)
    assert not lib.lb_gpu_ivf_new_u8(device, dim, metric, order, nlist, c.ctypes.data if cent else None, C.byref(st))
    return st.value


def test_new_u8_checks_its_arguments_in_the_documented_order(lib):
    for bad in (dict(dim=0), dict(dim=-1), dict(dim=16, metric=3), dict(dim=16, metric=-1), dict(dim=16, order=2), dict(dim=16, nlist=0),
                dict(dim=16, cent=False), dict(dim=0, device=-1), dict(dim=LB_MAX_DIM + 1, nlist=0), dict(dim=16, metric=1, nlist=0),
                dict(dim=16, metric=2, order=2)):
        assert _new(lib, **bad) == INVALID, bad
    for device in (0, -1):  # UNSUPPORTED before NO_DEVICE
        assert _new(lib, LB_MAX_DIM + 1, device=device) == UNSUPPORTED
        assert _new(lib, 16, nlist=MAX_NLIST + 1, device=device) == UNSUPPORTED
        assert _new(lib, 16, metric=1, device=device) == UNSUPPORTED  # the reference has a Euclidean uint8 kernel alone
        assert _new(lib, 16, metric=2, device=device) == UNSUPPORTED
    for dim, nlist, order, device in ((1, 1, 0, 0), (3, 7, 1, -1), (768, 8, 0, 0), (LB_MAX_DIM, 1, 1, -1)):
        assert _new(lib, dim, nlist=nlist, order=order, device=device) == NO_DEVICE, (dim, nlist, order)
    c = np.zeros((4, 16), np.float32)  # out_status is nullable
    assert not lib.lb_gpu_ivf_new_u8(-1, 16, 0, 0, 4, c.ctypes.data, None) and not lib.lb_gpu_ivf_new_u8(0, 16, 2, 0, 4, c.ctypes.data, None)


def test_null_handle_is_refused_and_nothing_is_written(lib):
    vec, ids, bits = np.full((3, 20), 7, np.uint8), np.full(3, 55, np.int64), np.full(1, 0xFF, np.uint8)
    dist, lab = np.full((3, 2), -3.0, np.float32), np.full((3, 2), -9, np.int64)
    v, b, out = vec.ctypes.data, bits.ctypes.data, (dist.ctypes.data, lab.ctypes.data)
    for n in (3, 0, -1):
        for ids_ in (None, ids.ctypes.data):
            assert lib.lb_gpu_ivf_add_u8(None, n, v, ids_) == INVALID and lib.lb_gpu_ivf_add_u8_device(None, n, v, ids_) == INVALID
        assert lib.lb_gpu_ivf_search_u8(None, n, v, 2, 1, *out) == INVALID
        assert lib.lb_gpu_ivf_search_u8_ctx(None, n, v, 2, 1, *out, None) == INVALID
        assert lib.lb_gpu_ivf_search_u8_device_ctx(None, n, v, 2, 1, *out, None, None) == INVALID
        assert lib.lb_gpu_ivf_search_u8_bitmap_ctx(None, n, v, 2, 1, b, 3, 0, *out, None) == INVALID
        assert lib.lb_gpu_ivf_search_u8_bitmap_device_ctx(None, n, v, 2, 1, b, 3, 0, *out, None, None) == INVALID
    assert (vec == 7).all() and (ids == 55).all() and (dist == -3.0).all() and (lab == -9).all() and bits[0] == 0xFF


def test_python_front_end_fails_loudly_without_a_gpu(lib):
    from longbow_amd import _lib, ivf
    device = 1 << 20 if lib.lb_gpu_device_count() > 0 else 0  # (a device that is not there, on a GPU box too)
    cent = np.zeros((4, 8), np.float32)
    with pytest.raises(_lib.GPUNotAvailable):
        ivf.IVFFlatUint8(cent, order=1, device=device)
    for metric in (1, 2, 3):
        with pytest.raises(ValueError):
            ivf.IVFFlatUint8(cent, metric=metric, device=device)  # before the library is touched
    for bad in (np.int8, np.float32, np.float16):
        with pytest.raises(TypeError):
            ivf.rows_u8(np.zeros((2, 8), bad), 8)
    assert ivf.rows_u8(np.zeros((2, 8), np.uint8), 8).shape == (2, 8)
