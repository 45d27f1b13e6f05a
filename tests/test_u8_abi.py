"""The uint8 index's entry points on a box without a GPU: declared, exported, bound, and every check that needs no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

U8_SYMBOLS = ["lb_gpu_index_new_u8", "lb_gpu_index_add_u8", "lb_gpu_index_add_u8_device", "lb_gpu_index_search_u8",
              "lb_gpu_index_search_u8_ctx", "lb_gpu_index_search_u8_device_ctx", "lb_gpu_index_search_u8_bitmap_ctx",
              "lb_gpu_index_search_u8_bitmap_device_ctx"]
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "longbow_gpu.h")


@pytest.fixture(scope="module")
def lib():
    from longbow_amd import _lib
    return _lib.load()


def test_symbols_exported_declared_and_bound(lib):
    from longbow_amd import _lib
    header = open(HEADER).read()
    bound = {name for name, _, _ in _lib.SIGNATURES}
    raw = C.CDLL(lib._name)
    for name in U8_SYMBOLS:
        assert re.search(rf"\b{name}\(", header), f"{name} not declared"
        assert name in bound and hasattr(lib, name), f"{name} not bound"
        getattr(raw, name)


def test_creation_checks_in_order_before_the_device(lib):
    st = C.c_int(-1)
    for dim, metric in [(0, 0), (-4, 1), (16, 3), (16, -1)]:  # INVALID_ARG first, whatever else is wrong
        st.value = -1
        assert not lib.lb_gpu_index_new_u8(0, dim, metric, C.byref(st)) and st.value == 1, (dim, metric)
    for dim, metric in [(8193, 0), (16, 1), (16, 2), (768, 2)]:  # dim beyond LB_MAX_DIM; cosine and dot have no uint8 kernel
        st.value = -1
        assert not lib.lb_gpu_index_new_u8(0, dim, metric, C.byref(st)) and st.value == 6, (dim, metric)
    if lib.lb_gpu_device_count() == 0:
        st.value = -1
        assert not lib.lb_gpu_index_new_u8(0, 16, 0, C.byref(st)) and st.value == 3  # NO_DEVICE last
    assert not lib.lb_gpu_index_new_u8(1 << 20, 16, 0, C.byref(st)) and st.value == 3


def test_null_handle_refused_with_outputs_untouched(lib):
    q = np.zeros(16, np.uint8)
    dist = np.full(4, 7.5, np.float32)
    lab = np.full(4, 77, np.int64)
    bm = np.zeros(1, np.uint8)
    a = (q.ctypes.data, 4, dist.ctypes.data, lab.ctypes.data)
    assert lib.lb_gpu_index_add_u8(None, 1, q.ctypes.data, None) == 1
    assert lib.lb_gpu_index_add_u8_device(None, 1, q.ctypes.data, None) == 1
    assert lib.lb_gpu_index_search_u8(None, 1, *a) == 1
    assert lib.lb_gpu_index_search_u8_ctx(None, 1, *a, None) == 1
    assert lib.lb_gpu_index_search_u8_device_ctx(None, 1, *a, None, None) == 1
    assert lib.lb_gpu_index_search_u8_bitmap_ctx(None, 1, q.ctypes.data, 4, bm.ctypes.data, 8, dist.ctypes.data, lab.ctypes.data, None) == 1
    assert lib.lb_gpu_index_search_u8_bitmap_device_ctx(None, 1, q.ctypes.data, 4, bm.ctypes.data, 8, dist.ctypes.data, lab.ctypes.data,
                                                        None, None) == 1
    assert (dist == 7.5).all() and (lab == 77).all()


def test_python_data_type_and_element_checks(lib):
    from longbow_amd import gpu
    assert gpu.DataType.Uint8 == 3
    cfg = gpu.GPUConfig(DeviceID=0, Dimension=16, DataType=gpu.DataType.Uint8)
    assert cfg.DataType == 3
    with pytest.raises(ValueError):  # the type has its own constructor
        gpu.Index(cfg)
    with pytest.raises(ValueError):
        gpu.NewUint8Index(gpu.GPUConfig(Dimension=16))
    if lib.lb_gpu_device_count() == 0:
        with pytest.raises(gpu.ErrGPUNotAvailable):
            gpu.NewUint8Index(cfg)
    idx = gpu.Index.__new__(gpu.Index)  # no device: only the element checks run
    idx._np = np.uint8
    for wrong in (np.int8, np.float32, np.float16):
        with pytest.raises(TypeError):
            idx._as_elems(np.zeros(4, wrong))
    assert idx._as_elems(np.zeros(4, np.uint8)).dtype == np.uint8
    idx._lib = lib
    assert idx._entry("lb_gpu_index_search", "_bitmap_ctx") is lib.lb_gpu_index_search_u8_bitmap_ctx
