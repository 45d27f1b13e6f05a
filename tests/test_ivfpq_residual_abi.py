"""lb_gpu_ivfpq_new_residual / lb_gpu_ivfpq_residual without a device: the residual constructor has the arguments, limits, order
of checks and status codes of lb_gpu_ivfpq_new (tests/test_ivfpq_abi.py), every refusal answers before a device is touched, and
the Python front end fails loudly where there is no GPU."""
import ctypes as C
import struct

import numpy as np
import pytest

INVALID, NO_DEVICE, UNSUPPORTED = 1, 3, 6
LB_MAX_DIM, MAX_NLIST = 8192, 65536


@pytest.fixture(scope="module")
def lib():
    from longbow_amd import _lib
    return _lib.load()


def _blob(dims=16, M=4, K=256, extra=0):
    return struct.pack("<III", dims, M, K) + bytes(M * K * (dims // M if M else 0) * 4 + extra)


def _new_both(lib, blob=None, order=0, nlist=4, device=0, cent=True, length=None, null_blob=False):
    """the status of both constructors for one refused argument set (on a GPU box `device` is moved out of range so that
    nothing is ever created); they must agree"""
    if lib.lb_gpu_device_count() > 0 and device >= 0:
        device = 1 << 20
    blob = _blob() if blob is None else blob
    c = np.zeros(64, np.float32)  # (never read: every call here is refused first)
    got = []
    for new in (lib.lb_gpu_ivfpq_new, lib.lb_gpu_ivfpq_new_residual):
        st = C.c_int(-1)
        h = new(device, None if null_blob else blob, len(blob) if length is None else length, order, nlist,
                c.ctypes.data if cent else None, C.byref(st))
        assert not h
        got.append(st.value)
    assert got[0] == got[1], got
    return got[1]


def test_new_residual_checks_its_arguments_as_new_does(lib):
    """the refused argument sets of tests/test_ivfpq_abi.py::test_new_checks_its_arguments_in_the_documented_order"""
    assert _new_both(lib, null_blob=True) == INVALID
    assert _new_both(lib, length=8) == INVALID
    assert _new_both(lib, _blob(extra=4)) == INVALID
    assert _new_both(lib, _blob()[:-4]) == INVALID
    assert _new_both(lib, _blob(dims=18, M=4)) == INVALID
    assert _new_both(lib, struct.pack("<III", 16, 0, 256)) == INVALID
    assert _new_both(lib, order=2) == INVALID
    assert _new_both(lib, order=-1) == INVALID
    assert _new_both(lib, nlist=0) == INVALID
    assert _new_both(lib, nlist=-3) == INVALID
    assert _new_both(lib, cent=False) == INVALID
    assert _new_both(lib, nlist=0, device=-1) == INVALID                    # INVALID_ARG before NO_DEVICE
    assert _new_both(lib, _blob(K=16), nlist=0) == INVALID                  # INVALID_ARG before UNSUPPORTED
    assert _new_both(lib, _blob(K=16)) == UNSUPPORTED
    assert _new_both(lib, _blob(K=257)) == UNSUPPORTED
    assert _new_both(lib, _blob(dims=160, M=160)) == UNSUPPORTED
    assert _new_both(lib, _blob(dims=LB_MAX_DIM + 1, M=1)) == UNSUPPORTED
    assert _new_both(lib, nlist=MAX_NLIST + 1) == UNSUPPORTED
    assert _new_both(lib, _blob(K=16), device=-1) == UNSUPPORTED            # UNSUPPORTED before NO_DEVICE
    for dims, M in ((16, 4), (159, 159), (768, 96), (4, 1)):
        for order in (0, 1):
            for nlist in (1, 7, MAX_NLIST):
                assert _new_both(lib, _blob(dims, M), order=order, nlist=nlist) == NO_DEVICE
    assert _new_both(lib, device=-1) == NO_DEVICE
    # out_status is nullable
    c = np.zeros(64, np.float32)
    b = _blob()
    assert not lib.lb_gpu_ivfpq_new_residual(-1, b, len(b), 0, 4, c.ctypes.data, None)
    assert not lib.lb_gpu_ivfpq_new_residual(0, None, 0, 0, 4, c.ctypes.data, None)


def test_no_handle_is_not_residual(lib):
    assert lib.lb_gpu_ivfpq_residual(None) == 0


def test_python_front_end_fails_loudly_without_a_gpu(lib):
    from longbow_amd import _lib, ivfpq
    device = 1 << 20 if lib.lb_gpu_device_count() > 0 else 0  # (a device that is not there, on a GPU box too)
    with pytest.raises(_lib.GPUNotAvailable):
        ivfpq.IVFPQ(_blob(8, 2), np.zeros((4, 8), np.float32), device=device, residual=True)
    with pytest.raises(_lib.GPUNotAvailable):
        ivfpq.train(np.zeros((600, 8), np.float32), 4, 2, device=device, residual=True)
    with pytest.raises(ValueError, match="dimensions"):
        ivfpq.IVFPQ(_blob(8, 2), np.zeros((4, 16), np.float32), device=device, residual=True)
