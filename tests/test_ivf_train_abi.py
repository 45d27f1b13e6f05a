"""lb_gpu_ivf_train / _train_device / _train_last_timing: the symbols, and every argument check answering before a device is
touched, in the order include/longbow_gpu.h states, so all of this runs on a box without a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

INVALID, NO_DEVICE, UNSUPPORTED = 1, 3, 6
NAMES = ("lb_gpu_ivf_train", "lb_gpu_ivf_train_device", "lb_gpu_ivf_train_last_timing")


@pytest.fixture(scope="module")
def lib():
    from longbow_amd import _lib
    return _lib.load()


def _call(lib, device_entry=False, device=0, dims=8, nlist=4, n=10, vectors=True, max_iter=3, seed=0, init_rows=None, centroids=True,
          iters=True):
    """one call with valid defaults; on a GPU box `device` is moved out of range so that nothing ever runs"""
    if lib.lb_gpu_device_count() > 0:
        device = 1 << 20
    v = np.zeros((max(min(n, 1024), 1), max(dims, 1)), np.float32)  # (never read: no call here reaches a device)
    cent = np.full(max(min(nlist, 1024), 1) * max(dims, 1), 0xAB, np.uint8).repeat(4)
    it = np.full(1, 0x5A5A5A5A, np.int32)
    rows = None if init_rows is None else np.ascontiguousarray(init_rows, np.int64)
    args = [device, dims, nlist, n, v.ctypes.data if vectors else None, max_iter, seed, rows.ctypes.data if rows is not None else None,
            cent.ctypes.data if centroids else None, it.ctypes.data if iters else None]
    rc = lib.lb_gpu_ivf_train_device(*args, None, None) if device_entry else lib.lb_gpu_ivf_train(*args, None)
    assert (cent == 0xAB).all(), "a refused call wrote into the centroids"
    assert it[0] == 0x5A5A5A5A, "a refused call wrote iters_out"
    return rc


def test_symbols_are_exported_declared_and_bound(lib):
    from longbow_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "longbow_gpu.h")) as f:
        header = f.read()
    bound = {s[0] for s in _lib.SIGNATURES}
    for name in NAMES:
        assert hasattr(lib, name)
        assert f"int {name}(" in header
        assert name in bound


@pytest.mark.parametrize("device_entry", [False, True])
def test_every_argument_check_answers_without_a_device(lib, device_entry):
    call = lambda **kw: _call(lib, device_entry, **kw)
    assert call(vectors=False) == INVALID
    assert call(centroids=False) == INVALID
    assert call(dims=0) == INVALID
    assert call(dims=-3) == INVALID
    assert call(nlist=0) == INVALID
    assert call(nlist=-1) == INVALID
    assert call(n=3, nlist=4) == INVALID             # "insufficient data for k-means: n < k"
    assert call(n=-1, nlist=1) == INVALID
    assert call(max_iter=-1) == INVALID
    for bad_at, bad in ((0, -1), (3, 10), (2, 1 << 40)):
        rows = np.arange(4)
        rows[bad_at] = bad
        assert call(init_rows=rows) == INVALID
    # INVALID_ARG comes before UNSUPPORTED: both wrong -> invalid
    assert call(nlist=65537, n=65536) == INVALID
    assert call(nlist=65537, n=70000, max_iter=-1) == INVALID
    assert call(dims=8200, max_iter=-1) == INVALID
    assert call(n=1 << 31, max_iter=-1) == INVALID
    assert call(nlist=65537, n=70000, init_rows=np.full(65537, 70000)) == INVALID
    # unsupported: nlist > 65536, dims > LB_MAX_DIM, n >= 2^31
    assert call(nlist=65537, n=70000) == UNSUPPORTED
    assert call(dims=8193, nlist=1, n=1) == UNSUPPORTED
    assert call(n=1 << 31) == UNSUPPORTED
    # UNSUPPORTED comes before NO_DEVICE
    assert call(nlist=65537, n=70000, device=-1) == UNSUPPORTED


@pytest.mark.parametrize("device_entry", [False, True])
def test_valid_arguments_need_a_device(lib, device_entry):
    call = lambda **kw: _call(lib, device_entry, **kw)
    assert call() == NO_DEVICE
    assert call(iters=False) == NO_DEVICE                        # iters_out is nullable
    assert call(init_rows=np.array([0, 0, 9, 9])) == NO_DEVICE   # duplicate init rows are allowed
    assert call(max_iter=0) == NO_DEVICE
    assert call(nlist=257, n=300) == NO_DEVICE                   # past lb_gpu_pq_train's K
    assert call(nlist=65536, n=65536, dims=2) == NO_DEVICE
    assert call(nlist=300, n=300, dims=8192) == NO_DEVICE
    assert call(nlist=1, n=1, dims=1) == NO_DEVICE
    assert call(n=(1 << 31) - 1) == NO_DEVICE
    assert call(device=-1) == NO_DEVICE


def test_last_timing(lib):
    ms = (C.c_float * 3)()
    assert lib.lb_gpu_ivf_train_last_timing(ms) == 0 and lib.lb_gpu_ivf_train_last_timing(None) == INVALID


def test_python_front_end_checks_before_the_device_is_asked_for(lib):
    from longbow_amd import _lib, ivf
    device = 1 << 20 if lib.lb_gpu_device_count() > 0 else 0  # (a device that is not there, on a GPU box too)
    X = np.zeros((300, 8), np.float32)
    for nlist in (0, -1, 65537):
        with pytest.raises(ValueError, match="nlist in 1..65536"):
            ivf.train_coarse(X, nlist, device=device)
        with pytest.raises(ValueError, match="nlist in 1..65536"):
            ivf.train_coarse_device(300, 0, 8, nlist, device=device)
    for empty in (np.zeros((0, 8), np.float32), np.zeros(8, np.float32)):
        with pytest.raises(ValueError, match="empty training data"):
            ivf.train_coarse(empty, 4, device=device)
    with pytest.raises(ValueError, match="empty training data"):
        ivf.train_coarse_device(0, 0, 8, 4, device=device)
    for rows in (np.arange(5), np.arange(3), np.arange(4).reshape(1, 4), np.arange(8).reshape(2, 4)):
        with pytest.raises(ValueError, match="init_rows of shape"):
            ivf.train_coarse(X, 4, init_rows=rows, device=device)
        with pytest.raises(ValueError, match="init_rows of shape"):
            ivf.train_coarse_device(300, 0, 8, 4, init_rows=rows, device=device)
    with pytest.raises(_lib.GPUNotAvailable):
        ivf.train_coarse(X, 257, device=device)
    with pytest.raises(_lib.GPUNotAvailable):
        ivf.train_coarse_device(300, 0, 8, 257, device=device)


def test_train_keeps_its_limit(lib):
    from longbow_amd import ivf
    device = 1 << 20 if lib.lb_gpu_device_count() > 0 else 0
    X = np.zeros((300, 8), np.float32)
    with pytest.raises(ValueError, match="nlist <= 256"):
        ivf.train(X, 257, device=device)
    with pytest.raises(ValueError, match="nlist <= 256"):
        ivf.train_device(300, 0, 8, 257, device=device)


def test_given_centroids_are_checked_before_anything_runs(lib):
    from longbow_amd import ivfpq, ivfsq8
    device = 1 << 20 if lib.lb_gpu_device_count() > 0 else 0
    X = np.zeros((300, 8), np.float32)
    for bad in (np.zeros((299, 8), np.float32), np.zeros((300, 4), np.float32), np.zeros(300 * 8, np.float32)):
        with pytest.raises(ValueError, match="centroids of shape"):
            ivfpq.train(X, 300, 2, device=device, centroids=bad)
        with pytest.raises(ValueError, match="centroids of shape"):
            ivfsq8.train(X, 300, device=device, centroids=bad)
