"""lb_gpu_pq_train / _train_device / lb_gpu_pq_blob_bytes: every argument check answers before a device is touched, in the
order include/longbow_gpu.h states, so all of this runs on a box without a GPU."""
import ctypes as C

import numpy as np
import pytest

INVALID, NO_DEVICE, UNSUPPORTED = 1, 3, 6


@pytest.fixture(scope="module")
def lib():
    from longbow_amd import _lib
    return _lib.load()


def _call(lib, device_entry=False, device=0, dims=8, M=2, K=4, n=10, vectors=True, max_iter=3, seed=0, init_rows=None, blob=True,
          blob_len=None, iters=True):
    """one call with valid defaults; on a GPU box `device` is moved out of range so that nothing ever runs"""
    if lib.lb_gpu_device_count() > 0:
        device = 1 << 20
    v = np.zeros((max(n, 1), max(dims, 1)), np.float32)
    size = 12 + max(M, 0) * max(K, 0) * (dims // M if M > 0 and dims > 0 else 0) * 4
    b = np.full(max(size, 12), 0xAB, np.uint8)
    it = np.zeros(max(M, 1), np.int32)
    rows = None if init_rows is None else np.ascontiguousarray(init_rows, np.int64)
    args = [device, dims, M, K, n, v.ctypes.data if vectors else None, max_iter, seed, rows.ctypes.data if rows is not None else None,
            b.ctypes.data if blob else None, size if blob_len is None else blob_len, it.ctypes.data if iters else None]
    rc = lib.lb_gpu_pq_train_device(*args, None, None) if device_entry else lib.lb_gpu_pq_train(*args, None)
    assert (b == 0xAB).all(), "a refused call wrote into the blob"
    return rc


@pytest.mark.parametrize("device_entry", [False, True])
def test_every_argument_check_answers_without_a_device(lib, device_entry):
    call = lambda **kw: _call(lib, device_entry, **kw)
    assert call(vectors=False) == INVALID
    assert call(blob=False) == INVALID
    assert call(M=0) == INVALID
    assert call(M=-1) == INVALID
    assert call(dims=9, M=2) == INVALID          # dims % M != 0
    assert call(dims=0) == INVALID
    assert call(n=3, K=4) == INVALID             # "insufficient data for k-means: n < k"
    assert call(n=-1, K=0) == INVALID
    assert call(max_iter=-1) == INVALID
    assert call(blob_len=12 + 2 * 4 * 4 * 4 - 1) == INVALID
    assert call(blob_len=12 + 2 * 4 * 4 * 4 + 4) == INVALID
    assert call(blob_len=0) == INVALID
    good = np.arange(8).reshape(2, 4)
    for bad_at, bad in ((0, -1), (7, 10), (3, 1 << 40)):
        rows = good.copy().reshape(-1)
        rows[bad_at] = bad
        assert call(init_rows=rows) == INVALID
    # INVALID_ARG comes before UNSUPPORTED: both wrong -> invalid
    assert call(K=300, n=299) == INVALID
    assert call(K=257, n=300, max_iter=-1) == INVALID
    assert call(dims=8200, M=2, max_iter=-1) == INVALID
    # unsupported: K outside 1..256, dims > LB_MAX_DIM
    assert call(K=0) == UNSUPPORTED
    assert call(K=257, n=300) == UNSUPPORTED
    assert call(dims=8200, M=2, K=1, n=1) == UNSUPPORTED
    assert call(dims=8192 + 4, M=4, K=1, n=1) == UNSUPPORTED


@pytest.mark.parametrize("device_entry", [False, True])
def test_valid_arguments_need_a_device(lib, device_entry):
    call = lambda **kw: _call(lib, device_entry, **kw)
    assert call() == NO_DEVICE
    assert call(iters=False) == NO_DEVICE                                   # iters_out is nullable
    assert call(init_rows=np.array([0, 0, 9, 9, 1, 1, 1, 1])) == NO_DEVICE  # duplicate init rows are allowed
    assert call(max_iter=0) == NO_DEVICE
    assert call(K=256, n=256, dims=8192, M=1) == NO_DEVICE
    assert call(K=1, n=1) == NO_DEVICE
    assert call(K=3, n=3, dims=5, M=1) == NO_DEVICE
    assert call(device=-1) == NO_DEVICE


def test_blob_bytes(lib):
    f = lib.lb_gpu_pq_blob_bytes
    assert f(768, 96, 256) == 12 + 96 * 256 * 8 * 4
    assert f(8, 2, 4) == 12 + 2 * 4 * 4 * 4
    assert f(5, 1, 3) == 12 + 3 * 5 * 4
    assert f(16, 16, 1) == 12 + 16 * 4
    assert f(8192, 1, 1000) == 12 + 1000 * 8192 * 4  # a K that persistence.go serialises and lb_gpu_pq_new refuses
    for dims, M, K in ((9, 2, 4), (8, 0, 4), (8, -2, 4), (0, 1, 4), (-8, 2, 4), (8, 2, 0), (8, 2, -1)):
        assert f(dims, M, K) == 0
    from longbow_amd import pq
    cb = np.zeros((3, 256, 4), np.float32)
    assert f(12, 3, 256) == len(pq.serialize_codebooks(cb))


def test_python_front_end_fails_loudly_without_a_gpu(lib):
    from longbow_amd import _lib, pq
    device = 1 << 20 if lib.lb_gpu_device_count() > 0 else 0  # (a device that is not there, on a GPU box too)
    with pytest.raises(_lib.GPUNotAvailable):
        pq.train(np.zeros((10, 8), np.float32), 2, 4, device=device)
    with pytest.raises(_lib.GPUNotAvailable):
        pq.PQEncoder.Train(np.zeros((300, 8), np.float32), 2, device=device)
    ms = (C.c_float * 3)()
    assert lib.lb_gpu_pq_train_last_timing(ms) == 0 and lib.lb_gpu_pq_train_last_timing(None) == INVALID
