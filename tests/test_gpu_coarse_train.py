"""The coarse quantiser's training on the GPU -- ivf.train / ivf.train_device, ivfpq.train and IVFFlatIndex.Build() without
centroids -- against tests/kmeans_oracle.py, bit for bit.  It is lb_gpu_pq_train with M = 1, K = nlist and sub = dims, so the
shape decides the E-step kernel:

  (1500,  768, 100)  km_estep_generic_kernel, 192 4-wide steps; 6 row blocks, one ordering chunk, K off the wave
  ( 600, 1536,  64)  generic, 384 steps; K one full wave
  ( 300, 8192,   8)  generic, 2048 steps (LB_MAX_DIM); 65,536 M-step lanes for 8 clusters
  (5000,  100, 200)  generic, 25 steps and no tail; two ordering chunks with K off the wave
  ( 300,    7, 256)  generic, one step and a 3-element tail; every scan lane holds a cluster
  (2000,   32, 256)  km_estep_kernel<32>, the 32 KB codebook in LDS
  dims 20, 24        generic, 5 and 6 steps (the nlist edges, Build(), the few-pattern rows)

tests/test_gpu_pq_train.py holds the same kernels at the PQ geometry (many narrow subspaces); tests/test_kmeans_semantics.py pins
the oracle to a scalar Lloyd loop and asserts what the few-pattern rows below rely on."""
import functools

import numpy as np
import pytest

from tests import ivf_oracle as io
from tests import ivfpq_oracle as pqo
from tests import kmeans_oracle as ko
from tests.gpu_util import gpu_or_skip

pytestmark = pytest.mark.gpu
F = np.float32
SHAPES = [(1500, 768, 100, 2), (600, 1536, 64, 2), (300, 8192, 8, 2), (5000, 100, 200, 3), (300, 7, 256, 3), (2000, 32, 256, 3)]
INITS = ["given", 0, 0xDEADBEEFCAFEF00D]  # init rows handed in, or drawn from this seed


def _first_difference(got, want):
    bad = np.argwhere(np.ascontiguousarray(got, F).view(np.uint32) != np.ascontiguousarray(want, F).view(np.uint32))
    return f"{len(bad)} centroid words differ, first (c, j) {bad[:5].tolist()}"


def _same(got, want):
    assert got.shape == want.shape and got.dtype == F
    assert got.tobytes() == np.ascontiguousarray(want, F).tobytes(), _first_difference(got, want)


@functools.lru_cache(maxsize=None)
def _case(shape, init):
    """-> (rows X, init rows or None, seed, the oracle's centroids): computed once, shared, never written to"""
    n, dims, nlist, max_iter = shape
    rng = np.random.default_rng(n + dims + nlist)
    X = rng.standard_normal((n, dims)).astype(F)
    rows = rng.permutation(n)[:nlist].astype(np.int64) if init == "given" else None
    seed = 5 if init == "given" else init
    want, _ = ko.train_kmeans(X, nlist, max_iter, rows, seed)
    for a in (X, want):
        a.setflags(write=False)
    return X, rows, seed, want


@pytest.mark.parametrize("init", INITS)
@pytest.mark.parametrize("shape", SHAPES)
def test_train_is_train_kmeans(shape, init):
    from longbow_amd import ivf
    gpu_or_skip()
    X, rows, seed, want = _case(shape, init)
    _same(ivf.train(X, shape[2], shape[3], seed, rows), want)


def test_one_list_is_the_sequential_column_mean():
    from longbow_amd import ivf
    gpu_or_skip()
    X = ko.order_sensitive_rows(3000, 20)
    seq = np.zeros(20, F)
    for i in range(X.shape[0]):
        seq = seq + X[i]
    for max_iter in (1, 3):  # (the second iteration changes nothing and is the last)
        got = ivf.train(X, 1, max_iter, init_rows=[17])
        _same(got, (seq / F(X.shape[0]))[None])
        _same(got, ko.train_kmeans(X, 1, max_iter, [17])[0])


@pytest.mark.parametrize("seed", [0, 9])
def test_as_many_lists_as_rows(seed):
    from longbow_amd import ivf
    gpu_or_skip()
    X = np.random.default_rng(100 + seed).standard_normal((100, 20)).astype(F)
    got = ivf.train(X, 100, 0, seed)
    _same(got, X[ko.init_rows(seed, 0, 100, 100)])
    assert sorted(r.tobytes() for r in got) == sorted(r.tobytes() for r in X)  # a permutation of all rows
    _same(ivf.train(X, 100, 2, seed), ko.train_kmeans(X, 100, 2, None, seed)[0])
    assert sorted(r.tobytes() for r in ivf.train(X, 100, 2, seed)) == sorted(r.tobytes() for r in X)  # every row its own list


def test_device_entry_point():
    import torch
    from longbow_amd import ivf
    gpu_or_skip()
    shape = SHAPES[0]
    n, dims, nlist, max_iter = shape
    for init in ("given", 0):
        X, rows, seed, want = _case(shape, init)
        dX = torch.from_numpy(np.array(X)).cuda()
        torch.cuda.synchronize()
        got = ivf.train_device(n, dX.data_ptr(), dims, nlist, max_iter, seed, rows)
        _same(got, want)
        _same(got, ivf.train(X, nlist, max_iter, seed, rows))
        first = ivf.train_device(n, dX.data_ptr(), dims, nlist, 0, seed, rows)
        _same(first, X[rows if rows is not None else ko.init_rows(seed, 0, nlist, n)])


def test_ivfpq_train():
    """the coarse centroids and the codebooks come from the same rows, and the drawn init rows follow (seed, m)"""
    from longbow_amd import ivfpq
    gpu_or_skip()
    X = np.random.default_rng(1500).standard_normal((1500, 32)).astype(F)
    cent, blob = ivfpq.train(X, 8, 4, max_iter=3, seed=3)
    _same(cent, ko.train_kmeans(X, 8, 3, None, 3)[0])
    cb, _ = ko.train_pq(X, 4, 256, 3, 3)
    assert blob[:12] == ko.blob(cb)[:12]
    _same(np.frombuffer(blob[12:], "<f4").reshape(4, 256 * 8), cb.reshape(4, 256 * 8))
    assert blob == ko.blob(cb)
    cent0, blob0 = ivfpq.train(X, 8, 4, max_iter=0, seed=3)
    _same(cent0, X[ko.init_rows(3, 0, 8, 1500)])
    cb0 = np.frombuffer(blob0[12:], "<f4").reshape(4, 256, 8)
    for m in range(4):
        _same(cb0[m], X[ko.init_rows(3, m, 256, 1500), m * 8:(m + 1) * 8])
    assert not np.array_equal(ko.init_rows(3, 0, 256, 1500), ko.init_rows(3, 1, 256, 1500))


def test_build_without_centroids_trains_on_every_buffered_row(oracle):
    from longbow_amd import ivf
    gpu_or_skip()
    X = np.random.default_rng(20).standard_normal((500, 20)).astype(F)
    idx = ivf.IVFFlatIndex(20, ivf.IVFFlatConfig(NClusters=12, NProbe=3), train_iters=3, seed=5)
    idx.AddBatch(np.arange(300), X[:300])
    idx.AddBatch(np.arange(300, 500), X[300:])
    idx.Build()
    want, _ = ko.train_kmeans(X, 12, 3, None, 5)
    assert want.tobytes() != ko.train_kmeans(X[:300], 12, 3, None, 5)[0].tobytes()  # (the second piece is seen)
    _same(idx._h.centroids(), want)
    assert idx.Size() == 500 and np.array_equal(idx.assignments(), io.assign(oracle, 0, 0, X, want))
    idx.Close()


@pytest.mark.parametrize("order", [0, 1])
def test_trained_centroids_with_equal_copies_are_usable(oracle, order):
    """few-pattern rows: the trained centroids are five patterns held by sixteen lists, and among equal centroids the lowest list
    takes the rows, in both handles"""
    from longbow_amd import ivf, ivfpq
    gpu_or_skip()
    X, rows = ko.few_pattern_case(1, 16, 77)
    want, _ = ko.train_kmeans(X, 16, 6, rows[0], 77)
    cent = ivf.train(X, 16, 6, 77, rows[0])
    _same(cent, want)
    assert np.unique(cent, axis=0).shape[0] == 5
    lists = io.assign(oracle, 0, order, X, cent)
    first = {c.tobytes(): i for i, c in reversed(list(enumerate(cent)))}  # the lowest list of every distinct centroid
    assert np.array_equal(lists, [first[x.tobytes()] for x in X]) and np.unique(lists).size == 5
    flat = ivf.IVFFlat(cent, 0, order)
    flat.add(X)
    assert np.array_equal(flat.assignments(), lists) and np.array_equal(flat.list_sizes(), np.bincount(lists, minlength=16))
    flat.Close()
    h = ivfpq.IVFPQ(pqo.blob(pqo.codebooks(24, 3, 7)), cent, order)
    h.add(X)
    assert np.array_equal(h.assignments(), lists) and np.array_equal(h.list_sizes(), np.bincount(lists, minlength=16))
    h.Close()


def test_refusals_stay_refusals():
    from longbow_amd import _lib, ivf
    gpu_or_skip()
    X = np.random.default_rng(3).standard_normal((600, 100)).astype(F)
    with pytest.raises(_lib.LongbowGPUError) as e:
        ivf.train(X[:5], 8)  # n < nlist
    assert e.value.code == 1
    for call in (lambda: ivf.train(X, 257, device=1 << 20), lambda: ivf.train_device(600, 0, 100, 257, device=1 << 20)):
        with pytest.raises(ValueError, match="nlist <= 256"):  # before the device is asked for: that one does not exist
            call()
    with pytest.raises(_lib.GPUNotAvailable):
        ivf.train(X, 256, device=1 << 20)
    Y = X.copy()
    Y[311, 97] = np.nan
    with pytest.raises(_lib.LongbowGPUError) as e:
        ivf.train(Y, 8, 3, init_rows=np.arange(8))
    assert e.value.code == 1 and type(e.value) is _lib.LongbowGPUError
    ivf.train(X, 8, 3, init_rows=np.arange(8))
