"""int8 index semantics, no device needed: the oracle (tests/i8_oracle.py) against line-for-line transcriptions of the
reference's int8 registry kernels, the properties the index's design rests on, the ABI and the Python argument checks."""
import ctypes as C

import numpy as np
import pytest

from tests import i8_oracle as io

F = np.float32
DIMS = [1, 3, 15, 16, 17, 100, 768, 1024, 1031, 4096]


def _rows(rng, n, D):
    X = rng.integers(-128, 128, (n, D), dtype=np.int64).astype(np.int8)
    X[0] = 127
    X[1] = -128
    X[2, ::2] = -128  # alternating extremes
    X[2, 1::2] = 127
    return X


@pytest.mark.parametrize("D", DIMS)
def test_vectorised_oracle_matches_the_transcriptions(D):
    rng = np.random.default_rng(D)
    X = _rows(rng, 6, D)
    Q = np.concatenate([_rows(rng, 3, D), X[:1], X[1:2]])
    l2 = io.l2_values(Q, X)
    dot = io.dot_values(Q, X)
    for i in range(Q.shape[0]):
        for j in range(X.shape[0]):
            assert l2[i, j] == io.euclidean_int8_avx2(Q[i], X[j]), (D, i, j)
            if D // 4 + D % 4 <= 1024:  # (the dot index's dimension limit: chains stay exact integers)
                assert dot[i, j] == io.dot_int8_unrolled4x(Q[i], X[j]), (D, i, j)
    d = io.distances(2, Q, X)
    assert np.array_equal(d, -dot)


@pytest.mark.parametrize("D", [16, 100, 768, 1024])
def test_unrolled4x_equals_avx2_below_2_24(D):
    # every total below 2^24 is an exact f32 integer in both forms
    rng = np.random.default_rng(7 + D)
    X = rng.integers(-40, 40, (8, D), dtype=np.int64).astype(np.int8)
    Q = rng.integers(-40, 40, (2, D), dtype=np.int64).astype(np.int8)
    for q in Q:
        for x in X:
            diff = q.astype(np.int64) - x.astype(np.int64)
            if int((diff * diff).sum()) < 2 ** 24:
                assert io.euclidean_int8_avx2(q, x) == io.euclidean_int8_unrolled4x(q, x)


def test_avx2_and_unrolled4x_forms_differ_beyond_2_24():
    # where the two registry forms disagree, the AVX2 form (what amd64 dispatches) is the index's
    rng = np.random.default_rng(11)
    D = 4096
    differ = 0
    for _ in range(40):
        a = rng.choice(np.array([-128, 127], np.int8), D)
        b = rng.choice(np.array([-128, 127, 0], np.int8), D)
        differ += io.euclidean_int8_avx2(a, b) != io.euclidean_int8_unrolled4x(a, b)
    assert differ > 0


def test_equal_values_from_unequal_sums_at_768():
    # at D = 768 the sums are near 2^23: sqrt maps neighbouring integers to one f32, so ranking by S is not ranking by value
    rng = np.random.default_rng(3)
    D = 768
    X = rng.integers(-128, 128, (20000, D), dtype=np.int64).astype(np.int8)
    q = rng.integers(-128, 128, (1, D), dtype=np.int64).astype(np.int8)
    v = io.l2_values(q, X)[0]
    diff = X.astype(np.int64) - q.astype(np.int64)
    S = (diff * diff).sum(1)
    assert np.array_equal(v, np.sqrt(S.astype(np.float64).astype(F).astype(np.float64)).astype(F))
    o = np.argsort(v, kind="stable")
    same_v = v[o][1:] == v[o][:-1]
    diff_s = S[o][1:] != S[o][:-1]
    assert np.count_nonzero(same_v & diff_s) > 0
    # the oracle orders such rows by row index
    lab, dist = io.topk(v, 20000)
    for i in range(1, len(lab)):
        assert (dist[i - 1], lab[i - 1]) < (dist[i], lab[i])


def test_search_oracle_ties_and_padding():
    X = np.zeros((5, 16), np.int8)
    X[3] = 1
    q = np.zeros((1, 16), np.int8)
    lab, dist = io.search(0, q, X, 7, chunk=2)
    assert lab.tolist() == [[0, 1, 2, 4, 3, -1, -1]]
    assert dist[0, :4].tolist() == [0, 0, 0, 0] and dist[0, 4] == F(4) and dist[0, 5] == np.finfo(F).max
    lab, dist = io.search(2, np.ones((1, 16), np.int8), X, 2, visible=[1, 3, 4])
    assert lab.tolist() == [[3, 1]] and dist[0].tolist() == [-16.0, 0.0]


I8_SYMBOLS = ["lb_gpu_index_new_i8", "lb_gpu_index_add_i8", "lb_gpu_index_add_i8_device", "lb_gpu_index_search_i8",
              "lb_gpu_index_search_i8_ctx", "lb_gpu_index_search_i8_device_ctx"]


def test_i8_symbols_exported():
    from longbow_amd import _lib
    lib = _lib.load()
    raw = C.CDLL(lib._name)
    for name in I8_SYMBOLS:
        assert hasattr(lib, name), name
        getattr(raw, name)


def test_i8_creation_checks_before_the_device():
    from longbow_amd import _lib
    lib = _lib.load()
    st = C.c_int(-1)
    assert not lib.lb_gpu_index_new_i8(0, 0, 0, C.byref(st)) and st.value == 1  # dim <= 0
    for dim, metric in [(16, 1), (4100, 2), (4099, 2), (8193, 0)]:  # cosine; dot beyond the exact chains; dim > 8192
        st.value = -1
        assert not lib.lb_gpu_index_new_i8(0, dim, metric, C.byref(st))
        assert st.value == 6, (dim, metric)
    assert lib.lb_gpu_index_add_i8(None, 1, None, None) == 1
    assert lib.lb_gpu_index_search_i8(None, 1, None, 1, None, None) == 1
    assert lib.lb_gpu_index_search_i8_ctx(None, 1, None, 1, None, None, None) == 1


def test_python_i8_data_type_and_element_checks():
    from longbow_amd import gpu
    assert gpu.DataType.Int8 == 2
    assert gpu.GPUConfig(DataType=gpu.DataType.Int8).DataType == 2
    idx = gpu.Index.__new__(gpu.Index)  # no device: only the element checks run
    idx._np = np.int8
    with pytest.raises(TypeError):
        idx._as_elems(np.zeros(4, np.float32))
    with pytest.raises(TypeError):
        idx._as_elems(np.zeros(4, np.uint8))
    assert idx._as_elems(np.zeros(4, np.int8)).dtype == np.int8
    with pytest.raises(ValueError):
        gpu.Index(gpu.GPUConfig(DeviceID=0, Dimension=8, DataType=3))


def test_arrow_int8_column_checks():
    pa = pytest.importorskip("pyarrow")
    from longbow_amd import arrow_io
    x = np.arange(-6, 6, dtype=np.int8)
    col8 = pa.FixedSizeListArray.from_arrays(pa.array(x, pa.int8()), 4)
    colu8 = pa.FixedSizeListArray.from_arrays(pa.array(x.astype(np.uint8), pa.uint8()), 4)
    col32 = pa.FixedSizeListArray.from_arrays(pa.array(x.astype(F), pa.float32()), 4)
    got = arrow_io._vector_values(col8, 4, i8=True)
    assert got.dtype == np.int8 and np.array_equal(got.reshape(-1), x)
    for bad in (colu8, col32):
        with pytest.raises(arrow_io.ExchangeError):
            arrow_io._vector_values(bad, 4, i8=True)


def test_arrow_exchange_refuses_an_int8_dataset():
    pytest.importorskip("pyarrow")
    from longbow_amd import arrow_io

    class DS:  # (no device: the refusal comes before any search)
        dim = 4
        i8 = True
    with pytest.raises(arrow_io.ExchangeError) as e:
        arrow_io.handle_vector_search_action({"d": DS()}, b'{"dataset": "d", "vectors": [[1, 2, 3, 4]], "k": 1}')
    assert e.value.code == "Unimplemented"
