"""float16 index, CPU side: the premise that the reference's F16 distances are its f32 arithmetic on widened values, the
exported ABI, and the argument checks the Python layer makes before it touches a device.

The reference's euclideanF16Unrolled4x / cosineF16Unrolled4x / dotF16Unrolled4x (internal/simd/simd.go:767-848) widen each
fp16 element to float32 and accumulate in four float32 chains (elements beyond the last group of four into chain 0), summed
((s0 + s1) + s2) + s3; Euclidean is float32(sqrt(float64(sum))), cosine 1 - dot / float32(sqrt(float64(|a|^2) * float64(|b|^2)))
with 1 for a zero vector, dot the raw sum.  Restated here step by step in numpy float32 and checked against oracle_c's
UNROLL4 order on the widened inputs: that oracle is then the exact yardstick of the GPU tests."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle_c as oc

F = np.float32


def _chains(terms):
    s = [F(0), F(0), F(0), F(0)]
    main = len(terms) // 4 * 4
    for i in range(main):
        s[i % 4] = F(s[i % 4] + terms[i])
    for i in range(main, len(terms)):
        s[0] = F(s[0] + terms[i])
    return F(F(F(s[0] + s[1]) + s[2]) + s[3])


def euclidean_f16_unrolled4x(a, b):
    a, b = a.astype(F), b.astype(F)
    return F(np.sqrt(np.float64(_chains([F(F(x - y) * F(x - y)) for x, y in zip(a, b)]))))


def dot_f16_unrolled4x(a, b):
    a, b = a.astype(F), b.astype(F)
    return _chains([F(x * y) for x, y in zip(a, b)])


def cosine_f16_unrolled4x(a, b):
    a, b = a.astype(F), b.astype(F)
    d = _chains([F(x * y) for x, y in zip(a, b)])
    na = _chains([F(x * x) for x in a])
    nb = _chains([F(y * y) for y in b])
    if len(a) == 0 or na == 0 or nb == 0:
        return F(1)
    return F(F(1) - F(d / F(np.sqrt(np.float64(na) * np.float64(nb)))))


def _vectors(rng, dim):
    vs = [rng.standard_normal(dim).astype(np.float16), (rng.random(dim) * 200 - 100).astype(np.float16),
          np.zeros(dim, np.float16)]
    sub = np.full(dim, np.float16(6e-6))  # subnormal fp16
    big = np.where(np.arange(dim) % 2 == 0, np.float16(65504), np.float16(-65504))
    return vs + [sub, big]


@pytest.mark.parametrize("dim", [1, 3, 4, 7, 13, 100])
def test_f16_restatement_equals_oracle_unroll4(dim):
    rng = np.random.default_rng(dim)
    vs = _vectors(rng, dim)
    for a in vs:
        flat = np.stack(vs).astype(F)
        for metric, fn in ((0, euclidean_f16_unrolled4x), (1, cosine_f16_unrolled4x), (2, dot_f16_unrolled4x)):
            want = np.array([fn(a, b) for b in vs], F)
            if metric == 2:
                want = -want  # the index ranks by the negated dot product (distance_resolvers.go)
            got = oc.batch_flat(metric, a.astype(F), flat, oc.UNROLL4)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) or np.array_equal(got, want, equal_nan=True), \
                f"metric {metric} dim {dim}: {got} vs {want}"


def test_cosine_zero_vector_is_one():
    z = np.zeros(8, np.float16)
    assert cosine_f16_unrolled4x(z, np.ones(8, np.float16)) == F(1)
    assert oc.batch_flat(1, z.astype(F), np.ones((1, 8), F), oc.UNROLL4)[0] == F(1)


F16_SYMBOLS = ["lb_gpu_index_new_f16", "lb_gpu_index_dtype", "lb_gpu_index_add_f16", "lb_gpu_index_add_f16_device",
               "lb_gpu_index_search_f16", "lb_gpu_index_search_f16_ctx", "lb_gpu_index_search_f16_device_ctx",
               "lb_gpu_index_hbm_bytes"]


def test_f16_symbols_exported():
    from longbow_amd import _lib
    lib = _lib.load()
    for name in F16_SYMBOLS:
        assert hasattr(lib, name), name
    raw = C.CDLL(lib._name)
    for name in F16_SYMBOLS:
        getattr(raw, name)  # AttributeError when the symbol is missing


def test_f16_null_handle_calls():
    from longbow_amd import _lib
    lib = _lib.load()
    assert lib.lb_gpu_index_dtype(None) == 0
    assert lib.lb_gpu_index_hbm_bytes(None) == 0
    assert lib.lb_gpu_index_add_f16(None, 1, None, None) == 1
    assert lib.lb_gpu_index_search_f16(None, 1, None, 1, None, None) == 1
    st = C.c_int(-1)
    assert not lib.lb_gpu_index_new_f16(0, 0, 0, C.byref(st)) and st.value == 1  # dim <= 0: before any device is asked


def test_python_validates_data_type_before_the_device():
    from longbow_amd import gpu
    with pytest.raises(ValueError):
        gpu.Index(gpu.GPUConfig(DeviceID=0, Dimension=8, DataType=7))
    assert gpu.GPUConfig().DataType == gpu.DataType.Float32


def test_python_f16_index_takes_float16_arrays_only():
    from longbow_amd import gpu
    idx = gpu.Index.__new__(gpu.Index)  # no device: only the element check runs
    idx._np = np.float16
    with pytest.raises(TypeError):
        idx._as_elems(np.zeros(4, np.float32))
    assert idx._as_elems(np.zeros(4, np.float16)).dtype == np.float16


def test_arrow_halffloat_column_checks():
    pa = pytest.importorskip("pyarrow")
    from longbow_amd import arrow_io
    x = np.arange(12, dtype=np.float16)
    col16 = pa.FixedSizeListArray.from_arrays(pa.array(x, pa.float16()), 4)
    col32 = pa.FixedSizeListArray.from_arrays(pa.array(x.astype(F), pa.float32()), 4)
    got = arrow_io._vector_values(col16, 4, f16=True)
    assert got.dtype == np.float16 and np.array_equal(got.reshape(-1), x)
    with pytest.raises(arrow_io.ExchangeError):
        arrow_io._vector_values(col32, 4, f16=True)
    assert arrow_io._vector_values(col32, 4).dtype == F  # the f32 path is unchanged
