"""Scalar-quantisation semantics, no device needed: tests/sq8_oracle.py against the reference tests' own literals
(tests/golden/sq8_kats.json) and against hand-computed values."""
import numpy as np
import pytest

from tests import sq8_oracle as so

F = np.float32


def test_oracle_reproduces_every_golden_case():
    k = so.load_kats()
    e = k["encode"]
    assert len(e["cases"]) == 5
    for c in e["cases"]:
        assert so.encode(F(c["input"]), e["min"], e["max"]).tolist() == c["expect"], c["name"]
    d = k["decode_ranges"]
    for c in d["cases"]:
        v = so.decode(np.uint8(c["input"]), d["min"], d["max"])
        assert ((v >= F(c["lo"])) & (v <= F(c["hi"]))).all(), c["name"]
    r = k["round_trip"]
    orig = F(r["original"])
    back = so.decode(so.encode(orig, r["min"], r["max"]), r["min"], r["max"])
    max_error = F(r["max_error_num"] / r["max_error_den"])
    assert (np.abs(orig.astype(np.float64) - back.astype(np.float64)).astype(F) <= max_error * F(r["allow"])).all()
    t = k["distance"]
    q1, q2, q3 = (so.encode(F(t[n]), t["min"], t["max"]) for n in ("v1", "v2", "v3"))
    eu = lambda a, b: so.euclid(a, b, t["min"], t["max"])[0]
    assert eu(q1, q1) <= t["d11_max"]
    assert t["d12"][0] <= eu(q1, q2) <= t["d12"][1]
    assert t["d13"][0] <= eu(q1, q3) <= t["d13"][1]
    assert t["d23"][0] <= eu(q2, q3) <= t["d23"][1]
    for c in k["distance_fast"]["cases"]:
        assert int(so.dist_s(c["a"], [c["b"]])[0]) == c["expected"]
    z = k["quantize"]
    n = len(z["src"])
    assert so.encode(F(z["src"]), np.full(n, z["min"], F), np.full(n, z["max"], F)).tolist() == z["expect"]
    cases = k["euclidean_sizes"]["cases"]
    assert sorted(c["size"] for c in cases) == [0, 5, 32, 33, 127, 1024]
    for c in cases:
        assert c["a"].size == c["size"] == c["b"].size
        assert int(so.dist_s(c["a"], c["b"].reshape(1, -1))[0]) == c["expected"], c["name"]


def test_constant_column_trains_at_one_and_fails_at_two():
    mn, mx = so.train(np.full((3, 2), 1.0, F))
    assert (mn == F(1.0)).all() and (mx == F(1.0) + F(1e-7)).all() and (mx > mn).all()
    assert F(2.0) + F(1e-7) == F(2.0)  # the epsilon is below half an ulp from 2.0 up
    with pytest.raises(ValueError, match="min must be less than max"):
        so.train(np.full((3, 2), 2.0, F))
    with pytest.raises(ValueError, match="min must be less than max"):
        so.train(np.array([[0.5, -4.0]], F))  # one row: every column is constant
    with pytest.raises(ValueError, match="no vectors"):
        so.train(np.zeros((0, 4), F))
    with pytest.raises(ValueError, match="zero dimensions"):
        so.train(np.zeros((4, 0), F))


def test_nan_in_row_zero_stays_and_a_later_nan_is_ignored():
    nan = F(np.nan)
    X = np.array([[nan, 1.0, 3.0], [2.0, nan, 1.0], [5.0, 4.0, nan], [-1.0, 0.0, 2.0]], F)
    mn, mx = so.train(X)  # NaN bounds pass Validate
    assert np.isnan(mn[0]) and np.isnan(mx[0])
    assert (mn[1:] == F([0.0, 1.0])).all() and (mx[1:] == F([4.0, 3.0])).all()
    # a NaN bound makes every product NaN: code 0; decode gives NaN
    assert (so.encode(X, mn, mx)[:, 0] == 0).all()
    assert np.isnan(so.decode(np.uint8([[7, 7, 7]]), mn, mx)[0, 0])


def test_encode_of_special_values():
    tiny = F(1e-45)
    mn, mx = F([-1.0] * 8), F([1.0] * 8)
    v = np.array([np.nan, np.inf, -np.inf, tiny, -tiny, np.finfo(F).tiny, -1.0, 1.0], F)
    # NaN passes both comparisons and its product converts to 0; the infinities clamp; denormals are not flushed
    assert so.encode(v, mn, mx).tolist() == [0, 255, 0, 127, 127, 127, 0, 255]
    # a denormal difference under a large scale: flushing it to zero would give code 0
    mn, mx = F([0.0] * 4), F([2.0 ** -119] * 4)
    den = F(0.75 * 2.0 ** -126)
    assert 0 < den < np.finfo(F).tiny and np.isfinite(so.params(mn, mx)[0]).all()
    assert so.encode(F([0.0, den, 2.0 ** -120, 2.0 ** -119]), mn, mx).tolist() == [0, 1, 127, 255]
    # bounds so close that scale overflows: 0 * inf is NaN, x * inf is inf, both convert to 0 (the amd64 conversion)
    mn, mx = F([0.0] * 2), F([1e-45] * 2)
    assert np.isinf(so.params(mn, mx)[0]).all()
    assert so.encode(F([0.0, 1e-45]), mn, mx).tolist() == [0, 0]


def test_the_sign_of_a_zero_bound_changes_nothing():
    X = np.array([[-0.0, 0.0, 0.3], [0.0, -0.0, -0.2], [0.7, -0.5, 0.0], [-0.3, 0.2, -0.0]], F)
    rng = np.random.default_rng(5)
    V = np.concatenate([X, (rng.random((50, 3), dtype=F) * F(2) - F(1)).astype(F)])
    codes = np.arange(256, dtype=np.uint8).repeat(3).reshape(256, 3)
    outs = []
    for z0 in (F(0.0), F(-0.0)):
        mn, mx = F([z0, -0.5, -0.2]), F([0.7, z0, 0.3])
        outs.append((so.encode(V, mn, mx), so.decode(codes, mn, mx)))
    assert np.array_equal(outs[0][0], outs[1][0])
    assert np.array_equal(outs[0][1], outs[1][1])  # compares equal: a decoded zero may differ in sign only
    # training itself: the bound compares equal whichever zero came first
    a, b = so.train(X), so.train(X[::-1])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_float32_of_s_merges_neighbours_but_the_order_is_the_integers():
    dims = 300
    codes = np.zeros((3, dims), np.uint8)
    q = np.zeros(dims, np.uint8)
    # three rows whose S are 2^24 + 1, 2^24, 2^24 + 2 -> float32 gives 2^24, 2^24, 2^24 + 2
    base = 258 * 65025  # 16776450

    def row(extra):  # S = base + extra, extra spread over further dimensions as squares
        r = np.zeros(dims, np.uint8)
        r[:258] = 255
        i = 258
        while extra > 0:
            d = min(255, int(np.sqrt(extra)))
            r[i] = d
            extra -= d * d
            i += 1
        return r
    want = [(1 << 24) + 1, 1 << 24, (1 << 24) + 2]
    for j, s in enumerate(want):
        codes[j] = row(s - base)
    assert so.dist_s(q, codes).tolist() == want
    labels, dist = so.topk(so.dist_s(q, codes), 3)
    assert labels.tolist() == [1, 0, 2]
    assert dist[0] == dist[1] == F(1 << 24) and dist[2] == F((1 << 24) + 2)


def test_search_oracle_equals_the_direct_sum():
    rng = np.random.default_rng(9)
    codes = rng.integers(0, 256, (500, 37), dtype=np.uint8)
    Q = rng.integers(0, 256, (4, 37), dtype=np.uint8)
    labels, dist = so.search(Q, codes, 20)
    for i in range(4):
        l, d = so.topk(so.dist_s(Q[i], codes), 20)
        assert np.array_equal(labels[i], l) and np.array_equal(dist[i], d)
