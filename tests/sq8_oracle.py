"""Plain-numpy restatement of store.SQ8Encoder (internal/store/scalar_quantization.go) and simd.EuclideanSQ8Generic
(internal/simd/sq8.go:45-66): what the lb_gpu_sq8_* entry points must reproduce bit for bit.  Every f32 operation is one numpy
f32 operation (one rounding); sums are sequential where the reference's are."""
import numpy as np

F = np.float32
FLT_MAX = np.finfo(np.float32).max
INT32_MAX = 0x7FFFFFFF


def validate(mn, mx):
    """SQ8Config.Validate (scalar_quantization.go:44-49): NaN bounds pass"""
    with np.errstate(invalid="ignore"):
        if (np.asarray(mn, F) >= np.asarray(mx, F)).any():
            raise ValueError("min must be less than max for all dimensions")


def train(X):
    """TrainSQ8Encoder (scalar_quantization.go:89-134) -> (min, max); raises as the reference errors"""
    X = np.asarray(X, F)
    if X.ndim != 2 or X.shape[0] == 0:
        raise ValueError("no vectors provided for training")
    if X.shape[1] == 0:
        raise ValueError("vectors have zero dimensions")
    mn, mx = X[0].copy(), X[0].copy()
    with np.errstate(invalid="ignore"):
        for v in X[1:]:
            lo, hi = v < mn, v > mx
            mn[lo] = v[lo]
            mx[hi] = v[hi]
        same = mn == mx
        mx[same] = (mn[same] + F(1e-7)).astype(F)
    validate(mn, mx)
    return mn, mx


def params(mn, mx):
    """NewSQ8Encoder (scalar_quantization.go:75-79) -> (scale, invScale), f32 divisions"""
    mn, mx = np.asarray(mn, F), np.asarray(mx, F)
    with np.errstate(all="ignore"):
        rng = (mx - mn).astype(F)
        return (F(255.0) / rng).astype(F), (rng / F(255.0)).astype(F)


def encode(X, mn, mx):
    """EncodeInto (scalar_quantization.go:155-170).  uint8(f) as amd64 converts: truncate to int32 and keep the low byte; a
    NaN or a value beyond int32 gives 0.  [n, dims] f32 -> [n, dims] uint8 (a 1-D vector -> [dims])."""
    X = np.asarray(X, F)
    mn, mx = np.asarray(mn, F), np.asarray(mx, F)
    scale, _ = params(mn, mx)
    with np.errstate(all="ignore"):
        v = np.where(X < mn, mn, np.where(X > mx, mx, X)).astype(F)
        p = ((v - mn).astype(F) * scale).astype(F)
        ok = (p >= F(-2147483648.0)) & (p < F(2147483648.0))
        t = np.trunc(np.where(ok, p, F(0))).astype(np.int64)
    return (t & 255).astype(np.uint8)


def decode(codes, mn, mx):
    """DecodeInto (scalar_quantization.go:180-184): min + float32(q) * invScale, the product rounded first"""
    mn = np.asarray(mn, F)
    _, inv = params(mn, mx)
    with np.errstate(all="ignore"):
        return (mn + (np.asarray(codes, np.uint8).astype(F) * inv).astype(F)).astype(F)


def dist_s(q, codes):
    """EuclideanSQ8Generic / SQ8DistanceFast: sum (a_i - b_i)^2.  q [dims], codes [n, dims] -> int32 [n]"""
    q = np.asarray(q, np.uint8).astype(np.int64).reshape(1, -1)
    c = np.asarray(codes, np.uint8).astype(np.int64)
    if q.shape[1] == 0:  # EuclideanSQ8Generic of two empty slices
        return np.zeros(c.shape[0] if c.ndim == 2 else 1, np.int32)
    c = c.reshape(-1, q.shape[1])
    d = c - q
    s = (d * d).sum(axis=1)
    assert (s <= INT32_MAX).all()
    return s.astype(np.int32)


def euclid(q, codes, mn, mx):
    """SQ8EuclideanDistance (scalar_quantization.go:192-203) of q against each row: the f32 sum runs over i in order"""
    v1 = decode(np.asarray(q, np.uint8).reshape(1, -1), mn, mx)
    v2 = decode(np.asarray(codes, np.uint8).reshape(-1, v1.shape[1]), mn, mx)
    total = np.zeros(v2.shape[0], F)
    with np.errstate(all="ignore"):
        for i in range(v1.shape[1]):
            diff = (v1[:, i] - v2[:, i]).astype(F)
            total = (total + (diff * diff).astype(F)).astype(F)
        return np.sqrt(total.astype(np.float64)).astype(F)


def topk(s, k):
    """ascending by (S, position), reported as float32(S); fewer than k rows: label -1, dist FLT_MAX"""
    s = np.asarray(s)
    order = np.lexsort((np.arange(s.size), s))[:k]
    labels = np.full(k, -1, np.int64)
    dist = np.full(k, FLT_MAX, F)
    labels[:order.size] = order
    dist[:order.size] = s[order].astype(F)
    return labels, dist


def dist_matrix(qcodes, codes):
    """dist_s of every query against every row as one matrix product: |x|^2 + |q|^2 - 2 x.q, every term an integer below
    2^53 in float64, so the result is the same integer as the sum of squared differences.  -> int64 [nq, n]"""
    q = np.asarray(qcodes, np.uint8)
    q = q.reshape(-1, q.shape[-1]).astype(np.float64)
    c = np.asarray(codes, np.uint8).reshape(-1, q.shape[1]).astype(np.float64)
    return ((c * c).sum(axis=1)[None, :] + (q * q).sum(axis=1)[:, None] - 2.0 * (q @ c.T)).astype(np.int64)


def search(qcodes, codes, k):
    """exact k-NN of each query code over codes -> (labels [nq, k], dist [nq, k])"""
    S = dist_matrix(qcodes, codes)
    labels = np.empty((S.shape[0], k), np.int64)
    dist = np.empty((S.shape[0], k), F)
    for i, s in enumerate(S):
        labels[i], dist[i] = topk(s, k)
    return labels, dist


def load_kats():
    """tests/golden/sq8_kats.json as a dict, the byte strings of the size cases decoded to uint8 arrays"""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sq8_kats.json")) as f:
        kats = json.load(f)
    for c in kats["euclidean_sizes"]["cases"]:
        c["a"] = np.frombuffer(bytes.fromhex(c["a"]), np.uint8)
        c["b"] = np.frombuffer(bytes.fromhex(c["b"]), np.uint8)
    return kats
