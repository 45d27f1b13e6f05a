"""Plain-numpy restatement of store.BQEncoder (internal/store/binary_quantization.go) and simd.HammingDistance
(internal/simd/simd_bitops.go:40-55): what the lb_gpu_bq_* entry points must reproduce bit for bit."""
import math

import numpy as np

FLT_MAX = np.finfo(np.float32).max


def words(dims):
    """CodeSize (binary_quantization.go:63-65)"""
    return (dims + 63) // 64


def encode(v):
    """Encode (binary_quantization.go:24-48): bit i % 64 of word i // 64 is set iff v[i] > 0; pad bits are zero.
    [n, dims] f32 -> [n, W] uint64 (a 1-D vector -> [W])."""
    v = np.asarray(v, np.float32)
    single = v.ndim == 1
    v = v.reshape(-1, v.shape[-1])
    with np.errstate(invalid="ignore"):
        bits = v > 0
    pad = words(v.shape[1]) * 64 - v.shape[1]
    bits = np.pad(bits, ((0, 0), (0, pad)))
    codes = np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little")).view("<u8").astype(np.uint64)
    return codes[0] if single else codes


def decode(codes, dims):
    """Decode (binary_quantization.go:80-92): bit 1 -> 1.0, bit 0 -> -1.0"""
    c = np.ascontiguousarray(np.asarray(codes, np.uint64).reshape(-1, words(dims))).astype("<u8")
    bits = np.unpackbits(c.view(np.uint8), axis=1, bitorder="little")[:, :dims]
    return np.where(bits == 1, np.float32(1.0), np.float32(-1.0)).astype(np.float32)


def hamming(q, codes):
    """HammingDistanceBatch: popcount of the XOR over all whole words.  q [W], codes [n, W] -> int32 [n]"""
    q = np.asarray(q, np.uint64).reshape(1, -1)
    codes = np.asarray(codes, np.uint64)
    if q.shape[1] == 0:  # simd.HammingDistance of two empty slices
        return np.zeros(codes.shape[0] if codes.ndim == 2 else 1, np.int32)
    codes = codes.reshape(-1, q.shape[1])
    return np.bitwise_count(codes ^ q).sum(axis=1, dtype=np.int64).astype(np.int32)


def topk(d, k):
    """ascending by (distance, position); fewer than k rows: label -1, dist FLT_MAX"""
    d = np.asarray(d)
    order = np.lexsort((np.arange(d.size), d))[:k]
    labels = np.full(k, -1, np.int64)
    dist = np.full(k, FLT_MAX, np.float32)
    labels[:order.size] = order
    dist[:order.size] = d[order].astype(np.float32)
    return labels, dist


def search(qcodes, codes, k):
    """exact k-NN of each query code over codes -> (labels [nq, k], dist [nq, k])"""
    qcodes = np.asarray(qcodes, np.uint64)
    qcodes = qcodes.reshape(-1, qcodes.shape[-1])
    labels = np.empty((qcodes.shape[0], k), np.int64)
    dist = np.empty((qcodes.shape[0], k), np.float32)
    for i, q in enumerate(qcodes):
        labels[i], dist[i] = topk(hamming(q, codes), k)
    return labels, dist


def score(h, dims):
    """ScoreToFloat32 (binary_quantization.go:69-71): 1.0 - float32(h) / float32(dims) in f32 operations"""
    return (np.float32(1.0) - np.asarray(h).astype(np.float32) / np.float32(dims)).astype(np.float32)


def float32_to_hamming(s, dims):
    """Float32ToHamming (binary_quantization.go:74-76)"""
    return int(math.floor(float(dims) * (1.0 - float(np.float32(s)))))


def load_kats():
    """tests/golden/bq_kats.json -> (encode cases [(name, vector f32, codes u64)], hamming cases [(name, a u64, b u64, expected)]),
    the a[i] = i, b[i] = ~i alignment cases expanded"""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bq_kats.json")) as f:
        kats = json.load(f)
    u64 = lambda ws: np.array([int(w, 16) for w in ws], np.uint64)
    enc = []
    for c in kats["encode"]:
        v = np.full(c["dims"], c["fill"], np.float32)
        for i, x in c["set"].items():
            v[int(i)] = x
        enc.append((c["name"], v, u64(c["codes"])))
    ham = [(c["name"], u64(c["a"]), u64(c["b"]), c["expected"]) for c in kats["hamming"]]
    for n in kats["alignments"]["lengths"]:
        a = np.arange(n, dtype=np.uint64)
        ham.append((f"alignment {n}", a, ~a, 64 * n))
    return enc, ham
