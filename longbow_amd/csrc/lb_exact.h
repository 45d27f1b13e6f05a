// lb_exact.h -- the reference's exact f32 arithmetic, stated once for every kernel whose results must equal it bit for bit:
//   SEQ     referenceEuclidean/referenceCosine (internal/simd/simd_test.go:13-33), cosineGeneric/dotGeneric (simd.go:138-163)
//   UNROLL4 euclideanUnrolled4x/cosineUnrolled4x/dotUnrolled4x (internal/simd/simd.go:365-479)
// Every f32 operation is one IEEE rounding.  Each helper turns FMA contraction off in its own body -- there is no file-scope
// pragma here, so including this header changes nothing else in a file.  A product that a caller forms and a helper sums
// must be formed in an off region as well.
#pragma once
#include "lb_device.h"

namespace lb {

// f32 accumulator chain(s) in the reference's order.  SEQ: one chain.  UNROLL4: element T of each group of four goes to chain
// T, the elements beyond the last whole group to chain 0, and the total is ((s0 + s1) + s2) + s3.
template <int ORDER>
struct Acc {
    float s[ORDER == ORDER_UNROLL4 ? 4 : 1];
    __device__ __forceinline__ void zero()
    {
#pragma unroll
        for (int i = 0; i < (ORDER == ORDER_UNROLL4 ? 4 : 1); i++) s[i] = 0.f;
    }
    template <int T>
    __device__ __forceinline__ void add(float v)
    {
#pragma clang fp contract(off)
        if (ORDER == ORDER_UNROLL4) s[T] = s[T] + v;
        else s[0] = s[0] + v;
    }
    __device__ __forceinline__ void add_tail(float v)
    {
#pragma clang fp contract(off)
        s[0] = s[0] + v;
    }
    // one group of four elements of sum x * x
    __device__ __forceinline__ void add4_sq(const f32x4 x)
    {
#pragma clang fp contract(off)
        add<0>(x.x * x.x);
        add<1>(x.y * x.y);
        add<2>(x.z * x.z);
        add<3>(x.w * x.w);
    }
    // one group of four elements of the metric's pair sum: (q - x)^2 (L2) or q * x (cosine, dot)
    template <int METRIC>
    __device__ __forceinline__ void add4_pair(const f32x4 q, const f32x4 x)
    {
#pragma clang fp contract(off)
        if (METRIC == METRIC_L2) {
            const float e0 = q.x - x.x, e1 = q.y - x.y, e2 = q.z - x.z, e3 = q.w - x.w;
            add<0>(e0 * e0);
            add<1>(e1 * e1);
            add<2>(e2 * e2);
            add<3>(e3 * e3);
        } else {
            add<0>(q.x * x.x);
            add<1>(q.y * x.y);
            add<2>(q.z * x.z);
            add<3>(q.w * x.w);
        }
    }
    __device__ __forceinline__ float total() const
    {
#pragma clang fp contract(off)
        if (ORDER == ORDER_UNROLL4) {
            float t = s[0] + s[1];
            t = t + s[2];
            t = t + s[3];
            return t;
        }
        return s[0];
    }
};

// ||q||^2 in the reference's order, q in LDS (16-B aligned; elements beyond D are not read), one lane
template <int ORDER>
__device__ __forceinline__ float exact_sq_norm_lds(const float *sq, int D)
{
#pragma clang fp contract(off)
    Acc<ORDER> a;
    a.zero();
    const int dmain = D & ~3;
#pragma unroll 8
    for (int i = 0; i < dmain; i += 4) a.add4_sq(*reinterpret_cast<const f32x4 *>(&sq[i]));
    for (int i = dmain; i < D; i++) a.add_tail(sq[i] * sq[i]);
    return a.total();
}
__device__ __forceinline__ float exact_sq_norm_lds(const float *sq, int D, int order)
{
    return order == ORDER_UNROLL4 ? exact_sq_norm_lds<ORDER_UNROLL4>(sq, D) : exact_sq_norm_lds<ORDER_SEQ>(sq, D);
}

// The sums of one (row, query) pair, one lane, straight from memory (any D, any alignment): t = the metric's pair sum,
// nbt = ||x||^2 (cosine; 0 otherwise).  exact_distance turns them into the result.
// (T = _Float16: an fp16 index's row, each element widened to f32 exactly)
template <int METRIC, int ORDER, typename T>
__device__ __forceinline__ void exact_pair_sums(const T *x, const float *q, int D, float &t, float &nbt)
{
#pragma clang fp contract(off)
    Acc<ORDER> acc, nb;
    acc.zero();
    nb.zero();
    const int dmain = D & ~3;
    for (int i = 0; i < dmain; i += 4) {
        const f32x4 xv = {(float)x[i], (float)x[i + 1], (float)x[i + 2], (float)x[i + 3]};
        const f32x4 qv = {q[i], q[i + 1], q[i + 2], q[i + 3]};
        if (METRIC == METRIC_COS) nb.add4_sq(xv);
        acc.template add4_pair<METRIC>(qv, xv);
    }
    for (int i = dmain; i < D; i++) {
        const float xv = (float)x[i], qv = q[i];
        if (METRIC == METRIC_COS) nb.add_tail(xv * xv);
        if (METRIC == METRIC_L2) {
            const float e = qv - xv;
            acc.add_tail(e * e);
        } else {
            acc.add_tail(qv * xv);
        }
    }
    t = acc.total();
    nbt = nb.total();
}

// The reported distance from the sums (t: pair sum, nbt: ||x||^2, na: ||q||^2): L2 sqrt((double)t); cosine
// 1 - t / sqrt(na nb), or 1 when D or either norm is 0; dot -t (raw_dot: t itself, as simd.DotProductBatch reports it).
template <int METRIC>
__device__ __forceinline__ float exact_distance(float t, float nbt, float na, int D, bool raw_dot)
{
#pragma clang fp contract(off)
    float dist;
    if (METRIC == METRIC_L2) {
        dist = (float)sqrt((double)t);
    } else if (METRIC == METRIC_COS) {
        if (D == 0 || na == 0.0f || nbt == 0.0f) dist = 1.0f;
        else dist = 1.0f - __fdiv_rn(t, (float)sqrt((double)na * (double)nbt));
    } else {
        dist = raw_dot ? t : -t;
    }
    return dist;
}

// ---- ADC (simd.adcBatchGeneric, internal/simd/simd.go:345-355) ------------------------------------------------------------------
// out = float32(sqrt(float64(sum_j table[j * 256 + code[j]]))): an f32 sum in j order, one rounding per addition.  Every kernel
// that reports an exact ADC distance (kernels_pq.hip, kernels_pq_list.hip, kernels_ivfpq.hip) sums and roots through these.
// sixteen code bytes, j = g * 16 .. g * 16 + 15, as one 16-byte piece of the row
__device__ __forceinline__ float adc_add16(float sum, const float *tab, int g, const uint4 v)
{
#pragma clang fp contract(off)
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
        for (int b = 0; b < 4; b++) sum = sum + tab[(g * 16 + t * 4 + b) * 256 + ((w[t] >> (8 * b)) & 0xffu)];
    return sum;
}

// the M code bytes at c, one at a time
__device__ __forceinline__ float adc_add_bytes(float sum, const float *tab, const uint8_t *c, int M)
{
#pragma clang fp contract(off)
    for (int j = 0; j < M; j++) sum = sum + tab[j * 256 + c[j]];
    return sum;
}

// one row's sum straight from its M code bytes at c: 16-byte loads (M % 16 == 0, c 16-byte aligned) or single bytes
template <bool VEC16> __device__ __forceinline__ float adc_row_sum(const float *tab, const uint8_t *c, int M)
{
    float sum = 0.f;
    if (VEC16) {
        for (int g = 0; g < M / 16; g++) sum = adc_add16(sum, tab, g, *reinterpret_cast<const uint4 *>(c + g * 16));
    } else {
        sum = adc_add_bytes(sum, tab, c, M);
    }
    return sum;
}

__device__ __forceinline__ float adc_distance(float sum) { return (float)sqrt((double)sum); }

} // namespace lb
