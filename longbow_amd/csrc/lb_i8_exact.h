// lb_i8_exact.h -- the int8 arithmetic of one (row, query) pair, defined once for kernels_i8.hip (the flat int8 index) and
// kernels_ivf_i8.hip (the list scan of an IVF-Flat handle over int8 rows).  It is the reference's DataTypeInt8 registry kernels
// (internal/simd/dispatch.go:241-242; the forms are spelled out at the head of kernels_i8.hip).  Device-only; a file that
// includes it compiles with fp contraction off.
#pragma once
#include "lb_device.h"

namespace lb {

// ---- the reference value of one pair, one lane, straight from memory (any D) ----------------------------------------
// QT: the queries' element type, int8_t or float holding int8 values (the flat index's scan reads its queries widened).
// returns the reported distance: L2 the value, dot -value
template <int METRIC, class QT>
__device__ __forceinline__ float i8_pair_distance(const int8_t *x, const QT *q, int D)
{
    if (METRIC == METRIC_L2) {
        const int m = D & ~15;
        int s = 0;
        for (int i = 0; i < m; i++) {
            const int e = (int)x[i] - (int)q[i];
            s += e * e;
        }
        float f = (float)s; // VCVTDQ2PS: round to nearest
        for (int i = m; i < D; i++) {
            const int e = (int)x[i] - (int)q[i];
            f = f + (float)(e * e); // CVTSI2SS + ADDSS, in order
        }
        return (float)sqrt((double)f); // VSQRTSS: correctly rounded
    } else {
        int p0 = 0, p1 = 0, p2 = 0, p3 = 0; // the four f32 chains, exact integers (|p| <= 2^24 by the dimension limit)
        const int m4 = D & ~3;
        for (int i = 0; i < m4; i += 4) {
            p0 += (int)x[i] * (int)q[i];
            p1 += (int)x[i + 1] * (int)q[i + 1];
            p2 += (int)x[i + 2] * (int)q[i + 2];
            p3 += (int)x[i + 3] * (int)q[i + 3];
        }
        for (int i = m4; i < D; i++) p0 += (int)x[i] * (int)q[i];
        float t = (float)p0 + (float)p1;
        t = t + (float)p2;
        t = t + (float)p3;
        return -t;
    }
}

} // namespace lb
