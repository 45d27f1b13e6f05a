// kernels_countsel.hip -- the two launches of the top-k by counting (lb_countsel.h) that need no distance: the scan of the
// per-workgroup counts and the finish.
#include "lb_countsel.h"

#include <cfloat>

namespace lb {

namespace {

// cnt[q][b][2] -> exclusive prefix over b, in place; tot[q] = rows below t
__global__ __launch_bounds__(256) void countsel_scan_kernel(CountSel a)
{
    __shared__ uint32_t part[256][2];
    const int tid = threadIdx.x, q = blockIdx.x;
    const int per = (a.nblk + 255) / 256;
    uint32_t *c = a.cnt + (int64_t)q * a.nblk * 2;
    const int b0 = tid * per < a.nblk ? tid * per : a.nblk, b1 = b0 + per < a.nblk ? b0 + per : a.nblk;
    uint32_t s0 = 0, s1 = 0;
    for (int b = b0; b < b1; b++) {
        s0 += c[2 * b];
        s1 += c[2 * b + 1];
    }
    part[tid][0] = s0;
    part[tid][1] = s1;
    __syncthreads();
    if (tid == 0) {
        uint32_t r0 = 0, r1 = 0;
        for (int i = 0; i < 256; i++) {
            const uint32_t v0 = part[i][0], v1 = part[i][1];
            part[i][0] = r0;
            part[i][1] = r1;
            r0 += v0;
            r1 += v1;
        }
        a.tot[q] = r0;
    }
    __syncthreads();
    s0 = part[tid][0];
    s1 = part[tid][1];
    for (int b = b0; b < b1; b++) {
        const uint32_t v0 = c[2 * b], v1 = c[2 * b + 1];
        c[2 * b] = s0;
        c[2 * b + 1] = s1;
        s0 += v0;
        s1 += v1;
    }
}

// the min(k, n) keys of a query, ascending by (distance, position) -> float32(distance) / labels, padded with FLT_MAX / -1;
// under a list of visible rows (posmap) the label is the row behind the position
__global__ __launch_bounds__(SEL_THREADS) void countsel_finish_kernel(CountSel a, float *dist, int64_t *labels, const uint32_t *posmap)
{
    __shared__ uint64_t sh[2048];
    const int tid = threadIdx.x, q = blockIdx.x;
    const uint32_t have = a.n < (int64_t)a.k ? (uint32_t)a.n : (uint32_t)a.k;
    const uint32_t P = next_pow2((uint32_t)a.k);
    for (uint32_t i = tid; i < P; i += SEL_THREADS) sh[i] = i < have ? a.keys[(int64_t)q * a.k + i] : ~0ull;
    __syncthreads();
    bitonic_sort_u64(sh, P, tid, SEL_THREADS);
    for (uint32_t i = tid; i < (uint32_t)a.k; i += SEL_THREADS) {
        const uint64_t key = sh[i];
        const bool pad = i >= have;
        dist[(int64_t)q * a.k + i] = pad ? FLT_MAX : (float)(uint32_t)(key >> 32);
        int64_t label = -1;
        if (!pad) {
            const uint32_t pos = (uint32_t)(key & 0xffffffffull);
            label = posmap ? (int64_t)posmap[pos] : (int64_t)pos; // (the emit wrote all `have` keys: every position is below n)
        }
        labels[(int64_t)q * a.k + i] = label;
    }
}

} // namespace

void countsel_plan(int64_t n, int max_blocks, int *nblk, int *tpb)
{
    const int64_t ntiles = (n + COUNTSEL_ROWS - 1) / COUNTSEL_ROWS;
    const int64_t per = (ntiles + max_blocks - 1) / max_blocks;
    *tpb = (int)(per < 1 ? 1 : per);
    *nblk = (int)((ntiles + *tpb - 1) / *tpb);
}

void launch_countsel_scan(const CountSel &a, hipStream_t s) { countsel_scan_kernel<<<dim3((unsigned)a.nq), dim3(256), 0, s>>>(a); }

void launch_countsel_finish(const CountSel &a, float *dist, int64_t *labels, hipStream_t s, const uint32_t *posmap)
{
    countsel_finish_kernel<<<dim3((unsigned)a.nq), dim3(SEL_THREADS), 0, s>>>(a, dist, labels, posmap);
}

} // namespace lb
