// kernels_ivf_train.hip -- the E-step of lb_gpu_ivf_train: pq.TrainKMeans' assignment loop (internal/pq/kmeans.go:91-108) at
// the coarse quantiser's shape, whole rows against up to 65,536 centroids.  The ordering is launch_ivf_sort (kernels_ivf.hip)
// and the M-step, the finish step and the init are kernels_pq_train.hip's over a KmState with M = 1 and sub = D; what is here
// is the tile that replaces km_estep_generic_kernel, and the step that turns the sort's offsets into the M-step's counts.
//
// The tile.  A 256-thread workgroup owns 64 rows and walks the centroid tiles of 64 in ascending order; per (centroid tile,
// chunk of 64 elements) one LDS stage [64 row chunks | 64 centroid chunks], padded to IT_LD floats a row, with the next
// stage's global loads held in registers meanwhile (ivf_scan_kernel's pipeline).  Lane (ty, tx) = (tid / 16, tid % 16) keeps
// the 4 x 4 pairs of rows ty + 16 i and centroids tx + 16 j, each pair its own Acc<ORDER_UNROLL4>: 64 accumulators.  A group
// of four elements is 8 ds_read_b128 for 192 sub / mul / add per lane.  The centroid reads of a 16-lane LDS group hit 16
// different 16-byte bank groups (tx * IT_LD * 4 B = tx * 16 B mod 256 B) and the row reads are two broadcasts: conflict-free.
//
// The first strict minimum as an integer minimum.  The reference keeps `best`, starting at FLT_MAX, and moves a row to c when
// dist_c < best: the row ends at the lowest c among those with the lowest dist, provided that dist is below FLT_MAX.  Here
// dist_c = s is a sum of squares accumulated from +0: every square is >= +0 or NaN, and +0 + +0 = +0, so s is never negative
// and never -0, and for such floats a < b  <=>  bits(a) < bits(b) as uint32.  With key_c = bits(s) << 32 | c for an admissible
// s (s < FLT_MAX, which is false for NaN and +inf) and ~0 otherwise, the minimum key over all c has the lowest s and among
// equal s the lowest c: the reference's answer, in whatever order the c are visited.  (An admissible key is below ~0 because
// bits(s) < bits(FLT_MAX).)  A row whose minimum stays ~0 has no admissible centroid: it gets -1 and raises `bad`.
#include "lb_exact.h"
#include "lb_ivf.h"

#pragma clang fp contract(off)

namespace lb {

constexpr int IT_THREADS = 256;
constexpr int IT_ROWS = 64;        // rows per workgroup
constexpr int IT_CENTS = 64;       // centroids per tile
constexpr int IT_DK = 64;          // floats per row per stage
constexpr int IT_LD = IT_DK + 4;   // padded LDS row stride (floats): conflict-free ds_read_b128
constexpr int IT_PER = 4;          // rows, and centroids, per lane; also 16-byte staging pieces per lane and operand
constexpr float IT_FLT_MAX = 3.40282346638528859811704183484516925e+38f;

// four floats of `base` from element k; VEC: D % 4 == 0 and 16-byte aligned rows (a piece past D is never consumed: it is moved
// inside the row).  Otherwise element by element, zero past D.
template <bool VEC>
__device__ __forceinline__ f32x4 it_piece(const float *base, int k, int D)
{
    if (VEC) {
        if (k > D - 4) k = D - 4;
        return *reinterpret_cast<const f32x4 *>(base + k);
    }
    f32x4 v;
    v.x = k < D ? base[k] : 0.f;
    v.y = k + 1 < D ? base[k + 1] : 0.f;
    v.z = k + 2 < D ? base[k + 2] : 0.f;
    v.w = k + 3 < D ? base[k + 3] : 0.f;
    return v;
}

// One workgroup = rows [64 b, 64 b + 64) against every centroid.  st.M == 1, st.sub == st.D.  VEC = false is the generic form
// (D % 4 != 0 or a misaligned base): the same tile and arithmetic behind scalar staging loads; the D % 4 elements past the
// last whole group of four go to chain 0 in order (they lie in one group of one chunk).
template <bool VEC>
__global__ __launch_bounds__(IT_THREADS) void ivt_estep_kernel(KmState st)
{
    __shared__ __attribute__((aligned(16))) float lds[2 * IT_ROWS * IT_LD];
    float *lx = lds, *lc = lds + IT_ROWS * IT_LD;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int D = st.D, K = st.K;
    const int64_t row0 = (int64_t)blockIdx.x * IT_ROWS;
    const int nchunks = (D + IT_DK - 1) / IT_DK;
    const int ntiles = (K + IT_CENTS - 1) / IT_CENTS;
    const int main4 = D & ~3, ntail = D - main4;

    // staging slot i of this lane: piece tx of row (or centroid) ty + 16 i of the tile -- the lanes of a row read 256 B in a run
    f32x4 sx[IT_PER], sc[IT_PER];
    int64_t xoff[IT_PER];
#pragma unroll
    for (int i = 0; i < IT_PER; i++) {
        int64_t r = row0 + ty + 16 * i;
        if (r >= st.n) r = st.n - 1; // (computed, never written)
        xoff[i] = r * D;
    }
    auto load_stage = [&](int ct, int c) {
        const int k = c * IT_DK + tx * 4;
#pragma unroll
        for (int i = 0; i < IT_PER; i++) {
            int cc = ct * IT_CENTS + ty + 16 * i;
            if (cc >= K) cc = K - 1; // (its key is masked)
            sx[i] = it_piece<VEC>(st.X + xoff[i], k, D);
            sc[i] = it_piece<VEC>(st.cent + (int64_t)cc * D, k, D);
        }
    };
    auto write_stage = [&]() {
#pragma unroll
        for (int i = 0; i < IT_PER; i++) {
            *reinterpret_cast<f32x4 *>(&lx[(ty + 16 * i) * IT_LD + tx * 4]) = sx[i];
            *reinterpret_cast<f32x4 *>(&lc[(ty + 16 * i) * IT_LD + tx * 4]) = sc[i];
        }
    };

    Acc<ORDER_UNROLL4> acc[IT_PER][IT_PER]; // [row ty + 16 i][centroid tx + 16 j]
    unsigned long long best[IT_PER];
#pragma unroll
    for (int i = 0; i < IT_PER; i++) best[i] = ~0ull;

    int ct = 0, c = 0;
    load_stage(0, 0);
    write_stage();
    __syncthreads();
    while (true) {
        int nct = ct, nc = c + 1;
        if (nc == nchunks) {
            nc = 0;
            nct = ct + 1;
        }
        const bool has_next = nct < ntiles;
        if (has_next) load_stage(nct, nc);
        if (c == 0) {
#pragma unroll
            for (int i = 0; i < IT_PER; i++)
#pragma unroll
                for (int j = 0; j < IT_PER; j++) acc[i][j].zero();
        }
        const int d0 = c * IT_DK;
        const int nfull4 = (min(main4, d0 + IT_DK) - d0) >> 2;
#pragma unroll 2
        for (int g = 0; g < nfull4; g++) {
            f32x4 xv[IT_PER], cv[IT_PER];
#pragma unroll
            for (int i = 0; i < IT_PER; i++) {
                xv[i] = *reinterpret_cast<const f32x4 *>(&lx[(ty + 16 * i) * IT_LD + g * 4]);
                cv[i] = *reinterpret_cast<const f32x4 *>(&lc[(tx + 16 * i) * IT_LD + g * 4]);
            }
#pragma unroll
            for (int i = 0; i < IT_PER; i++)
#pragma unroll
                for (int j = 0; j < IT_PER; j++) acc[i][j].template add4_pair<METRIC_L2>(xv[i], cv[j]);
        }
        if (ntail && main4 >= d0 && main4 < d0 + IT_DK) {
            const int g4 = main4 - d0;
            for (int t = 0; t < ntail; t++) {
                float xs[IT_PER], cs[IT_PER];
#pragma unroll
                for (int i = 0; i < IT_PER; i++) {
                    xs[i] = lx[(ty + 16 * i) * IT_LD + g4 + t];
                    cs[i] = lc[(tx + 16 * i) * IT_LD + g4 + t];
                }
#pragma unroll
                for (int i = 0; i < IT_PER; i++)
#pragma unroll
                    for (int j = 0; j < IT_PER; j++) {
                        const float e = xs[i] - cs[j];
                        acc[i][j].add_tail(e * e);
                    }
            }
        }
        __syncthreads(); // every wave is done reading the stage
        if (has_next) write_stage();
        if (c == nchunks - 1) {
#pragma unroll
            for (int j = 0; j < IT_PER; j++) {
                const int cc = ct * IT_CENTS + tx + 16 * j;
#pragma unroll
                for (int i = 0; i < IT_PER; i++) {
                    const float s = acc[i][j].total();
                    const unsigned long long key =
                        (s < IT_FLT_MAX && cc < K) ? ((unsigned long long)__float_as_uint(s) << 32) | (unsigned)cc : ~0ull;
                    best[i] = key < best[i] ? key : best[i];
                }
            }
        }
        __syncthreads();
        if (!has_next) break;
        ct = nct;
        c = nc;
    }

    // the 16 lanes of a row (one ty) are neighbours in a wave: fold their minima; lane tx == 0 commits rows ty + 16 i
    unsigned nchg = 0;
#pragma unroll
    for (int i = 0; i < IT_PER; i++) {
        unsigned long long b = best[i];
#pragma unroll
        for (int o = 8; o >= 1; o >>= 1) {
            const unsigned long long other = __shfl_xor(b, o, 64);
            b = other < b ? other : b;
        }
        const int64_t row = row0 + ty + 16 * i;
        if (tx == 0 && row < st.n) {
            const int32_t bestc = b == ~0ull ? -1 : (int32_t)(uint32_t)b;
            nchg += st.assign[row] != bestc;
            st.assign[row] = bestc;
            if (bestc < 0) atomicOr(st.bad, 1u);
        }
    }
    // rows whose assignment changed: one integer atomic per wave (km_commit's count, four rows to a lane here)
    unsigned wsum = nchg;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) wsum += __shfl_xor(wsum, o, 64);
    if ((tid & 63) == 0 && wsum) atomicAdd(&st.changed[0], wsum);
}

void launch_ivt_estep(const KmState &st, hipStream_t s)
{
    const unsigned grid = (unsigned)((st.n + IT_ROWS - 1) / IT_ROWS); // n < 2^31
    const bool vec = st.D % 4 == 0 && ((reinterpret_cast<uintptr_t>(st.X) | reinterpret_cast<uintptr_t>(st.cent)) & 15) == 0;
    if (vec) hipLaunchKernelGGL(ivt_estep_kernel<true>, dim3(grid), dim3(IT_THREADS), 0, s, st);
    else hipLaunchKernelGGL(ivt_estep_kernel<false>, dim3(grid), dim3(IT_THREADS), 0, s, st);
}

// the sort's offsets are the M-step's starts as they are; its counts are their differences
__global__ __launch_bounds__(256) void ivt_counts_kernel(const uint32_t *off, int K, uint32_t *count)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < K) count[c] = off[c + 1] - off[c];
}

void launch_ivt_counts(const uint32_t *off, int K, uint32_t *count, hipStream_t s)
{
    hipLaunchKernelGGL(ivt_counts_kernel, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, s, off, K, count);
}

} // namespace lb
