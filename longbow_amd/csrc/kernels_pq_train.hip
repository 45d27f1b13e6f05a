// kernels_pq_train.hip -- exact Lloyd k-means per PQ subspace on gfx950: pq.TrainKMeans (internal/pq/kmeans.go:64-151) as
// pq.(*PQEncoder).Train calls it once per subspace (encoder.go:38-73).  All M subspaces go through every launch.
//
// One iteration is five launches:
//   km_estep    one workgroup = 256 rows x one subspace (pq_encode_kernel's shape): the row goes to the FIRST centroid whose
//               simd.L2Squared sum (four f32 chains, tail in chain 0, no sqrt) is strictly below the best so far, starting
//               from FLT_MAX.  This is not pq_encode's argmin, which compares the rounded square roots.  Writes the assignment,
//               counts the rows whose assignment changed and the histogram of (chunk of 4096 rows, cluster) -- integer atomics.
//   km_scan     per subspace: cluster sizes, cluster starts, and per chunk the offset of its rows inside each cluster.
//   km_scatter  one wave per (chunk, subspace) places the chunk's rows, in row order, behind those offsets: `order` then
//               holds every cluster's members in ascending row order (a stable counting sort by assignment).
//   km_mstep    one lane per (subspace, cluster, element) walks its cluster's members in that order: ONE sequential f32
//               chain per sum, then sum / float32(count).  No float atomics, no tree: the row order is the contract.
//               An empty cluster takes the copy of the drawn row (km_draw).
//   km_finish   iteration count and stop rule per subspace; a finished subspace is skipped by every later launch (done[m]).
#include "lb_exact.h"

#pragma clang fp contract(off)

namespace lb {

constexpr int KM_THREADS = 256;

// splitmix64's finaliser and increment: draw(seed, m, t) = mix64(mix64(seed + m) + (t + 1) * gamma)  (longbow_gpu.h)
__host__ __device__ __forceinline__ uint64_t km_mix64(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__host__ __device__ __forceinline__ uint64_t km_draw_impl(uint64_t seed, uint64_t m, uint64_t t)
{
    return km_mix64(km_mix64(seed + m) + (t + 1) * 0x9E3779B97F4A7C15ull);
}
uint64_t km_draw(uint64_t seed, uint64_t m, uint64_t t) { return km_draw_impl(seed, m, t); }

// centroid c of subspace m = the copy of row init_rows[m][c]; assignments start at -1
__global__ __launch_bounds__(KM_THREADS) void km_init_kernel(KmState st, const int64_t *init_rows)
{
    const int64_t total = (int64_t)st.M * st.K * st.sub;
    for (int64_t i = (int64_t)blockIdx.x * KM_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * KM_THREADS) {
        const int64_t mc = i / st.sub;
        const int j = (int)(i - mc * st.sub);
        const int m = (int)(mc / st.K);
        st.cent[i] = st.X[init_rows[mc] * st.D + (int64_t)m * st.sub + j];
    }
}

// the strict first minimum of one row over the K centroids at cb (stride `sub`); -1: no centroid below FLT_MAX
template <int SUB>
__device__ __forceinline__ int km_nearest(const float *v, const float *cb, int K)
{
    float best = 3.40282346638528859811704183484516925e+38f;
    int bestc = -1;
    constexpr int MAIN = SUB & ~3;
    for (int k = 0; k < K; k++) {
        const float *c = cb + k * SUB;
        Acc<ORDER_UNROLL4> a;
        a.zero();
#pragma unroll
        for (int t = 0; t < MAIN; t += 4) {
            const f32x4 q = {v[t], v[t + 1], v[t + 2], v[t + 3]};
            const f32x4 x = {c[t], c[t + 1], c[t + 2], c[t + 3]};
            a.add4_pair<METRIC_L2>(q, x);
        }
#pragma unroll
        for (int t = MAIN; t < SUB; t++) {
            const float d = v[t] - c[t];
            a.add_tail(d * d);
        }
        const float s = a.total();
        if (s < best) { // false for NaN
            best = s;
            bestc = k;
        }
    }
    return bestc;
}

// what every row of an E-step workgroup does once its centroid is known
__device__ __forceinline__ void km_commit(const KmState &st, int m, int64_t rb, int64_t row, bool active, int bestc, uint32_t *lhist)
{
    bool chg = false;
    if (active) {
        int32_t *as = st.assign + (int64_t)m * st.n + row;
        chg = *as != bestc;
        *as = bestc;
        if (bestc >= 0) atomicAdd(&lhist[bestc], 1u);
        else atomicOr(st.bad, 1u);
    }
    const unsigned long long b = __ballot(chg);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&st.changed[m], (uint32_t)__popcll(b));
    __syncthreads();
    const int64_t chunk = rb * KM_THREADS / KM_CHUNK; // (the 256 rows of a workgroup lie in one chunk)
    uint32_t *h = st.chunk_hist + ((int64_t)m * st.nchunks + chunk) * st.K;
    for (int c = threadIdx.x; c < st.K; c += KM_THREADS)
        if (lhist[c]) atomicAdd(&h[c], lhist[c]);
}

template <int SUB>
__global__ __launch_bounds__(KM_THREADS) void km_estep_kernel(KmState st)
{
    extern __shared__ __attribute__((aligned(16))) float cb[];
    __shared__ uint32_t lhist[256];
    const int m = blockIdx.x % st.M;
    const int64_t rb = blockIdx.x / st.M;
    if (st.done[m]) return;
    const float *src = st.cent + (int64_t)m * st.K * SUB;
    for (int i = threadIdx.x; i < st.K * SUB; i += KM_THREADS) cb[i] = src[i];
    lhist[threadIdx.x] = 0;
    __syncthreads();
    const int64_t row = rb * KM_THREADS + threadIdx.x;
    const bool active = row < st.n;
    int bestc = -1;
    if (active) {
        float v[SUB];
        const float *x = st.X + row * st.D + (int64_t)m * SUB;
#pragma unroll
        for (int t = 0; t < SUB; t++) v[t] = x[t];
        bestc = km_nearest<SUB>(v, cb, st.K);
    }
    km_commit(st, m, rb, row, active, bestc, lhist);
}

// any SubDim: operands straight from global memory (correctness path), tail elements in chain 0
__global__ __launch_bounds__(KM_THREADS) void km_estep_generic_kernel(KmState st)
{
    __shared__ uint32_t lhist[256];
    const int m = blockIdx.x % st.M;
    const int64_t rb = blockIdx.x / st.M;
    if (st.done[m]) return;
    lhist[threadIdx.x] = 0;
    __syncthreads();
    const int64_t row = rb * KM_THREADS + threadIdx.x;
    const bool active = row < st.n;
    int bestc = -1;
    if (active) {
        const int sub = st.sub, main4 = sub & ~3;
        const float *x = st.X + row * st.D + (int64_t)m * sub;
        const float *cbm = st.cent + (int64_t)m * st.K * sub;
        float best = 3.40282346638528859811704183484516925e+38f;
        for (int k = 0; k < st.K; k++) {
            const float *c = cbm + (int64_t)k * sub;
            Acc<ORDER_UNROLL4> a;
            a.zero();
            for (int t = 0; t < main4; t += 4) {
                const f32x4 q = {x[t], x[t + 1], x[t + 2], x[t + 3]};
                const f32x4 y = {c[t], c[t + 1], c[t + 2], c[t + 3]};
                a.add4_pair<METRIC_L2>(q, y);
            }
            for (int t = main4; t < sub; t++) {
                const float d = x[t] - c[t];
                a.add_tail(d * d);
            }
            const float s = a.total();
            if (s < best) {
                best = s;
                bestc = k;
            }
        }
    }
    km_commit(st, m, rb, row, active, bestc, lhist);
}

// One workgroup per subspace, thread c = cluster c: the chunk histogram column becomes the exclusive prefix over the
// chunks (in place), its total the cluster's size, and the exclusive scan of the sizes the cluster's start in `order`.
__global__ __launch_bounds__(256) void km_scan_kernel(KmState st)
{
    __shared__ uint32_t s_scan[256];
    const int m = blockIdx.x, c = threadIdx.x;
    if (st.done[m] || *st.bad) return;
    uint32_t run = 0;
    if (c < st.K) {
        uint32_t *h = st.chunk_hist + (int64_t)m * st.nchunks * st.K + c;
        for (int64_t ch = 0; ch < st.nchunks; ch++) {
            const uint32_t v = h[ch * st.K];
            h[ch * st.K] = run;
            run += v;
        }
    }
    s_scan[c] = run;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const uint32_t add = c >= off ? s_scan[c - off] : 0u;
        __syncthreads();
        s_scan[c] += add;
        __syncthreads();
    }
    if (c < st.K) {
        st.count[m * st.K + c] = run;
        st.start[m * st.K + c] = s_scan[c] - run;
    }
}

// One wave per (chunk, subspace): 64 rows at a time, in row order.  A lane's place is its cluster's cursor plus the number
// of lower lanes with the same cluster (eight ballots, one per bit of the cluster index); the last such lane moves the cursor.
__global__ __launch_bounds__(64) void km_scatter_kernel(KmState st)
{
    __shared__ uint32_t cur[256];
    const int m = blockIdx.x % st.M;
    const int64_t chunk = blockIdx.x / st.M;
    if (st.done[m] || *st.bad) return;
    const int lane = threadIdx.x;
    uint32_t *h = st.chunk_hist + ((int64_t)m * st.nchunks + chunk) * st.K;
    for (int c = lane; c < st.K; c += 64) {
        cur[c] = st.start[m * st.K + c] + h[c];
        h[c] = 0; // the next iteration's histogram starts from zero
    }
    __syncthreads();
    const int32_t *as = st.assign + (int64_t)m * st.n;
    uint32_t *ord = st.order + (int64_t)m * st.n;
    const unsigned long long lt = (1ull << lane) - 1ull;
    const int64_t r0 = chunk * KM_CHUNK;
    for (int step = 0; step < KM_CHUNK / 64; step++) {
        const int64_t row = r0 + step * 64 + lane;
        if (r0 + step * 64 >= st.n) break;
        const bool valid = row < st.n;
        const int key = valid ? as[row] : 0;
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const unsigned long long bal = __ballot(valid && ((key >> b) & 1));
            peers &= ((key >> b) & 1) ? bal : ~bal;
        }
        const uint32_t rank = (uint32_t)__popcll(peers & lt), cnt = (uint32_t)__popcll(peers);
        uint32_t base = 0;
        if (valid) base = cur[key];
        __syncthreads();
        if (valid) {
            ord[base + rank] = (uint32_t)row;
            if (rank == cnt - 1) cur[key] = base + cnt;
        }
        __syncthreads();
    }
}

// One lane per (subspace, cluster, element).  The member rows of eight steps are fetched ahead of the chain that consumes them.
__global__ __launch_bounds__(KM_THREADS) void km_mstep_kernel(KmState st, uint64_t seed, int it)
{
    const int64_t i = (int64_t)blockIdx.x * KM_THREADS + threadIdx.x;
    if (i >= (int64_t)st.M * st.K * st.sub) return;
    const int64_t mc = i / st.sub;
    const int j = (int)(i - mc * st.sub);
    const int m = (int)(mc / st.K), c = (int)(mc - (int64_t)m * st.K);
    if (st.done[m] || *st.bad) return;
    const uint32_t cnt = st.count[mc], s0 = st.start[mc];
    const float *xc = st.X + (int64_t)m * st.sub + j;
    if (cnt == 0) { // kmeans.go:137-141 with the documented draw in place of rand.Intn
        const uint64_t row = km_draw_impl(seed, (uint64_t)m, (uint64_t)st.K + (uint64_t)it * (uint64_t)st.K + (uint64_t)c) % (uint64_t)st.n;
        st.cent[i] = xc[(int64_t)row * st.D];
        return;
    }
    const uint32_t *ord = st.order + (int64_t)m * st.n + s0;
    float sum = 0.f;
    uint32_t t = 0;
    for (; t + 8 <= cnt; t += 8) {
        float x[8];
#pragma unroll
        for (int u = 0; u < 8; u++) x[u] = xc[(int64_t)ord[t + u] * st.D];
#pragma unroll
        for (int u = 0; u < 8; u++) sum = sum + x[u];
    }
    for (; t < cnt; t++) sum = sum + xc[(int64_t)ord[t] * st.D];
    st.cent[i] = __fdiv_rn(sum, (float)cnt);
}

// iteration `it` is over: count it for every live subspace, apply the stop rule (kmeans.go:145), clear `changed`, and tell
// the host (pinned words) how many subspaces go on and whether a row had no admissible centroid
__global__ __launch_bounds__(256) void km_finish_kernel(KmState st, int it, uint32_t thr, uint32_t *h_state)
{
    __shared__ uint32_t live;
    if (threadIdx.x == 0) live = 0;
    __syncthreads();
    const uint32_t bad = *st.bad;
    for (int m = threadIdx.x; m < st.M; m += 256) {
        if (st.done[m]) continue;
        if (!bad) {
            st.iters[m] = it + 1;
            if (it > 0 && st.changed[m] < thr) st.done[m] = 1;
        }
        st.changed[m] = 0;
        if (!st.done[m]) atomicAdd(&live, 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        h_state[0] = live;
        h_state[1] = bad;
    }
}

void launch_km_init(const KmState &st, const int64_t *d_init_rows, hipStream_t s)
{
    int64_t blocks = ((int64_t)st.M * st.K * st.sub + KM_THREADS - 1) / KM_THREADS;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(km_init_kernel, dim3((unsigned)blocks), dim3(KM_THREADS), 0, s, st, d_init_rows);
}

// (grid.x carries M x row-blocks with the subspace index fastest, as launch_pq_encode has it: the M workgroups that read
// the same 256 rows run back to back and share the rows' cache lines in L2)
void launch_km_estep(const KmState &st, hipStream_t s)
{
    const int64_t nrb = (st.n + KM_THREADS - 1) / KM_THREADS;
    const dim3 grid((unsigned)(nrb * st.M)), block(KM_THREADS);
    const size_t shmem = (size_t)st.K * st.sub * sizeof(float);
#define LB_KM(S) hipLaunchKernelGGL((km_estep_kernel<S>), grid, block, shmem, s, st)
    switch (st.sub) {
    case 1: LB_KM(1); break;
    case 2: LB_KM(2); break;
    case 4: LB_KM(4); break;
    case 8: LB_KM(8); break;
    case 12: LB_KM(12); break;
    case 16: LB_KM(16); break;
    case 32: LB_KM(32); break;
    default: hipLaunchKernelGGL(km_estep_generic_kernel, grid, block, 0, s, st); break;
    }
#undef LB_KM
}

void launch_km_order(const KmState &st, hipStream_t s)
{
    hipLaunchKernelGGL(km_scan_kernel, dim3((unsigned)st.M), dim3(256), 0, s, st);
    hipLaunchKernelGGL(km_scatter_kernel, dim3((unsigned)(st.nchunks * st.M)), dim3(64), 0, s, st);
}

void launch_km_mstep(const KmState &st, uint64_t seed, int it, hipStream_t s)
{
    const int64_t blocks = ((int64_t)st.M * st.K * st.sub + KM_THREADS - 1) / KM_THREADS;
    hipLaunchKernelGGL(km_mstep_kernel, dim3((unsigned)blocks), dim3(KM_THREADS), 0, s, st, seed, it);
}

void launch_km_finish(const KmState &st, int it, uint32_t thr, uint32_t *h_state, hipStream_t s)
{
    hipLaunchKernelGGL(km_finish_kernel, dim3(1), dim3(256), 0, s, st, it, thr, h_state);
}

} // namespace lb
