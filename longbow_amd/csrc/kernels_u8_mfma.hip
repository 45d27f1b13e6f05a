// kernels_u8_mfma.hip -- the uint8 index's i8 matrix-core pass (route 83): batches of queries, D % 16 == 0.
//
// With x' = x XOR 0x80 read as int8, x' = x - 128, so sum (x_i - q_i)^2 = sum (x'_i - q'_i)^2 = |x'|^2 + |q'|^2 - 2 x'.q', exact
// in int32 (|x'.q'| <= 8192 * 2^14 = 2^27, S < 2^30), and x'.q' is what v_mfma_i32_32x32x32_i8 computes.  The decomposition is
// mfma_i8_kernel's (kernels_i8.hip): a workgroup of 256 threads holds 128 query slots (blockIdx.y) and walks tiles of 128
// positions grid-strided; its four waves own 64 x 64 quarters of the 128 x 128 outputs as 2 x 2 blocks of the instruction; a
// stage is 128 B of each row and query, 16-B pieces into LDS at a 144-B row stride; (tile, stage) is one flat pipeline with the
// next stage's pieces in registers while the current one feeds the matrix cores.  Lane l hands the 16 bytes
// [32 s + 16 (l >> 5), +16) of row / query l & 31 to the A and B fragments alike, so the result does not depend on the byte
// order inside a lane; outputs: query column l & 31, row (reg & 3) + 8 (reg >> 2) + 4 (l >> 5) of the block.
//
// This kernel's own:
//   shift while staging  a thread XORs the dwords of each piece with 0x80808080 between the global load and the LDS store, rows
//                        and queries alike: the rows stay uint8 in HBM, the queries uint8 in the caller's buffer, no shifted
//                        copy of either exists.  A piece beyond D, and every piece of a query slot beyond nq, is stored as zeros
//                        (zero in the shifted domain; 0x80 would add (-128)^2 per padded k).
//   row norms in flight  the eight consecutive lanes that stage one row each take sum b^2 of their shifted piece by four
//                        v_dot4_i32_i8 and keep a running partial per staged row across the tile's stages; with the tile's last
//                        stage the eight lanes reduce and one stores |x'|^2 into the tile's metadata slot.  Nothing is stored
//                        per row in HBM: the handle keeps no side array.
//   the 2^24 rule        per output S = |x'|^2 + |q'|^2 - 2 acc.  S <= 2^24: the value is u8_value_of_s(S), after the integer
//                        skip S > smax(tau).  Beyond: the admitting pass drops the pair if pack(lower bound, row) >= tau (first
//                        by an integer form of the same bound), else the lane recomputes it by the chain arithmetic straight
//                        from global memory, in a function kept out of line so that its registers are not the K-loop's.  The
//                        sample pass recomputes every such pair.
#include "lb_device.h"
#include "lb_u8_exact.h"

#pragma clang fp contract(off)

namespace lb {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

constexpr int UM_ROWS = 128, UM_QS = 128, UM_CK = 128, UM_LD = UM_CK + 16;
constexpr int UM_PPR = UM_CK / 16;             // 16-B pieces per row per stage: the lanes that share a row
constexpr int UM_PT = UM_ROWS * UM_PPR / 256;  // pieces per thread per stage (rows; the queries alike)
constexpr int UM_SHIFT = (int)0x80808080u;

struct MfmaU8Args {
    const uint8_t *X;
    int64_t npos; // positions walked: the row view's (rowmap / all rows), or `count` samples
    int D;
    const uint8_t *Q8; // nq uint8 queries, row-major, 16-B aligned rows
    int nq;
    const int32_t *qn; // [nq] exact |q'|^2 (launch_query_norms_u8_shifted)
    const uint8_t *mask;
    const uint32_t *rowmap;
    CandState cs;
    int sample;
    int64_t span;
};

// corpus row behind position pos of the walk (clamped into it)
__device__ __forceinline__ uint32_t um_row(const MfmaU8Args &a, int64_t pos)
{
    if (pos >= a.npos) pos = a.npos - 1;
    const int64_t vpos = a.sample ? (int64_t)(((uint64_t)pos * (uint64_t)a.span) / (uint64_t)a.npos) : pos;
    return a.rowmap ? a.rowmap[vpos] : (uint32_t)vpos;
}

// sum of the squares of the 16 int8 bytes of a piece, added to s
__device__ __forceinline__ int um_piece_norm(i32x4 v, int s)
{
    s = __builtin_amdgcn_sdot4(v.x, v.x, s, false);
    s = __builtin_amdgcn_sdot4(v.y, v.y, s, false);
    s = __builtin_amdgcn_sdot4(v.z, v.z, s, false);
    s = __builtin_amdgcn_sdot4(v.w, v.w, s, false);
    return s;
}

// the value of a pair beyond 2^24: the reference's chains from memory.  Out of line: rare, and its registers stay out of the
// kernel's loop
__device__ __attribute__((noinline)) float um_chain_value(const uint8_t *x, const uint8_t *q, int D)
{
    return (float)sqrt((double)u8_chain_sum<true>(x, q, D));
}

// (launch bounds: two workgroups per CU.  Held to three, the 168 registers of mfma_i8_kernel, the compiler spills some 60 registers
// and reloads part of them between the MFMAs; at two it takes 225 and no scratch -- DESIGN.md section 2.3)
__global__ __launch_bounds__(256, 2) void mfma_u8_kernel(MfmaU8Args a)
{
    __shared__ __attribute__((aligned(16))) int8_t lx[UM_ROWS * UM_LD];
    __shared__ __attribute__((aligned(16))) int8_t lq[UM_QS * UM_LD];
    __shared__ uint32_t lrow[2][UM_ROWS]; // per parity of the tiles walked: corpus row, |x'|^2, (2: past the walk | 1: masked out)
    __shared__ int lnx[2][UM_ROWS];
    __shared__ uint8_t lhid[2][UM_ROWS];
    __shared__ uint64_t ltau[UM_QS];
    __shared__ int lsmax[UM_QS], lqn[UM_QS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave & 1, wq = wave >> 1;
    const int D = a.D;
    const int nchunks = (D + UM_CK - 1) / UM_CK;
    const int64_t ntiles = (a.npos + UM_ROWS - 1) / UM_ROWS;
    if ((int64_t)blockIdx.x >= ntiles) return;
    const int q0 = blockIdx.y * UM_QS;

    // the tile's query columns: threshold, integer bound, norm.  In LDS, not in registers: the epilogue reads them once a tile
    if (tid < UM_QS) {
        const int qc = q0 + tid < a.nq ? q0 + tid : a.nq - 1;
        const uint64_t t = a.sample ? kEntryMax : a.cs.tau[qc];
        int sm = 0x7fffffff;
        if (t != kEntryMax) {
            const double tk = (double)entry_key(t);
            const double b = tk * tk * (1.0 + 0x1p-20);
            if (b < 2147483647.0) sm = (int)b; // S > smax => sqrt_rn(float(S)) > tau's key
        }
        ltau[tid] = t;
        lsmax[tid] = sm;
        lqn[tid] = a.qn[qc];
    }
    const int lbk = D / 4 + 6; // u8_value_lower_bound: the value's sum is at least S (1 - lbk 2^-24)

    // staging: piece tid & 7 of the rows / query slots (tid >> 3) + 32 i
    const int kp = (tid & (UM_PPR - 1)) * 16;
    uint32_t rid[UM_PT];
    i32x4 px[UM_PT], pq[UM_PT];
    int xnp[UM_PT]; // running |x'|^2 of this lane's pieces of the tile being staged
    auto tile_rows = [&](int64_t t) {
#pragma unroll
        for (int i = 0; i < UM_PT; i++) rid[i] = um_row(a, t * UM_ROWS + (tid >> 3) + 32 * i);
    };
    auto tile_meta = [&](int64_t t, int p) {
        if (tid < UM_ROWS) {
            const int64_t pos = t * UM_ROWS + tid;
            const uint32_t row = um_row(a, pos);
            lrow[p][tid] = row;
            lhid[p][tid] = (pos >= a.npos ? 2 : 0) | ((a.mask != nullptr && !a.mask[row]) ? 1 : 0);
        }
    };
    auto load_stage = [&](int c) {
        const int k = c * UM_CK + kp;
#pragma unroll
        for (int i = 0; i < UM_PT; i++) {
            px[i] = i32x4{0, 0, 0, 0};
            pq[i] = i32x4{0, 0, 0, 0};
            if (k < D) {
                px[i] = __builtin_nontemporal_load(reinterpret_cast<const i32x4 *>(a.X + (int64_t)rid[i] * D + k)); // streamed once
                const int q = q0 + (tid >> 3) + 32 * i;
                if (q < a.nq) pq[i] = *reinterpret_cast<const i32x4 *>(a.Q8 + (int64_t)q * D + k);
            }
        }
    };
    // stage c of a tile of parity p goes to LDS shifted; its pieces' squares join the row partials, which the tile's last stage
    // reduces over the row's eight lanes into lnx[p]
    auto write_stage = [&](int c, int p) {
        const bool inside = c * UM_CK + kp < D;
#pragma unroll
        for (int i = 0; i < UM_PT; i++) {
            const int r = (tid >> 3) + 32 * i;
            i32x4 x = px[i], q = pq[i];
            if (c == 0) xnp[i] = 0;
            if (inside) { // (outside: both were loaded as zeros, zero in the shifted domain)
                x ^= UM_SHIFT;
                xnp[i] = um_piece_norm(x, xnp[i]);
                if (q0 + r < a.nq) q ^= UM_SHIFT;
            }
            const int o = r * UM_LD + kp;
            *reinterpret_cast<i32x4 *>(&lx[o]) = x;
            *reinterpret_cast<i32x4 *>(&lq[o]) = q;
        }
        if (c == nchunks - 1) {
#pragma unroll
            for (int i = 0; i < UM_PT; i++) {
                int v = xnp[i];
                v += __shfl_xor(v, 1);
                v += __shfl_xor(v, 2);
                v += __shfl_xor(v, 4);
                if ((tid & (UM_PPR - 1)) == 0) lnx[p][(tid >> 3) + 32 * i] = v;
            }
        }
    };

    i32x16 acc[2][2];
    int64_t tile = blockIdx.x;
    int c = 0, par = 0; // par: parity of the tiles this workgroup has walked (not of the tile index: gridDim.x may be even)
    tile_rows(tile);
    tile_meta(tile, 0);
    load_stage(0);
    write_stage(0, 0);
    __syncthreads();
    while (true) {
        int64_t ntile = tile;
        int nc = c + 1;
        if (nc == nchunks) {
            nc = 0;
            ntile = tile + gridDim.x;
        }
        const bool has_next = ntile < ntiles;
        if (has_next) {
            if (nc == 0) tile_rows(ntile);
            load_stage(nc);
        }
        if (c == 0) {
#pragma unroll
            for (int bi = 0; bi < 2; bi++)
#pragma unroll
                for (int bj = 0; bj < 2; bj++)
#pragma unroll
                    for (int e = 0; e < 16; e++) acc[bi][bj][e] = 0;
        }
#pragma unroll
        for (int st = 0; st < UM_CK / 32; st++) {
            const int off = st * 32 + (lane >> 5) * 16;
            i32x4 fa[2], fb[2];
#pragma unroll
            for (int b = 0; b < 2; b++) {
                fa[b] = *reinterpret_cast<const i32x4 *>(&lx[(wr * 64 + b * 32 + (lane & 31)) * UM_LD + off]);
                fb[b] = *reinterpret_cast<const i32x4 *>(&lq[(wq * 64 + b * 32 + (lane & 31)) * UM_LD + off]);
            }
#pragma unroll
            for (int bi = 0; bi < 2; bi++)
#pragma unroll
                for (int bj = 0; bj < 2; bj++)
                    acc[bi][bj] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[bi], fb[bj], acc[bi][bj], 0, 0, 0);
        }
        __syncthreads(); // every wave is done with the stage
        if (has_next) {
            // (a new tile takes the other parity: the previous tile's epilogue is behind the barrier above)
            write_stage(nc, nc == 0 ? par ^ 1 : par);
            if (nc == 0) tile_meta(ntile, par ^ 1);
        }
        __syncthreads();
        if (c == nchunks - 1) { // epilogue: exact entries, admission
            uint64_t tau[2];
            int smax[2], qnl[2];
#pragma unroll
            for (int bj = 0; bj < 2; bj++) {
                const int ql = wq * 64 + bj * 32 + (lane & 31);
                tau[bj] = ltau[ql];
                smax[bj] = lsmax[ql];
                qnl[bj] = lqn[ql];
            }
#pragma unroll
            for (int bi = 0; bi < 2; bi++) {
#pragma unroll
                for (int e = 0; e < 16; e++) {
                    const int rl = wr * 64 + bi * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
                    const int hid = lhid[par][rl];
                    if (hid & 2) continue;
                    const uint32_t row = lrow[par][rl];
                    const int xn = lnx[par][rl];
                    const int64_t pos = tile * UM_ROWS + rl;
#pragma unroll
                    for (int bj = 0; bj < 2; bj++) {
                        const int q = q0 + wq * 64 + bj * 32 + (lane & 31);
                        if (q >= a.nq) continue;
                        const uint32_t S = (uint32_t)(xn + qnl[bj] - 2 * acc[bi][bj][e]); // exact: sum (x_i - q_i)^2 < 2^30
                        if (a.sample) {
                            uint64_t ent = kEntryMax;
                            if (!hid) {
                                const float dist = S <= U8_EXACT_S ? u8_value_of_s(S) : um_chain_value(a.X + (int64_t)row * D, a.Q8 + (int64_t)q * D, D);
                                ent = pack_entry(dist, row);
                            }
                            a.cs.lists[(size_t)q * a.cs.cap + pos] = ent;
                            continue;
                        }
                        if (hid) continue;
                        float dist;
                        if (S <= U8_EXACT_S) {
                            if ((int)S > smax[bj]) continue;
                            dist = u8_value_of_s(S);
                        } else {
                            // the lower bound's sum is at least S - slack, an integer: beyond smax its value is beyond tau's key
                            const uint32_t slack = (uint32_t)(((uint64_t)S * (uint32_t)lbk) >> 24) + 2u;
                            if ((int)(S - slack) > smax[bj]) continue;
                            if (pack_entry(u8_value_lower_bound(S, D), row) >= tau[bj]) continue;
                            dist = um_chain_value(a.X + (int64_t)row * D, a.Q8 + (int64_t)q * D, D);
                        }
                        const uint64_t ent = pack_entry(dist, row);
                        if (ent < tau[bj]) {
                            const uint32_t p = atomicAdd(&a.cs.cnt[q], 1u);
                            if (p < a.cs.cap) a.cs.lists[(size_t)q * a.cs.cap + p] = ent;
                        }
                    }
                }
            }
        }
        if (!has_next) break;
        if (nc == 0) par ^= 1;
        tile = ntile;
        c = nc;
    }
}

bool mfma_u8_supported(int D, const void *X, const void *Q8)
{
    return D % 16 == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0 && (reinterpret_cast<uintptr_t>(Q8) & 15) == 0;
}

void launch_mfma_u8(const uint8_t *X, int64_t npos, int D, const uint8_t *Q8, int nq, const int32_t *qn, const uint8_t *mask,
                    const uint32_t *rowmap, CandState cs, bool sample, int64_t span, hipStream_t s)
{
    if (npos <= 0 || nq <= 0) return;
    MfmaU8Args a;
    a.X = X; a.npos = npos; a.D = D; a.Q8 = Q8; a.nq = nq; a.qn = qn; a.mask = mask; a.rowmap = rowmap;
    a.cs = cs; a.sample = sample ? 1 : 0; a.span = span;
    const int64_t ntiles = (npos + UM_ROWS - 1) / UM_ROWS;
    const int qtiles = (nq + UM_QS - 1) / UM_QS;
    // the workgroups that fit at once (__launch_bounds__: 2 per CU, 256 CUs) over the batch's query tiles; each walks row tiles
    // grid-strided
    int64_t gx = (512 + qtiles - 1) / qtiles;
    if (gx > ntiles) gx = ntiles;
    hipLaunchKernelGGL(mfma_u8_kernel, dim3((unsigned)gx, (unsigned)qtiles), dim3(256), 0, s, a);
}

// exact |q'|^2 of each uint8 query shifted by 128, one wave per query
__global__ __launch_bounds__(64) void query_norms_u8_shifted_kernel(const uint8_t *Q8, int D, int32_t *qn)
{
    const uint8_t *q = Q8 + (int64_t)blockIdx.x * D;
    int s = 0;
    for (int i = threadIdx.x; i < D; i += 64) {
        const int v = (int)q[i] - 128;
        s += v * v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (threadIdx.x == 0) qn[blockIdx.x] = s;
}
void launch_query_norms_u8_shifted(const uint8_t *Q8, int nq, int D, int32_t *qn, hipStream_t s)
{
    if (nq > 0) hipLaunchKernelGGL(query_norms_u8_shifted_kernel, dim3((unsigned)nq), dim3(64), 0, s, Q8, D, qn);
}

} // namespace lb
