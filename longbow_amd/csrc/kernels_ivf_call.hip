// kernels_ivf_call.hip -- the row bitmap given with a search call on the IVF-Flat, IVF-PQ and IVF-SQ8 handles (lb_gpu_ivf_search*_bitmap*,
// lb_gpu_ivfpq_search_bitmap*, lb_gpu_ivfsq8_search_bitmap*; semantics in include/longbow_gpu.h): the probed lists of a batch are
// compacted under the call's bitmap into synthetic lists of this call alone, which the plan, every scan and the selection then
// walk unchanged through IvfBatch.L / IvfBatch.probes.  Under ONE bitmap for a call that would walk more list positions than the
// handle holds, every list is compacted once instead (the same two launches over a pseudo-query that probes every list), and a
// batch only renames its probes (ivf_call_shared_probes_kernel).
//
// The synthetic lists.  Probe slot (q, p), pair i = q np + p, gets TWO lists: 2 i holds the rows of the probed list whose bit is
// set, ascending, and 2 i + 1 is a gap that nobody probes.  List 2 i starts where the UNFILTERED rows of the slots before p would
// end, at q pmax + (the sizes of the lists probed in slots 0 .. p - 1): that place is known before any bit is read, so one pass
// places the rows, and the gap takes up what the bitmap hid.  soff is one monotone array over srows[nq][pmax]:
//   soff[2 i]     = q pmax + sum of len(probes[q][p']) over p' < p      (ivf_call_starts_kernel, one wave per query)
//   soff[2 i + 1] = soff[2 i] + the rows kept                           (ivf_call_compact_kernel, one workgroup per pair)
//   soff[2 nq np] = nq pmax
//   sprobes[i]    = 2 i
// Two launches, no count pass and no read-back: the visible counts never reach the host, which keeps sizing by its upper bounds.
// Integer only; no workgroup waits for another; the output depends on the inputs alone.
#include "lb_device.h"
#include "lb_ivf.h"
#include "lb_select.h"

#include <algorithm>
#include <stdexcept>

namespace lb {

constexpr int ICF_THREADS = 256;
constexpr int ICF_PER = 8;                        // rows per thread per step: two 16-byte loads
constexpr int ICF_STEP = ICF_THREADS * ICF_PER;   // rows per workgroup per step
static_assert(ICF_STEP == IVF_CALL_STEP_ROWS, "lb_ivf.h names the step for the tests' shapes");

// One wave per query, as ivf_plan_kernel scans: the starts of the query's synthetic lists and its synthetic probes.
__global__ __launch_bounds__(64) void ivf_call_starts_kernel(IvfCallLists a)
{
    const int q = blockIdx.x, lane = threadIdx.x;
    const uint64_t q0 = (uint64_t)q * (uint64_t)a.pmax;
    uint64_t run = 0;
    for (int p0 = 0; p0 < a.np; p0 += 64) {
        const int p = p0 + lane;
        const int64_t pair = (int64_t)q * a.np + p;
        uint32_t len = 0;
        if (p < a.np) {
            const int64_t l = a.probes[pair];
            if (l >= 0 && l < a.L.nlist) len = a.L.off[l + 1] - a.L.off[l];
        }
        const uint32_t incl = wave_incl_scan(len, lane); // (distinct lists: at most the handle's rows, < 2^31)
        if (p < a.np) {
            a.soff[2 * pair] = (uint32_t)(q0 + std::min<uint64_t>(run + incl - len, (uint64_t)a.pmax));
            a.sprobes[pair] = 2 * pair;
        }
        run += __shfl(incl, 63);
    }
    if (q == a.nq - 1 && lane == 0) a.soff[2 * (int64_t)a.nq * a.np] = (uint32_t)(q0 + (uint64_t)a.pmax);
}

// One workgroup per (query, probe slot).  The list is walked in steps of ICF_STEP positions of L.rows, counted from the 8-aligned
// position at or below its first one, so that a thread's eight row numbers are two aligned 16-byte loads (VEC: L.rows is 32-byte
// aligned); positions outside the list are loaded as well, being entries of the array, and masked.  The bit of a row is a byte gather from the
// query's bitmap.  Per step: popcount per thread, wave scan, the four wave totals through LDS (two sets, used in turn, so that a
// step costs one barrier), then the kept rows are stored behind the workgroup's running count.  The loads of the next step are
// issued before the scan of this one: they do not depend on the count, only the store addresses do.
struct IcfStep {
    uint32_t r[ICF_PER];
    uint32_t keep; // bit i: r[i] is a row of the list and its bit is set
};

// Every load is issued whether or not its value is wanted, at an address clamped into the array, and masked afterwards: a load
// inside a divergent branch is waited for before the branch ends, which made a step eight dependent round trips.  Only the last,
// partial group of eight of the whole array takes guarded loads a row.
//
// MODE (lb_ivf.h, IVF_CALL_*): what an entry of L.rows is.  ROWS: the row, stored and looked up as it is; this form is the
// kernel as it was.  POS_ALL: the same loads, the entry being the row whose bit decides, and the position `at` is what is stored.
// POS_VISIBLE: the entry is a position, which is stored; the row whose bit decides is rowof[pos], one more dependent gather.  Its
// eight loads are issued together, each at an address clamped into rowof, before the first bitmap byte is asked for, so the chain
// is three round trips a step and not ten.
template <bool VEC, int MODE>
__device__ __forceinline__ void icf_load(const IvfCallLists &a, const uint8_t *bm, uint32_t lo, uint32_t hi, uint32_t pos, IcfStep &s)
{
    const uint32_t last = a.rows_len - 1; // the array's last entry (rows_len >= 1 here: hi > lo)
    if (VEC) { // (rows_len >= ICF_PER too: the launcher saw to it)
        const uint32_t vpos = pos + ICF_PER <= a.rows_len ? pos : 0u;
        const uint4 x = *reinterpret_cast<const uint4 *>(a.L.rows + vpos), y = *reinterpret_cast<const uint4 *>(a.L.rows + vpos + 4);
        s.r[0] = x.x, s.r[1] = x.y, s.r[2] = x.z, s.r[3] = x.w;
        s.r[4] = y.x, s.r[5] = y.y, s.r[6] = y.z, s.r[7] = y.w;
        if (vpos != pos) {
#pragma unroll
            for (int i = 0; i < ICF_PER; i++) s.r[i] = a.L.rows[min(pos + (uint32_t)i, last)];
        }
    } else {
#pragma unroll
        for (int i = 0; i < ICF_PER; i++) s.r[i] = a.L.rows[min(pos + (uint32_t)i, last)];
    }
    uint32_t rowv[ICF_PER]; // the row whose bit decides
#pragma unroll
    for (int i = 0; i < ICF_PER; i++) rowv[i] = s.r[i];
    if (MODE == IVF_CALL_POS_VISIBLE) {
#pragma unroll
        for (int i = 0; i < ICF_PER; i++) rowv[i] = a.rowof[s.r[i] < a.rowof_len ? s.r[i] : 0u]; // (rowof_len >= 1: the launcher saw to it)
    }
    uint32_t byte[ICF_PER];
#pragma unroll
    for (int i = 0; i < ICF_PER; i++) byte[i] = bm[((int64_t)rowv[i] < a.nbits ? rowv[i] : 0u) >> 3]; // (nbits >= 1)
    s.keep = 0;
#pragma unroll
    for (int i = 0; i < ICF_PER; i++) {
        const uint32_t at = pos + (uint32_t)i, row = rowv[i]; // (pos + 8 <= 2^31 + ICF_STEP: no wrap)
        const bool inside = MODE != IVF_CALL_POS_VISIBLE || s.r[i] < a.rowof_len; // (the entry is a position of the handle)
        if (at >= lo && at < hi && inside && (int64_t)row < a.nbits && ((byte[i] >> (row & 7u)) & 1u)) s.keep |= 1u << i;
        if (MODE == IVF_CALL_POS_ALL) s.r[i] = at; // what is stored: the position
    }
}

template <bool VEC, int MODE>
__global__ __launch_bounds__(ICF_THREADS) void ivf_call_compact_kernel(IvfCallLists a)
{
    __shared__ uint32_t s_wave[2][ICF_THREADS / 64];
    const int64_t pair = blockIdx.x;
    const int q = (int)(pair / a.np);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t start = a.soff[2 * pair];
    const uint32_t limit = a.soff[2 * pair + 2]; // the next slot's start: what this list had room for before the bitmap
    const int64_t l = a.probes[pair];
    uint32_t lo = 0, hi = 0;
    if (l >= 0 && l < a.L.nlist) {
        lo = a.L.off[l];
        hi = a.L.off[l + 1];
    }
    const uint8_t *bm = a.bits + (int64_t)q * a.stride;
    const uint32_t g0 = lo & ~(uint32_t)(ICF_PER - 1);
    const uint32_t nsteps = hi > lo ? (hi - g0 + ICF_STEP - 1) / ICF_STEP : 0u;
    uint32_t run = 0; // rows kept by the steps so far
    IcfStep cur{}, nxt{};
    if (nsteps > 0) icf_load<VEC, MODE>(a, bm, lo, hi, g0 + (uint32_t)tid * ICF_PER, cur);
    for (uint32_t st = 0; st < nsteps; st++) {
        if (st + 1 < nsteps) icf_load<VEC, MODE>(a, bm, lo, hi, g0 + (st + 1) * ICF_STEP + (uint32_t)tid * ICF_PER, nxt);
        const uint32_t c = (uint32_t)__popc(cur.keep);
        const uint32_t incl = wave_incl_scan(c, lane);
        uint32_t *sw = s_wave[st & 1u];
        if (lane == 63) sw[wave] = incl;
        __syncthreads();
        uint32_t before = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < ICF_THREADS / 64; w++) {
            const uint32_t t = sw[w];
            if (w < wave) before += t;
            tot += t;
        }
        uint32_t at = start + run + before + incl - c;
#pragma unroll
        for (int i = 0; i < ICF_PER; i++)
            if ((cur.keep >> i) & 1u) {
                if (at < limit) a.srows[at] = cur.r[i]; // (always: a list keeps at most its own rows)
                at++;
            }
        run += tot;
        cur = nxt;
    }
    if (tid == 0) a.soff[2 * pair + 1] = start + std::min<uint32_t>(run, limit - start);
}

template <int MODE> static void launch_ivf_call_compact(const IvfCallLists &a, int64_t pairs, hipStream_t s)
{
    if ((reinterpret_cast<uintptr_t>(a.L.rows) & 31) == 0 && a.rows_len >= (uint32_t)ICF_PER)
        hipLaunchKernelGGL((ivf_call_compact_kernel<true, MODE>), dim3((unsigned)pairs), dim3(ICF_THREADS), 0, s, a);
    else hipLaunchKernelGGL((ivf_call_compact_kernel<false, MODE>), dim3((unsigned)pairs), dim3(ICF_THREADS), 0, s, a);
}

void launch_ivf_call_lists(const IvfCallLists &a, hipStream_t s)
{
    const int64_t pairs = (int64_t)a.nq * a.np;
    if (pairs <= 0) return;
    const bool visible = a.mode == IVF_CALL_POS_VISIBLE;
    if ((visible && (!a.rowof || a.rowof_len < 1)) || a.mode < IVF_CALL_ROWS || a.mode > IVF_CALL_POS_VISIBLE)
        throw std::logic_error("the call's lists: no such mode, or positions without their rows"); // (before anything is launched)
    hipLaunchKernelGGL(ivf_call_starts_kernel, dim3((unsigned)a.nq), dim3(64), 0, s, a);
    if (visible) launch_ivf_call_compact<IVF_CALL_POS_VISIBLE>(a, pairs, s);
    else if (a.mode == IVF_CALL_POS_ALL) launch_ivf_call_compact<IVF_CALL_POS_ALL>(a, pairs, s);
    else launch_ivf_call_compact<IVF_CALL_ROWS>(a, pairs, s);
}

// The shared form's probes: list l of the handle is synthetic list 2 l of the call.  A thread an entry.
__global__ __launch_bounds__(256) void ivf_call_shared_probes_kernel(const int64_t *probes, int64_t count, int nlist, int64_t *out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const int64_t l = probes[i];
    out[i] = l >= 0 && l < nlist ? 2 * l : -1;
}

void launch_ivf_call_shared_probes(const int64_t *probes, int64_t count, int nlist, int64_t *out, hipStream_t s)
{
    if (count <= 0) return;
    hipLaunchKernelGGL(ivf_call_shared_probes_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, probes, count, nlist, out);
}

} // namespace lb
