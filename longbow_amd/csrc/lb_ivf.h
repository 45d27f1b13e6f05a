// lb_ivf.h -- what ivf.hip (host) and kernels_ivf.hip / kernels_ivf_call.hip (device) of the IVF-Flat index share: the argument
// blocks of the kernels and their launchers.  The semantics are stated in include/longbow_gpu.h (lb_gpu_ivf_*).
#pragma once
#include "lb_device.h"

namespace lb {

// The inverted lists over rows kept in insertion order: list l is rows[off[l], off[l + 1]), ascending.
struct IvfLists {
    const uint32_t *off;  // [nlist + 1]
    const uint32_t *rows; // [n]
    int nlist;
};

// One batch of queries as the search kernels take it (by value).
struct IvfBatch {
    const float *X; // [n][D] rows, insertion order
    int D;
    IvfLists L;
    const float *Q;        // [nq][D]
    const float *qna;      // [nq] ||q||^2 in the handle's order (cosine; else unused)
    int nq;
    const int64_t *probes; // [nq][np] the coarse search's labels: distinct lists per query
    int np;
    uint32_t *seg;         // [nq][np + 1]: exclusive prefix of the probed lists' sizes, then their total P_q
    uint64_t *keys;        // [nq][pmax]: pack_entry(distance, row) of every scanned row, list by list
    int64_t pmax;          // keys per query: the sum of the np largest list sizes
};

constexpr int IVF_MAX_NLIST = 65536;
constexpr uint32_t IVF_SELECT_LDS_KEYS = 16384; // a query with at most this many scanned rows is selected from an LDS copy

// probes[q][p] = p: every list, for a search that probes them all without asking the coarse index
void launch_ivf_all_probes(int64_t *probes, int nq, int np, hipStream_t s);
// seg of every query; stats (u64[4], zero before a search's first batch): [1] += P_q, [2] = max P_q, [3] += P_q fits LDS
void launch_ivf_plan(const IvfBatch &a, unsigned long long *stats, hipStream_t s);
// keys[q][seg[q][p] + i] = entry of the i-th row of the p-th probed list; maxlen: the longest list of the handle
void launch_ivf_scan(int metric, int order, const IvfBatch &a, int64_t maxlen, hipStream_t s);
// the k smallest keys of each query, ascending -> dist / labels [nq][k] (ids nullable: the row itself), padded FLT_MAX / -1
void launch_ivf_select(const IvfBatch &a, int k, const int64_t *ids, float *dist, int64_t *labels, hipStream_t s);

// assign[i] = labels[i] (the coarse search's k = 1 labels)
void launch_ivf_narrow(const int64_t *labels, int64_t n, uint32_t *assign, hipStream_t s);
// Stable counting sort of rows [0, n) by assign: off[nlist + 1] and rows[n].  hist: scratch of ivf_sort_hist_words(n, nlist) u32.
// Returns the error of the memset that clears hist (nothing is launched then).
size_t ivf_sort_hist_words(int64_t n, int nlist);
hipError_t launch_ivf_sort(const uint32_t *assign, int64_t n, int nlist, uint32_t *hist, uint32_t *off, uint32_t *rows, hipStream_t s);

// The visible lists of a row filter: visible list l is the rows of L's list l whose mask byte is non-zero, in the same order; with
// `positions` it holds, in place of each such row, its position in L.rows (ascending in [off[l], off[l + 1])).
// voff[nlist + 1] and vrows[voff[nlist]] (room for n) are written, voff[nlist] being the number of visible rows; scratch holds
// ivf_visible_scratch_bytes(n) bytes, 16-byte aligned.  Three launches, or with n == 0 the memset of voff alone, whose error is
// returned.
size_t ivf_visible_scratch_bytes(int64_t n);
hipError_t launch_ivf_visible(const uint8_t *mask, const IvfLists &L, int64_t n, bool positions, void *scratch, uint32_t *voff, uint32_t *vrows,
                              hipStream_t s);

// A row bitmap given with a search call (kernels_ivf_call.hip): the probed lists of a batch, compacted under the call's bitmap
// into synthetic lists that the plan, the scans and the selection walk in place of L and probes.  Row r passes iff
// bits[q stride + (r >> 3)] >> (r & 7) & 1 (stride 0: one bitmap for every query); rows at or beyond nbits never pass.
//   soff    [2 nq np + 1]  list 2 (q np + p) holds the passing rows of the list probed in slot p of query q, ascending, and
//                          starts at q pmax + the sizes of the lists probed in the slots before p; list 2 (q np + p) + 1 is the
//                          gap up to the next start and is never probed.  Monotone, soff[2 nq np] = nq pmax
//   sprobes [nq][np]       2 (q np + p)
//   srows   [nq][pmax]     the entries of the synthetic lists
// pmax: at least the rows of any np distinct lists of L, and nq pmax < 2^32.  An invalid probe gives an empty list.
// What an entry of L.rows is, and with it what a synthetic list holds and which row's bit decides (`mode`):
//   IVF_CALL_ROWS          a row: stored as it is, and its own bit is looked up (IVF-Flat, IVF-SQ8: their scans gather by row)
//   IVF_CALL_POS_ALL       L is the lists of ALL rows of a handle whose scans read list-major codes by position (IVF-PQ): entry
//                          `at` is the row at position `at`; the position is stored, the bit is that of L.rows[at]
//   IVF_CALL_POS_VISIBLE   L is the visible lists of such a handle, whose entries are positions: the position is stored, the bit
//                          is that of rowof[pos], rowof being the rows of the lists of all rows; pos < rowof_len before it indexes
// In the two position modes the scans take their `_visible` forms over the synthetic lists, with rows = rowof.
enum { IVF_CALL_ROWS = 0, IVF_CALL_POS_ALL = 1, IVF_CALL_POS_VISIBLE = 2 };
struct IvfCallLists {
    IvfLists L;            // the handle's lists: the visible ones under a handle filter or removals
    uint32_t rows_len;     // entries of L.rows that may be read: at least L.off[L.nlist]
    const int64_t *probes; // [nq][np] the coarse search's labels
    int nq, np;
    int64_t pmax;
    const uint8_t *bits;
    int64_t stride, nbits;
    uint32_t *soff;
    int64_t *sprobes;
    uint32_t *srows;
    int mode;              // IVF_CALL_*
    const uint32_t *rowof; // [rowof_len] IVF_CALL_POS_VISIBLE: position -> row; else unused
    uint32_t rowof_len;
    IvfLists lists() const { return IvfLists{soff, srows, 2 * nq * np}; }
};
constexpr int IVF_CALL_STEP_ROWS = 2048; // list positions a workgroup of the compaction takes per step
// two launches: the starts and the synthetic probes (a wave per query), then the compaction (a workgroup per probe slot)
void launch_ivf_call_lists(const IvfCallLists &a, hipStream_t s);
// One compaction for a whole call under ONE bitmap: launch_ivf_call_lists over a single pseudo-query that probes every list in
// order (probes = launch_ivf_all_probes(., 1, nlist), pmax = the rows of all lists) leaves list l of L as synthetic list 2 l.
// Every batch then only renames its probes: out[i] = 2 probes[i] for a probe in [0, nlist), else -1 (no list of either numbering)
void launch_ivf_call_shared_probes(const int64_t *probes, int64_t count, int nlist, int64_t *out, hipStream_t s);

// Coarse-quantiser training (kernels_ivf_train.hip; host side ivf_train.hip).  st.M == 1, st.sub == st.D, st.K <= IVF_MAX_NLIST.
// E-step: st.assign[row] = the first strict minimum of simd.L2Squared over st.cent (-1 and *st.bad: none below FLT_MAX),
// st.changed[0] += rows whose assignment changed.  chunk_hist, count, start and order are not touched.
void launch_ivt_estep(const KmState &st, hipStream_t s);
// count[c] = off[c + 1] - off[c] of launch_ivf_sort's offsets (which are the M-step's starts as they are)
void launch_ivt_counts(const uint32_t *off, int K, uint32_t *count, hipStream_t s);

} // namespace lb
