/*
 * longbow_gpu.h -- C ABI of liblongbow_gpu.so: the MI355X (gfx950) k-NN
 * distance / top-k / PQ-ADC backend that drops in behind Longbow's
 * internal/gpu plug-point and keeps internal/simd's metric semantics.
 *
 * Plain pointers and sizes only; every call returns an lb_status code (0 = ok)
 * and never aborts the process (reference convention: non-zero -> Go
 * fmt.Errorf("... code %d"), NULL handle = init failure;
 * internal/gpu/faiss_gpu.go:56-66,99-101,134-137).
 *
 * Each entry point cites the reference interface it replaces
 * (paths relative to 23skdu/longbow).  The cgo stub a maintainer adds is in
 * INTEGRATION.md and go/internal/gpu/hip_gpu.go.
 *
 * Pointer naming: plain names are HOST pointers, borrowed for the call only
 * (cgo pointer rules: the library copies/DMAs during the call and retains
 * nothing).  `d_` names are DEVICE (HBM) pointers on the index's device.
 */
#ifndef LONGBOW_GPU_H
#define LONGBOW_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* simd.MetricType values (internal/simd/registry.go:8-15); search returns the
 * value Longbow ranks by, ascending: L2 with sqrt, 1-cos, NEGATED dot
 * (internal/store/distance_resolvers.go:12-16,74-83). */
typedef enum {
    LB_METRIC_EUCLIDEAN = 0,
    LB_METRIC_COSINE = 1,
    LB_METRIC_DOT = 2
} lb_metric;

/* f32 accumulation order of the reported distances (both exist in the reference):
 * SEQ     one accumulator, i ascending (internal/simd/simd_test.go:13-33,
 *         simd.go:138-163) -- the canonical oracle order, default;
 * UNROLL4 four accumulators (internal/simd/simd.go:365-479,
 *         distance_functions.go:195-227) -- what EuclideanDistanceBatchFlat runs. */
typedef enum { LB_ORDER_SEQ = 0, LB_ORDER_UNROLL4 = 1 } lb_order;

typedef enum {
    LB_OK = 0,
    LB_ERR_INVALID_ARG = 1, /* NULL / negative / mismatched sizes                  */
    LB_ERR_CLOSED = 2,      /* "index is closed" (faiss_gpu.go:79,111)             */
    LB_ERR_NO_DEVICE = 3,   /* no HIP device / bad device id (ErrGPUNotAvailable)   */
    LB_ERR_HIP = 4,         /* a HIP runtime call failed; see lb_gpu_last_error     */
    LB_ERR_OOM = 5,         /* HBM or pinned-host allocation failed                 */
    LB_ERR_UNSUPPORTED = 6, /* e.g. PQ with K != 256 (simd.go:350 stride)           */
    LB_ERR_INTERNAL = 7,
    LB_ERR_CANCELLED = 8,   /* the call's lb_cancel fired: ctx.Err() == context.Canceled          */
    LB_ERR_DEADLINE = 9     /* its deadline passed:        ctx.Err() == context.DeadlineExceeded  */
} lb_status;

typedef struct lb_gpu_index lb_gpu_index; /* opaque; replaces FaissGpuResourcesPtr +
                                             FaissGpuIndexFlatL2Ptr (faiss_gpu.go:12-13) */

/* ---- library ------------------------------------------------------------ */
int lb_gpu_device_count(void);          /* 0 when no GPU is visible; never fails */
const char *lb_gpu_version(void);
const char *lb_gpu_status_string(int status);

/* ---- gpu.Index: NewIndexWithConfig / Add / Search / Close ------------------
 * Replaces faiss_gpu_resources_new + faiss_gpu_index_flat_l2_new
 * (internal/gpu/faiss_gpu.go:16-19,44-72; interface.go:3-19).  dim <= 0 or an
 * unknown metric -> NULL (gpu_test.go:49-55).  out_status (nullable) receives
 * the reason.  dim > LB_MAX_DIM -> NULL / LB_ERR_UNSUPPORTED (the kernels stage one query row in LDS;
 * the reference has no cap, embedding widths in practice are <= 4096). */
#define LB_MAX_DIM 8192
#define LB_MAX_K 2048 /* largest k of a search entry point (LB_ERR_UNSUPPORTED beyond); lb_gpu_pq_search* alone take k up to 4096 */
lb_gpu_index *lb_gpu_index_new(int device, int dim, int metric, int *out_status);

/* Close (faiss_gpu.go:147-167): frees HBM; idempotent on NULL.  Must not race with any other call on the same
 * handle: the caller's lock orders Close after the last Add / Search (the Go shim's RWMutex does, as
 * faiss_gpu.go:148 does); a call on a freed handle is a use-after-free like with any C handle. */
void lb_gpu_index_free(lb_gpu_index *h);

/* Text of the last failure on this handle ("" if none).  Valid until the next
 * failing call on the same handle.  Concurrent host-pointer searches of a few queries are combined into one
 * device batch (lb_gpu_index_set_combining): this text, last_fallbacks and last_route describe the last device
 * BATCH on the handle, which may have held other callers' queries.  Return codes are per caller: a combined
 * batch that fails is searched again request by request before anybody is told. */
const char *lb_gpu_last_error(const lb_gpu_index *h);

int lb_gpu_index_set_order(lb_gpu_index *h, int order);

/* How the batched path generates candidates before the exact f32 re-rank.  Results are identical in every mode:
 * the re-rank recomputes every reported distance in the reference's f32 order and a rounding-error bound proves
 * that the candidate set contains the true top-k, else the query is re-done by the exact scan.
 *   LB_CAND_AUTO       (default) the cheapest route at every batch size: narrow tiles (HBM-bound passes) for small
 *                      batches, beyond them q.x as hi*hi + hi*lo + lo*hi on the bf16 MFMA with BOTH f32 operands split
 *                      into bf16 pairs in registers after the LDS read (no second copy of the corpus).
 *   LB_CAND_F32_MFMA   strict: beyond 384 queries q.x on the f32 MFMA (v_mfma_f32_32x32x2_f32); batches of
 *                      5..384 queries as AUTO.  The headline of bench.py is measured in this mode.
 *   LB_CAND_SPLIT_BF16 the split contraction over a pre-split image of the corpus (x = hi + lo + O(2^-18));
 *                      costs a second N*dim*4-byte copy in HBM; dim % 32 == 0.
 *   LB_CAND_SPLIT_BF16_INREG the in-register split for every batch beyond the narrow tiles.
 *   LB_CAND_F16        beyond 64 queries q.x as ONE fp16 product per element (corpus rounded to fp16 in registers, each
 *                      query scaled by a power of two): a third of the matrix work, error bound ~1.1e-3 |q||x| -- still
 *                      inside what the containment proof needs on embedding-like data; AUTO takes this route by itself
 *                      while the corpus norms allow it (max |x| <= 2^13, smallest non-zero |x| >= 2^-6), otherwise the
 *                      split contraction. */
typedef enum { LB_CAND_F32_MFMA = 0, LB_CAND_SPLIT_BF16 = 1, LB_CAND_SPLIT_BF16_INREG = 2, LB_CAND_AUTO = 3, LB_CAND_F16 = 4 } lb_candidate_mode;
int lb_gpu_index_set_candidate_mode(lb_gpu_index *h, int mode);
/* The fp16 route's own copy of the corpus (2 bytes per element, K-blocked): half the bytes to stage per batched search of
 * more than 64 queries (1M x 768, 1024 queries: see LABNOTES.md 4.2).  mode 1 (default): kept while the route is on offer for
 * this index (LB_CAND_AUTO from 16,384 rows, or LB_CAND_F16; norms in range; any dimension: the copy is laid out in
 * zero-padded planes of 32 dimensions, which is also what opens the matrix-core routes to dimensions like 100 or 300) and the copy leaves
 * max(2 GiB, 1/16 of the device) free -- brought up to date inside Add, dropped when the conditions end; mode 0: never (the
 * route then rounds the f32 rows in registers).  Results do not depend on it: both forms see the same fp16 values, and every
 * reported distance comes from the exact f32 re-rank.  There is no reference counterpart (a memory-for-speed knob of this
 * backend, like the index's capacity reservation). */
int lb_gpu_index_set_f16_image(lb_gpu_index *h, int mode);
int64_t lb_gpu_index_f16_image_bytes(const lb_gpu_index *h); /* HBM held by that copy right now (0: none) */

/* Concurrent host-pointer searches (lb_gpu_index_search with at most 16 queries and no cancellation context -- the reference's
 * gpu.Index.Search is ONE query per call, from many goroutines: internal/gpu/faiss_gpu.go:108-145) are COMBINED: one or two
 * callers search at once; callers that arrive while the device is taken queue, and the first of them then answers everybody who
 * queued with the same k by ONE batched search (at most 256 queries); after a combined batch the next caller waits up to 50 us
 * for the others to come back before it launches.  A batch's lists are the single searches' lists bit for bit, so only the clock
 * can tell: sixteen threads of single-query searches on 1M x 768 go from 4.2 k to 40 k queries/s, p50 3.7 -> 0.40 ms.  On by
 * default; 0 switches it off for the handle.  stats: out[0] = combined batches run, out[1] = requests they answered. */
int lb_gpu_index_set_search_combining(lb_gpu_index *h, int enable);
int lb_gpu_index_combining_stats(const lb_gpu_index *h, int64_t out[2]);
/* rows committed so far; safe beside Add / Search from other threads (read under the handle's reader lock, so it waits out an Add
 * in progress and never reports half a chunk) */
int64_t lb_gpu_index_ntotal(const lb_gpu_index *h);
int lb_gpu_index_dim(const lb_gpu_index *h);
int lb_gpu_index_device(const lb_gpu_index *h); /* GPUConfig.DeviceID (interface.go:15-19); -1 on NULL */

/* Pre-size HBM for n_total rows (optional; add grows geometrically otherwise). */
int lb_gpu_index_reserve(lb_gpu_index *h, int64_t n_total);

/* Add (replaces faiss_gpu_index_add, faiss_gpu.go:20,75-104): APPENDS n rows of
 * row-major f32[n*dim] -- the values buffer of an Arrow FixedSizeList<float32>
 * column (internal/store/adaptive_index.go:276-315).  ids nullable: labels are
 * then insertion positions (what the FAISS binding does, faiss_gpu.go:93-97).
 * The host buffer is staged through library-owned pinned memory and DMA'd. */
int lb_gpu_index_add(lb_gpu_index *h, int64_t n, const float *vectors, const int64_t *ids);
/* Same with the rows already in HBM on the index's device (D2D append). */
int lb_gpu_index_add_device(lb_gpu_index *h, int64_t n, const float *d_vectors,
                            const int64_t *d_ids);

/* Search (replaces faiss_gpu_index_search, faiss_gpu.go:21,107-144; semantics of
 * BruteForceIndex.SearchVectors, internal/store/adaptive_index.go:161-225):
 * exact k-NN of nq queries, results ascending by (distance, row position).
 * dist/labels are nq*k; fewer than k hits -> label -1 / dist FLT_MAX padding.
 * Thread-safe for concurrent calls on one handle (faiss_gpu.go:108 RLock). */
int lb_gpu_index_search(lb_gpu_index *h, int64_t nq, const float *queries, int k,
                        float *dist, int64_t *labels);
/* Queries and results resident in HBM; `stream` is a hipStream_t (NULL = the
 * library's own).  Results are complete when the call returns. */
int lb_gpu_index_search_device(lb_gpu_index *h, int64_t nq, const float *d_queries, int k,
                               float *d_dist, int64_t *d_labels, void *stream);

/* ---- float16 indexes: VectorTypeFloat16 (internal/store/arrow_utils.go:67-80) --------------------------
 * Rows live in HBM as IEEE binary16, 2 bytes per element; half values cross the ABI as uint16_t bit patterns (the layout of
 * Arrow HalfFloat and Go float16.Num).  Distances are the reference's F16 functions (internal/simd/simd.go:767-848): f32
 * arithmetic on the widened values, so results equal the f32 index's over the widened data bit for bit -- same lists, same
 * ascending (distance, row) order, dot negated.  Default order LB_ORDER_UNROLL4 (the reference's only F16 order); SEQ works too.
 * Batched searches take the fp16-image routes (last_route 63 / 73: the image is a relayout of the rows, exact) while they are
 * on offer -- image kept, persistent kernels, no per-row mask -- and the exact scan over the fp16 rows otherwise (route 0).
 * On an F16 handle reserve / ntotal / dim / set_filter / filter_* / set_f16_image / f16_image_bytes / last_* / profiling / free
 * work as on an f32 one; set_candidate_mode takes AUTO and F16 only (else LB_ERR_UNSUPPORTED); rerank and comm searches
 * return LB_ERR_UNSUPPORTED.  An f32 add / search on an F16 handle, or an _f16 call on an f32 handle, is LB_ERR_INVALID_ARG
 * with a last_error text.  _f16 host searches are not combined. */
lb_gpu_index *lb_gpu_index_new_f16(int device, int dim, int metric, int *out_status);
int lb_gpu_index_dtype(const lb_gpu_index *h); /* 0 float32, 1 float16, 2 int8 (simd.DataType, internal/simd/registry.go) */
int lb_gpu_index_add_f16(lb_gpu_index *h, int64_t n, const uint16_t *vectors, const int64_t *ids);
int lb_gpu_index_add_f16_device(lb_gpu_index *h, int64_t n, const uint16_t *d_vectors, const int64_t *d_ids);
/* HBM the index holds now: rows (as mapped / allocated), the per-row side arrays, the row list and any accelerator image */
int64_t lb_gpu_index_hbm_bytes(const lb_gpu_index *h);

/* ---- cancellation: the ctx of SearchVectors(ctx, ...) ------------------------------------------
 * The reference's brute-force loop polls ctx.Err() every 1000 rows (internal/store/adaptive_index.go:182).
 * A cgo caller makes one lb_cancel per call, fires it from `go func(){ <-ctx.Done(); C.lb_cancel_fire(c) }()`
 * (or sets the ctx's deadline on it) and passes it to a *_ctx entry point.  The library polls it on the host
 * before every kernel launch of the search -- a launch covers at most one pass over <= 2.5M rows of one
 * batch (dense) or one query's pass over the codes (PQ), i.e. <= ~12 ms on 1M x 768 x 1024 queries -- stops
 * enqueuing, waits for what is already on the stream and returns LB_ERR_CANCELLED / LB_ERR_DEADLINE; the
 * output buffers then hold unspecified values.  NULL ctx = never cancelled.  All calls are thread-safe. */
typedef struct lb_cancel lb_cancel;
lb_cancel *lb_cancel_new(void);
void lb_cancel_fire(lb_cancel *c);                            /* idempotent                           */
void lb_cancel_set_deadline_ms(lb_cancel *c, int64_t ms_from_now); /* < 0 clears the deadline          */
int lb_cancel_state(const lb_cancel *c);                      /* 0, LB_ERR_CANCELLED or LB_ERR_DEADLINE */
void lb_cancel_free(lb_cancel *c);                            /* after the call that used it returned */
int lb_gpu_index_search_ctx(lb_gpu_index *h, int64_t nq, const float *queries, int k, float *dist, int64_t *labels,
                            const lb_cancel *ctx);
int lb_gpu_index_search_device_ctx(lb_gpu_index *h, int64_t nq, const float *d_queries, int k, float *d_dist,
                                   int64_t *d_labels, void *stream, const lb_cancel *ctx);
/* the float16 index's searches: fp16 queries (widened exactly on the device) */
int lb_gpu_index_search_f16(lb_gpu_index *h, int64_t nq, const uint16_t *queries, int k, float *dist, int64_t *labels);
int lb_gpu_index_search_f16_ctx(lb_gpu_index *h, int64_t nq, const uint16_t *queries, int k, float *dist, int64_t *labels,
                                const lb_cancel *ctx);
int lb_gpu_index_search_f16_device_ctx(lb_gpu_index *h, int64_t nq, const uint16_t *d_queries, int k, float *d_dist,
                                       int64_t *d_labels, void *stream, const lb_cancel *ctx);

/* ---- int8 indexes: VectorTypeInt8 (internal/store/types/types.go; arrow_utils.go maps FixedSizeList<Int8> to it) ----------
 * Rows live in HBM as signed int8, 1 byte per element, row-major; queries are int8 too.  Distances are the reference's
 * DataTypeInt8 registry kernels (internal/simd/dispatch.go): L2 euclideanInt8AVX2Kernel (the exact int32 sum of the first
 * 16 floor(D/16) squared differences, rounded once to f32, the tail added in f32 in order, sqrt correctly rounded), dot
 * dotInt8Unrolled4x (four f32 chains over i mod 4, tail in chain 0, ((p0 + p1) + p2) + p3), negated.  Same lists and ascending
 * (distance, row) order as the f32 index.  Metrics: L2 and dot; cosine (no int8 kernel in the reference) and dot with
 * floor(D/4) + D mod 4 > 1024 (the chains would leave the exact integers) are NULL / LB_ERR_UNSUPPORTED at creation.
 * Searches take the exact int8 scan (last_route 80) or, from 16 queries with D % 16 == 0 (dot: D <= 1024), the i8 MFMA pass
 * (81); both compute every entry's exact value.  On an int8 handle reserve / ntotal / dim / set_filter / filter_* /
 * last_* / profiling / free work as on an f32 one; set_order is accepted and changes nothing (the arithmetic has one form);
 * set_candidate_mode takes AUTO only (else LB_ERR_UNSUPPORTED); set_f16_image is accepted and has no effect (no image is
 * built: f16_image_bytes stays 0); rerank and comm searches return LB_ERR_UNSUPPORTED; dtype is 2.  A float32 / _f16 add or
 * search on an int8 handle, or an _i8 call on another, is LB_ERR_INVALID_ARG with a last_error text.  _i8 host searches are
 * not combined. */
lb_gpu_index *lb_gpu_index_new_i8(int device, int dim, int metric, int *out_status);
int lb_gpu_index_add_i8(lb_gpu_index *h, int64_t n, const int8_t *vectors, const int64_t *ids);
int lb_gpu_index_add_i8_device(lb_gpu_index *h, int64_t n, const int8_t *d_vectors, const int64_t *d_ids);
int lb_gpu_index_search_i8(lb_gpu_index *h, int64_t nq, const int8_t *queries, int k, float *dist, int64_t *labels);
int lb_gpu_index_search_i8_ctx(lb_gpu_index *h, int64_t nq, const int8_t *queries, int k, float *dist, int64_t *labels,
                               const lb_cancel *ctx);
int lb_gpu_index_search_i8_device_ctx(lb_gpu_index *h, int64_t nq, const int8_t *d_queries, int k, float *d_dist,
                                      int64_t *d_labels, void *stream, const lb_cancel *ctx);

/* Metadata predicate mask for filtered search (SURVEY f-3; byte-per-row 0/1 as
 * internal/query/filter_evaluator.go:79-115 produces).  mask has ntotal bytes;
 * NULL clears it.  Rows with mask 0 never appear in results. */
int lb_gpu_index_set_filter(lb_gpu_index *h, const uint8_t *mask, int64_t n);
/* rows a plain search sees: the live rows that pass the handle's filter (ntotal without a filter and with nothing removed), as
 * lb_gpu_bq_nvisible; a bitmap given with a search call does not move it; 0 on NULL */
int64_t lb_gpu_index_nvisible(const lb_gpu_index *h);

/* ---- call bitmap: a row filter given with the search call ------------------------------------------------------------------
 * The reference brings the filter with the request (SearchVectorsWithBitmap, SearchVectors(..., filters, ...), every
 * VectorSearchRequest), from many goroutines at once; set_filter is a property of the handle, set under the exclusive lock.
 * The six entry points below take exactly what their plain counterparts take and, behind k, a row filter of THIS CALL alone:
 * (bitmap, nbits).
 *   bit layout    one bit per row POSITION (as set_filter's mask is by position), least significant bit first as in an Arrow
 *                 validity buffer: row r is visible to the call iff bitmap[r >> 3] >> (r & 7) & 1.
 *   reading       byte by byte at any byte address: no alignment is owed, nothing past bit nbits - 1 is read as a row and
 *                 nothing beyond ceil(nbits / 8) bytes is read at all.  The host forms take a host pointer, the _device forms
 *                 device memory, read on `stream`.
 *   one bitmap    per call, shared by all nq queries; there is no stride: a flat batch walks the corpus once for all its
 *                 queries, so a view per query would be nq searches -- which a caller can issue concurrently itself.
 *   result        the exact k-NN among the rows that are live, pass the handle's filter if one is set AND have their bit set:
 *                 labels and distances are bit for bit what the same index answers after lb_gpu_index_set_filter with the mask
 *                 bit(r) != 0 (ANDed with its filter and liveness); label -1 / dist FLT_MAX padding when fewer than k rows
 *                 pass; labels are ids when the index holds ids.
 *   handle state  not changed, and held shared like any search: calls with different bitmaps run concurrently.  nvisible, the
 *                 handle's filter, its mask, its row list and its shared sample of the view are neither read as the call's view
 *                 nor written, and every later call answers as before.  (The adaptive hints any search may move -- the fp16
 *                 route's back-off and the widened candidate list -- may move.)
 *   arguments     a NULL bitmap is the plain search through the plain path, combining included; nbits is then ignored.  A
 *                 non-NULL bitmap with nbits != ntotal (the n != ntotal rule of set_filter) is LB_ERR_INVALID_ARG with both
 *                 numbers in last_error, answered before any launch -- behind the plain entry point's own checks, which come
 *                 first and in their order (so nq == 0 is LB_OK whatever the bitmap).  An empty index answers all padding.  An
 *                 index never holds more rows than a row list can name (Add refuses beyond 2^32), so no size is refused here
 *                 that set_filter takes.
 *   combining     a call with a bitmap is never combined with other requests: it is its own device search, as a call with a
 *                 ctx is.  Plain calls running beside it keep being combined.
 *   cancellation  ctx is polled before the view is built, and then as in every search.
 *   device work   the view is built once per call on the call's stream, into the call's pooled workspace (ntotal bytes of mask,
 *                 4 ntotal of row list): one pass turns the bits, ANDed with the handle's effective mask, into the call's byte
 *                 mask and a count per 2,048 rows, a one-workgroup scan and a scatter leave the ascending row list, and four
 *                 bytes (the visible count) return to the host in one synchronisation.  From that count set_filter's rule: at
 *                 most 95 % visible and the search walks the list, above it tests the call's mask per row, and with every bit
 *                 set and no handle mask it is the unmasked search.  Under profiling these three launches fall into ms[1] /
 *                 n_launch[1] of lb_gpu_index_last_timing.
 * Not here: a bitmap per query, predicates (filter_int64 / _float32) given per call.  (The IVF-Flat, IVF-PQ and IVF-SQ8 handles
 * have their own *_search_bitmap* entry points below; the IVF-BQ handle has none.) */
int lb_gpu_index_search_bitmap_ctx(lb_gpu_index *h, int64_t nq, const float *queries, int k, const uint8_t *bitmap, int64_t nbits,
                                   float *dist, int64_t *labels, const lb_cancel *ctx);
int lb_gpu_index_search_bitmap_device_ctx(lb_gpu_index *h, int64_t nq, const float *d_queries, int k, const uint8_t *d_bitmap,
                                          int64_t nbits, float *d_dist, int64_t *d_labels, void *stream, const lb_cancel *ctx);
int lb_gpu_index_search_f16_bitmap_ctx(lb_gpu_index *h, int64_t nq, const uint16_t *queries, int k, const uint8_t *bitmap, int64_t nbits,
                                       float *dist, int64_t *labels, const lb_cancel *ctx);
int lb_gpu_index_search_f16_bitmap_device_ctx(lb_gpu_index *h, int64_t nq, const uint16_t *d_queries, int k, const uint8_t *d_bitmap,
                                              int64_t nbits, float *d_dist, int64_t *d_labels, void *stream, const lb_cancel *ctx);
int lb_gpu_index_search_i8_bitmap_ctx(lb_gpu_index *h, int64_t nq, const int8_t *queries, int k, const uint8_t *bitmap, int64_t nbits,
                                      float *dist, int64_t *labels, const lb_cancel *ctx);
int lb_gpu_index_search_i8_bitmap_device_ctx(lb_gpu_index *h, int64_t nq, const int8_t *d_queries, int k, const uint8_t *d_bitmap,
                                             int64_t nbits, float *d_dist, int64_t *d_labels, void *stream, const lb_cancel *ctx);

/* simd.CompareOp values (internal/simd/simd.go:38-45) */
typedef enum { LB_CMP_EQ = 0, LB_CMP_NEQ = 1, LB_CMP_GT = 2, LB_CMP_GE = 3, LB_CMP_LT = 4, LB_CMP_LE = 5 } lb_compare_op;

/* Evaluate a metadata predicate ON THE DEVICE straight into the index's row mask: the GPU form of
 * query.int64FilterOp/float32FilterOp.MatchBitmap (internal/query/filter_evaluator.go:79-115,205-241).
 * column has ntotal values (host pointer, e.g. an Arrow Int64/Float32 values buffer); validity is the
 * Arrow validity bitmap (LSB first; NULL = no nulls; nulls never match); combine 0 replaces the
 * mask, 1 ANDs into it (FilterEvaluator's AND chain, simd.AndBytes). */
int lb_gpu_index_filter_int64(lb_gpu_index *h, const int64_t *column, int64_t n, int64_t value, int op,
                              const uint8_t *validity, int64_t validity_offset, int combine);
int lb_gpu_index_filter_float32(lb_gpu_index *h, const float *column, int64_t n, float value, int op,
                                const uint8_t *validity, int64_t validity_offset, int combine);

/* Removal: rows leave the index, as ArrowHNSW.Delete / DeleteBatch put ids on a tombstone set (internal/store/arrow_hnsw.go:468-513),
 * and the index knows: no search has to over-fetch and drop afterwards (SearchHybrid's k * 10, hnsw_gpu.go:84-123).  A removed row
 * keeps its position (and its HBM) until lb_gpu_index_compact; it is live no more, and nothing but compaction undoes that.
 *   remove       labels, the values Search returns: ids[row] when the index holds ids, else the row position.  With ids EVERY live
 *                row whose id is in the set goes (two rows added under one id both go).  _device: the labels are in device
 *                memory (on an index with ids they make a round trip through the host to be sorted; n is small beside ntotal).
 *   remove_rows  row POSITIONS whether or not the index holds ids: the currency of rerank, refine and the code handles.
 *   ignored      an unknown label, a position outside [0, ntotal), -1 (the padding of a result list), a label given twice and a
 *                row already removed are ignored, not errors: the reference's Delete never fails.
 *   n_removed    nullable; the number of rows this call newly removed.
 *   errors       n == 0 is LB_OK; a NULL handle, n < 0, or n > 0 with a null pointer: LB_ERR_INVALID_ARG, answered before a device
 *                is touched and with nothing written.
 *   searches     every search entry point of the handle (host and device forms, _ctx, _f16, _i8, combined concurrent host
 *                searches) answers the exact k-NN among the rows that are live AND pass the filter, in ascending (distance, row
 *                position) order: bit for bit what a fresh index holding only the live rows, in their order, with ids = the old
 *                labels and the same filter restricted to them would answer.  Fewer such rows than k: -1 / FLT_MAX padding.
 *   filters      set_filter / filter_* keep taking ntotal values (removed rows included: positions do not move) and never
 *                resurrect a removed row; set_filter(NULL) leaves the live rows visible.  Rows added later are live.
 *   refine       treats a removed position as outside the index (it joins the -1 padding): a code handle's shortlist cannot
 *                resurrect a deleted row.  It keeps ignoring the filter.
 *   rerank       is left alone: it reports one distance per given position over the stored bytes, removed or not.
 *   types        float32, float16 and int8 handles alike; no element data is touched.  The accelerator images stay as they are.
 *   cost         a pass over the labels (positions) or over the index's ids (labels of an index with ids), then the row list is
 *                rebuilt as after a filter call; searches then cost what they cost under a filter with the same visible rows.
 * Exclusive against everything else on the handle, as add and the filter calls. */
int lb_gpu_index_remove(lb_gpu_index *h, int64_t n, const int64_t *labels, int64_t *n_removed);
int lb_gpu_index_remove_device(lb_gpu_index *h, int64_t n, const int64_t *d_labels, int64_t *n_removed);
int lb_gpu_index_remove_rows(lb_gpu_index *h, int64_t n, const int64_t *rows, int64_t *n_removed);
/* ntotal - ndeleted; 0 for a NULL handle */
int64_t lb_gpu_index_nlive(const lb_gpu_index *h);
/* removed rows the index still holds (ntotal counts them); 0 for a NULL handle */
int64_t lb_gpu_index_ndeleted(const lb_gpu_index *h);

/* Compaction: the removed rows leave physically and stably, survivor j being the j-th live row of before.  Afterwards
 * ntotal == nlive and ndeleted == 0; an index with ids keeps every label; an index WITHOUT ids labels by the new positions, as
 * FAISS's flat remove_ids does: the caller renumbers through old_rows.  A filter in force survives, its bytes move with the rows.
 *   old_rows  nullable, room for cap >= nlive entries (else LB_ERR_INVALID_ARG with a last_error text and nothing changed):
 *             receives each survivor's former position, ascending, for a code handle or a location table kept beside the index.
 *   nothing removed: LB_OK and nothing changes (old_rows: 0, 1, ...).  Everything removed: the index is empty and takes adds again.
 *   memory    mapped memory is kept and reused by later adds (hbm_bytes need not shrink).  The gather runs in place, in rounds
 *             through a bounded scratch: no second copy of the corpus is ever resident.  The accelerator images are rebuilt.
 *   failure   a refusal before the rows move (an allocation) leaves the index as it was; once they are in place nothing fails
 *             the call.  A device fault while they move leaves the handle unusable, as it leaves the device.
 * Exclusive against everything else on the handle. */
int lb_gpu_index_compact(lb_gpu_index *h, int64_t *old_rows, int64_t cap);

/* Per-search telemetry of the most recent search on this handle (for benches):
 * number of queries that needed the exact-scan fallback. */
int64_t lb_gpu_index_last_fallbacks(const lb_gpu_index *h);
/* Cumulative count of small-batch searches (1..32 queries) whose in-launch threshold hand-off gave up after its
 * ~1 ms bound (the launch's workgroups were not co-resident, e.g. many such launches from many streams at once) and
 * were redone on the exact path: a latency event worth a metric, never a correctness one. */
int64_t lb_gpu_index_fused_giveups(const lb_gpu_index *h);
/* Which kernel generated the candidates of the most recent batched search on this handle: kind * 10 + operand form.
 * kind: 0 exact scan path (<= 4 queries, non-finite data), 1 / 2 narrow tile (32 / 64 queries per pass), (3: retired
 * in round 4), 4 128 x 128 f32-MFMA tile, 5 256 x 256 split-bf16 tile, 6 256 x 256 fp16 single-product tile, 8 the int8
 * index (80: exact scan, 81: i8 MFMA pass);
 * form: 0 f32 operands, 1 pre-split corpus image, 2 split in registers, 3 fp16.  Telemetry only. */
int lb_gpu_index_last_route(const lb_gpu_index *h);

/* Candidate re-rank: the distance step of processChunkInternal
 * (internal/store/parallel_search.go:274-364).  The reference gathers the candidates' vectors into a
 * flat buffer and calls simd.EuclideanDistanceBatchFlat (:347), then emits
 * SearchResult{ID, Distance: d, Score: 1/(1+d)} (:355-362).  Here the candidate rows are gathered from the
 * corpus already resident in HBM (no PCIe re-upload): rows[i] is a row POSITION (the label Search returns
 * when Add got no ids, faiss_gpu.go:93-97); dist[i] is the index metric's distance in the requested
 * accumulation order (LB_ORDER_UNROLL4 is what the reference runs here; -1 = the index's own order),
 * score[i] = 1/(1+dist[i]) in f32 (nullable).  A row outside [0, ntotal) reports FLT_MAX / 0 -- the value
 * EuclideanDistanceBatch gives a nil vector (internal/simd/batch_operations.go:39-42).  The caller sorts
 * and truncates (parallel_search.go:123-130). */
int lb_gpu_index_rerank(lb_gpu_index *h, const float *query, const int64_t *rows, int64_t n, int order,
                        float *dist, float *score);
int lb_gpu_index_rerank_device(lb_gpu_index *h, const float *d_query, const int64_t *d_rows, int64_t n, int order,
                               float *d_dist, float *d_score, void *stream);

/* Batched exact refine of shortlists: nq queries x c candidate rows each -> the exact top k of every shortlist, on the device,
 * over the rows of a float32 or a float16 index.  The second stage behind a code index (BQ, SQ8, PQ, IVF-Flat, IVF-PQ), whose
 * k-NN under the codes is a shortlist and not the answer; the reference's hybrid hand-off searches k * 10 and keeps k
 * (hnsw_gpu.go:84-123).
 *   queries   f32[nq][dim], on a float16 index too: the arithmetic is the f32 arithmetic on the widened rows, so the result is
 *             that of a float32 index holding the same values.
 *   rows      int64[nq][c] row POSITIONS, as for rerank.  The candidate set S_q of query q is the set of values of rows[q][.]
 *             inside [0, ntotal) that name a live row: anything else (the -1 padding of a short shortlist, a row that
 *             lb_gpu_index_remove* has removed) is skipped, a value that occurs more than
 *             once counts once, and the order of the entries does not matter.  The index's row filter is ignored, as rerank
 *             ignores it (a filter on the code handle has already shaped the shortlist).
 *   result    dist / labels [nq][k]: the first k members of S_q in ascending (distance, row) order, the distance being the
 *             index metric's in `order` (-1: the index's own) -- L2 with the square root, cosine 1 - cos, dot negated: bit for
 *             bit what lb_gpu_index_search reports for those rows.  labels are ids[row] when the index holds ids, else the row;
 *             FLT_MAX / -1 beyond |S_q|.
 *   limits    1 <= k <= LB_MAX_K, 1 <= c <= LB_REFINE_MAX_C (k > c is allowed and gives padding); nq is unlimited (the host
 *             walks it in batches under a scratch bound) and nq == 0 is LB_OK.
 *   errors    null pointers, nq < 0, a bad order, c out of range or k <= 0: LB_ERR_INVALID_ARG; k > LB_MAX_K:
 *             LB_ERR_UNSUPPORTED; an int8 index: LB_ERR_UNSUPPORTED with a last_error text.  An empty index gives all padding.
 * Thread-safe against each other and against searches (shared lock), exclusive against add, reserve and the filter calls.
 * The _device form enqueues on `stream`, or on a private stream when it is null; ctx (nullable) is polled before every launch
 * (LB_ERR_CANCELLED / LB_ERR_DEADLINE, the outputs then hold unspecified values).  Results are complete on return. */
#define LB_REFINE_MAX_C 16384
int lb_gpu_index_refine(lb_gpu_index *h, int64_t nq, const float *queries, int64_t c, const int64_t *rows, int k, int order,
                        float *dist, int64_t *labels);
int lb_gpu_index_refine_ctx(lb_gpu_index *h, int64_t nq, const float *queries, int64_t c, const int64_t *rows, int k, int order,
                            float *dist, int64_t *labels, const lb_cancel *ctx);
int lb_gpu_index_refine_device_ctx(lb_gpu_index *h, int64_t nq, const float *d_queries, int64_t c, const int64_t *d_rows, int k,
                                   int order, float *d_dist, int64_t *d_labels, void *stream, const lb_cancel *ctx);
/* ms of the last refine that ran while lb_gpu_index_set_profiling was on, summed over its batches: the preparation of the lists,
 * the scan (with a cosine index's query norms), the selection.  Profiling costs a drain per batch.  Telemetry only. */
int lb_gpu_index_refine_last_timing(lb_gpu_index *h, float ms[3]);

/* ---- internal/simd batch interface on the GPU --------------------------------
 * simd.EuclideanDistanceBatchFlat / CosineDistanceBatch / DotProductBatch
 * (internal/simd/batch_operations.go:64-87,131-157): one query x n rows of
 * flat[n*dims] -> results[n], in the requested accumulation order, bit-exact
 * with the scalar formulas.  metric DOT returns the RAW dot product here (as
 * simd.DotProduct does, distance_functions.go:59-73), not the negated value. */
int lb_simd_distance_batch_flat(int device, int metric, int order, const float *query,
                                const float *flat, int64_t n, int dims, float *results);
int lb_simd_distance_batch_flat_device(int device, int metric, int order, const float *d_query,
                                       const float *d_flat, int64_t n, int dims,
                                       float *d_results, void *stream);
/* simd.EuclideanDistanceBatch / CosineDistanceBatch / DotProductBatch over a SLICE OF SLICES
 * (internal/simd/batch_operations.go:29-60,131-157): vectors[i] points at vector i (host), lens[i] is its
 * length.  Per-vector rules of the reference:
 *   Euclidean  a nil or length-mismatched vector yields math.MaxFloat32 (batch_operations.go:39-42,51;
 *              simd_amd64.go:217-220);
 *   Cosine/Dot a nil vector is skipped -- results[i] keeps the value the caller put there (simd.go:241-267) --
 *              and a length mismatch makes the reference's loop stop at that vector with the error swallowed
 *              (batch_operations.go:140,155): results[i..] keep the caller's values.
 * The valid vectors are packed into one pinned block, DMA'd and scored by the same kernel as the flat call. */
int lb_simd_distance_batch(int device, int metric, int order, const float *query, int dims,
                           const float *const *vectors, const int *lens, int64_t n, float *results);

/* simd.MatchInt64 / simd.MatchFloat32 (internal/simd/simd.go:570-761): dst[i] = src[i] OP val ? 1 : 0,
 * and simd.AndBytes (simd.go:119-125): dst[i] &= src[i].  Host pointers. */
int lb_simd_match_int64(int device, const int64_t *src, int64_t n, int64_t value, int op, uint8_t *dst);
int lb_simd_match_float32(int device, const float *src, int64_t n, float value, int op, uint8_t *dst);
int lb_simd_and_bytes(int device, uint8_t *dst, const uint8_t *src, int64_t n);

/* ---- internal/pq on the GPU ---------------------------------------------------
 * Codebooks arrive as the reference's serialised blob (internal/pq/persistence.go:9-35:
 * u32 LE dims, M, K, then M*K*SubDim f32 LE).  K must be 256 (simd.go:350). */
typedef struct lb_gpu_pq lb_gpu_pq;
lb_gpu_pq *lb_gpu_pq_new(int device, const uint8_t *codebook_blob, size_t len, int *out_status);
void lb_gpu_pq_free(lb_gpu_pq *p);
const char *lb_gpu_pq_last_error(const lb_gpu_pq *p);
int lb_gpu_pq_m(const lb_gpu_pq *p);
int lb_gpu_pq_dims(const lb_gpu_pq *p);
int64_t lb_gpu_pq_ntotal(const lb_gpu_pq *p);
/* Append n codes u8[n*M] (row-major, as pq.Encode emits them). */
int lb_gpu_pq_add_codes(lb_gpu_pq *p, int64_t n, const uint8_t *codes);
int lb_gpu_pq_add_codes_device(lb_gpu_pq *p, int64_t n, const uint8_t *d_codes);
int lb_gpu_pq_reserve(lb_gpu_pq *p, int64_t n_total);
/* Read back stored codes rows [row0, row0+n) as u8[n*M] (e.g. to persist what add_vectors_device encoded). */
int lb_gpu_pq_get_codes(lb_gpu_pq *p, int64_t row0, int64_t n, uint8_t *codes);
/* pq.(*PQEncoder).Encode (internal/pq/encoder.go:76-136) for n vectors of f32[dims] -> codes u8[n*M]:
 * per subspace the FIRST centroid with the strictly smallest float32(sqrt(float64(L2^2))) in the
 * 4-accumulator order, as simd.FindNearestCentroid's K > 8 branch computes it
 * (internal/simd/simd.go:305-326, 365-396).  (K <= 16 codebooks -- the encodeSequential branch -- are
 * rejected at lb_gpu_pq_new with LB_ERR_UNSUPPORTED: K must be 256.) */
int lb_gpu_pq_encode(lb_gpu_pq *p, int64_t n, const float *vectors, uint8_t *codes);
int lb_gpu_pq_encode_device(lb_gpu_pq *p, int64_t n, const float *d_vectors, uint8_t *d_codes, void *stream);
/* Encode n device-resident vectors and append their codes (the ingest step that produces config 4's codes). */
int lb_gpu_pq_add_vectors_device(lb_gpu_pq *p, int64_t n, const float *d_vectors);
/* pq.(*PQEncoder).Decode (encoder.go:139-158): codes u8[n*M] -> vectors f32[n*dims]. */
int lb_gpu_pq_decode(lb_gpu_pq *p, int64_t n, const uint8_t *codes, float *vectors);
int lb_gpu_pq_decode_device(lb_gpu_pq *p, int64_t n, const uint8_t *d_codes, float *d_vectors, void *stream);
/* processChunkInternal's PQ branch (internal/store/parallel_search.go:292-345): ADC distance of the stored
 * code rows rows[0..n) to `query` (table built per call) + score = 1/(1+d) (nullable); rows outside
 * [0, ntotal) report FLT_MAX / 0. */
int lb_gpu_pq_rerank(lb_gpu_pq *p, const float *query, const int64_t *rows, int64_t n, float *dist, float *score);
int lb_gpu_pq_rerank_device(lb_gpu_pq *p, const float *d_query, const int64_t *d_rows, int64_t n, float *d_dist,
                            float *d_score, void *stream);
/* pq.BuildADCTable (internal/pq/adc_table.go:15-51): table f32[M*K] for one query. */
int lb_gpu_pq_build_adc_table(lb_gpu_pq *p, const float *query, float *table);
/* simd.ADCDistanceBatch (internal/simd/batch_operations.go:119-127, simd.go:345-355):
 * results[i] = float32(sqrt(float64(sum_j table[j*256+codes[i*M+j]]))) over the stored codes
 * rows [row0, row0+n). */
int lb_gpu_pq_adc_distance_batch(lb_gpu_pq *p, const float *table, int64_t row0, int64_t n,
                                 float *results);
/* ADC k-NN over all stored codes: builds the table per query, scans, top-k ascending by
 * (distance, position).  nq queries of f32[dims]. */
int lb_gpu_pq_search(lb_gpu_pq *p, int64_t nq, const float *queries, int k, float *dist,
                     int64_t *labels);
int lb_gpu_pq_search_device(lb_gpu_pq *p, int64_t nq, const float *d_queries, int k,
                            float *d_dist, int64_t *d_labels, void *stream);
/* the same with a cancellation context, polled between the queries of the batch and the launches of one query */
int lb_gpu_pq_search_ctx(lb_gpu_pq *p, int64_t nq, const float *queries, int k, float *dist, int64_t *labels,
                         const lb_cancel *ctx);
/* Concurrent host-pointer ADC searches are combined like lb_gpu_index_search's (lb_gpu_index_set_search_combining): queued calls
 * with the same k are answered by one batch, in which two queries share each pass over the codes.  On by default. */
int lb_gpu_pq_set_search_combining(lb_gpu_pq *p, int enable);
int lb_gpu_pq_combining_stats(const lb_gpu_pq *p, int64_t out[2]);
int lb_gpu_pq_search_device_ctx(lb_gpu_pq *p, int64_t nq, const float *d_queries, int k, float *d_dist,
                                int64_t *d_labels, void *stream, const lb_cancel *ctx);
/* 1 (default): the search runs the byte-table prefilter + exact survivors; 0: the exact f32-table
 * pass over every row.  Results are bit-identical; the switch exists for A/B timing and for the parity tests. */
int lb_gpu_pq_set_prefilter(lb_gpu_pq *p, int enable);
/* What served the queries of the last COMPLETED device batch on this handle (a refused, cancelled or failed search
 * leaves the previous record; observing only, the PQ counterpart of
 * lb_gpu_index_last_fallbacks / last_route), in queries: out[0] planned with a sampled threshold (nq or 0),
 * out[1] served by a four-query prefilter pass, out[2] by a two-query pass, out[3] by a single prefilter pass
 * (including quads and pairs whose M has no shared form), out[4] redone on the bootstrap schedule, out[5] redone
 * on the schedule that cannot overflow.  Concurrent searches overwrite each other's record. */
int lb_gpu_pq_last_search_stats(const lb_gpu_pq *p, int64_t out[6]);
/* The row filter of a PQ handle, with the prototypes and the semantics of lb_gpu_bq_set_filter / _filter_int64 / _filter_float32 /
 * _nvisible (and of lb_gpu_index_set_filter / _filter_*): a row is visible iff its mask byte is non-zero; a NULL mask clears the
 * filter; n != ntotal is LB_ERR_INVALID_ARG with a last_error text and leaves the filter as it was.
 *   search    with a filter every lb_gpu_pq_search* call (_device, _ctx and combined concurrent host searches too) returns the
 *             exact ADC k-NN among the visible rows: the distances of the unfiltered search, ascending by (distance, row),
 *             labels are corpus rows.  Fewer than k visible rows: they come first, then label -1 / dist FLT_MAX; no visible
 *             row: all padding.  lb_gpu_pq_last_search_stats reports as without a filter; there is no four-query pass over a
 *             list, so out[1] == 0.
 *   adds      rows added under a filter are visible.
 *   ignored   rerank*, adc_distance_batch, get_codes, encode and decode address rows directly and ignore the filter.
 *   cost      any filter, an all-visible one too, searches the ascending list of visible rows, so the cost follows their number.
 *   limits    the list holds fewer than 2^31 rows: a filter call on a handle with more, and an add that would take a filtered
 *             handle there, answer LB_ERR_UNSUPPORTED with a last_error text before the device is touched.  A handle without
 *             a filter keeps its 2^32 - 1 rows.
 *   locking   the filter calls are exclusive against everything else on the handle; searches and reads share it. */
int lb_gpu_pq_set_filter(lb_gpu_pq *p, const uint8_t *mask, int64_t n);
int lb_gpu_pq_filter_int64(lb_gpu_pq *p, const int64_t *column, int64_t n, int64_t value, int op, const uint8_t *validity,
                           int64_t validity_offset, int combine);
int lb_gpu_pq_filter_float32(lb_gpu_pq *p, const float *column, int64_t n, float value, int op, const uint8_t *validity,
                             int64_t validity_offset, int combine);
/* rows a search sees: ntotal without a filter; 0 for a NULL handle */
int64_t lb_gpu_pq_nvisible(const lb_gpu_pq *p);

/* instrumentation (bench.py): HIP-event times of the most recent profiled search on this handle, recorded on the
 * search stream: ms[0] = the pass over the codes of the LAST query (prefilter kernel, or the exact kernel when
 * the prefilter is off), ms[1] = the whole search on the device.  Enable before the search; one search at a time. */
int lb_gpu_pq_set_profiling(lb_gpu_pq *p, int enable);
int lb_gpu_pq_last_timing(const lb_gpu_pq *p, float ms[2]);

/* ---- PQ training --------------------------------------------------------------
 * pq.(*PQEncoder).Train (encoder.go:38-73): TrainKMeans (kmeans.go:64-151) per subspace.  vectors: n rows of f32[dims];
 * subspace m trains on the sub-vectors v_i = row_i[m*sub, (m+1)*sub), sub = dims / M, exactly as TrainKMeans(., n, sub, K,
 * max_iter) does (TrainKMeans itself is the case M = 1):
 *   init    centroid c = the copy of row init_rows[m*K + c]  (init_rows: HOST pointer in both entry points; duplicates allowed)
 *   E-step  dist = simd.L2Squared(v_i, cent_c) (four f32 chains over i mod 4, tail in chain 0, ((s0+s1)+s2)+s3, no sqrt);
 *           the row goes to the first c with dist < best, best starting at FLT_MAX.  (Not lb_gpu_pq_encode's argmin, which
 *           compares the rounded square roots.)  A row with no such centroid (NaN, overflow) makes the reference panic;
 *           here the call returns LB_ERR_INVALID_ARG and writes nothing.
 *   M-step  sums[c][j] += v_i[j] as ONE f32 chain over the cluster's members in ascending row order, then
 *           cent = sum / float32(count); an empty cluster takes the copy of a drawn row.
 *   stop    after an iteration with iter > 0 && changed < n/1000 + 1 (rows whose assignment differs from the previous
 *           iteration's, assignments starting at -1), or after max_iter iterations; max_iter == 0 returns the init rows.
 *           Subspaces stop independently; iters_out[m] (nullable) = iterations subspace m ran.
 * The reference draws from Go's unseeded global source, so its draws cannot be reproduced; they are restated counter-based:
 *   mix64(z): z = (z ^ z>>30) * 0xBF58476D1CE4E5B9; z = (z ^ z>>27) * 0x94D049BB133111EB; z ^ z>>31   (splitmix64's finaliser)
 *   draw(seed, m, t) = mix64(mix64(seed + m) + (t + 1) * 0x9E3779B97F4A7C15)                          (u64 arithmetic)
 *   init_rows == NULL: subspace m's rows are the first K entries of a Fisher-Yates shuffle of [0, n):
 *                      for i in 0..K-1: j = i + draw(seed, m, i) mod (n - i), swap entries i and j
 *   empty cluster c in iteration it: row draw(seed, m, K + it*K + c) mod n
 * blob receives the persistence.go layout that lb_gpu_pq_new reads; blob_len must equal lb_gpu_pq_blob_bytes(dims, M, K)
 * (12 + M*K*(dims/M)*4; 0 for dims, M or K <= 0 or dims % M != 0).  K is a run-time bound in 1..256 (the reference's own
 * tests train k = 3): a blob with K != 256 serialises correctly and is still refused by lb_gpu_pq_new.
 * Checked before a device is touched, in this order: LB_ERR_INVALID_ARG (NULL vectors / blob, M <= 0, dims % M != 0, n < K,
 * max_iter < 0, blob_len, an init_rows entry outside [0, n)); LB_ERR_UNSUPPORTED (K outside 1..256, dims > LB_MAX_DIM,
 * n >= 2^31); LB_ERR_NO_DEVICE.  All rows stay resident for the iterations (n*dims*4 bytes, plus 8 bytes per row and
 * subspace): LB_ERR_OOM if they do not fit.  ctx (nullable) is polled once per iteration. */
int lb_gpu_pq_train(int device, int dims, int M, int K, int64_t n, const float *vectors, int max_iter, uint64_t seed,
                    const int64_t *init_rows, uint8_t *blob, size_t blob_len, int32_t *iters_out, const lb_cancel *ctx);
int lb_gpu_pq_train_device(int device, int dims, int M, int K, int64_t n, const float *d_vectors, int max_iter, uint64_t seed,
                           const int64_t *init_rows, uint8_t *blob, size_t blob_len, int32_t *iters_out, void *stream,
                           const lb_cancel *ctx);
size_t lb_gpu_pq_blob_bytes(int dims, int M, int K);
/* instrumentation (tools/pq_train_bench.py): HIP-event times of the first iteration of the last training call of this
 * process that ran one: ms[0] E-step, ms[1] ordering (scan + scatter), ms[2] M-step. */
int lb_gpu_pq_train_last_timing(float ms[3]);

/* ---- coarse quantiser training ---------------------------------------------------
 * pq.TrainKMeans(vectors, n, dims, nlist, max_iter) (kmeans.go:64-151) for the centroids of the IVF handles, nlist in 1..65,536.
 * It is the lb_gpu_pq_train block above with M = 1, m = 0, sub = dims and K = nlist, the centroids returned as plain f32
 * instead of a blob:
 *   init    centroid c = the copy of row init_rows[c] (HOST pointer in both entry points; duplicates allowed).  init_rows ==
 *           NULL: the first nlist entries of the Fisher-Yates shuffle of [0, n) stated above, with draw(seed, 0, i).
 *   E-step  s = simd.L2Squared(row, cent_c): four f32 chains over i mod 4, tail elements in chain 0, ((s0+s1)+s2)+s3, no sqrt,
 *           no FMA contraction; the row goes to the first c with s < best, best starting at FLT_MAX.  A row with no such
 *           centroid (NaN, overflow) makes the call return LB_ERR_INVALID_ARG and write nothing.
 *   M-step  ONE sequential f32 chain per (cluster, element) over the members in ascending row order, then
 *           sum / float32(count); an empty cluster c in iteration it takes the copy of row draw(seed, 0, nlist + it*nlist + c) mod n.
 *   stop    after an iteration with it > 0 && changed < n/1000 + 1, or after max_iter iterations; max_iter == 0 returns the
 *           init rows.  *iters_out (nullable, one value) = iterations run.
 * centroids: HOST pointer in both entry points, f32[nlist * dims].  For nlist <= 256 the result equals
 * lb_gpu_pq_train(device, dims, 1, nlist, ...) byte for byte (that blob's bytes 12 onwards), with equal iteration counts.
 * Checked before a device is touched, in this order: LB_ERR_INVALID_ARG (NULL vectors / centroids, dims <= 0, nlist <= 0,
 * n < nlist, max_iter < 0, an init_rows entry outside [0, n)); LB_ERR_UNSUPPORTED (nlist > 65536, dims > LB_MAX_DIM,
 * n >= 2^31); LB_ERR_NO_DEVICE.  A refused or cancelled call writes neither centroids nor iters_out.  All rows stay resident
 * for the iterations (n*dims*4 bytes); beside them the call holds 8 bytes per row, the ordering's histogram (at most 2^24
 * counters) and nlist*dims*4 bytes: LB_ERR_OOM if they do not fit.  ctx (nullable) is polled before every launch of an
 * iteration (E-step, ordering, M-step, finish), since one iteration can be long at this shape. */
int lb_gpu_ivf_train(int device, int dims, int nlist, int64_t n, const float *vectors, int max_iter, uint64_t seed,
                     const int64_t *init_rows, float *centroids, int32_t *iters_out, const lb_cancel *ctx);
int lb_gpu_ivf_train_device(int device, int dims, int nlist, int64_t n, const float *d_vectors, int max_iter, uint64_t seed,
                            const int64_t *init_rows, float *centroids, int32_t *iters_out, void *stream, const lb_cancel *ctx);
/* instrumentation (tools/ivf_train_bench.py): HIP-event times of the first iteration of the last lb_gpu_ivf_train* call of this
 * process that ran one: ms[0] E-step, ms[1] ordering (sort + counts), ms[2] M-step. */
int lb_gpu_ivf_train_last_timing(float ms[3]);

/* ---- binary quantisation: sign-bit codes and exact Hamming k-NN ------------------------
 * store.BQEncoder (internal/store/binary_quantization.go) and simd.HammingDistance (internal/simd/simd_bitops.go:40-55),
 * which the HNSW build and search use as float32(HammingDistance(q, t)) when BQEnabled is set
 * (internal/store/arrow_hnsw_bulk.go:420-476).  Everything here is integer-exact: there is no tolerance and no fallback.
 *   layout    W = (dims + 63) / 64 little-endian uint64 words per row, row-major; bit i % 64 of word i / 64 is dimension i
 *             (binary_quantization.go:34-45).  CodeSize() is lb_gpu_bq_words.
 *   encode    the bit is set iff v[i] > 0 as an f32 comparison (binary_quantization.go:41): +0, -0, NaN, every negative value
 *             and -inf give 0, +inf and positive denormals give 1 (denormals are not flushed); pad bits of the last word are 0.
 *   distance  sum over all W whole words of popcount(a[w] ^ b[w]) (simd_bitops.go:40-55): pad bits that a caller put into
 *             codes passed to add_codes count.  Integer results are int32; searches and rerank report float32(distance),
 *             exact because the distance is at most 8192.
 *   score     1.0f - float32(h) / float32(dims) in f32 operations (ScoreToFloat32, binary_quantization.go:69-71).
 *   decode    bit 1 -> 1.0f, bit 0 -> -1.0f, dims values per row (binary_quantization.go:80-92).
 *   search    exact k-NN of each query over all stored codes, ascending by (distance, row position): the lowest position
 *             wins every tie (as lb_gpu_index_search).  Labels are row positions.  Fewer than k rows: label -1, dist FLT_MAX.
 *   filter    a row filter on the handle, with the semantics of lb_gpu_index_set_filter / _filter_*: a row is visible iff its mask
 *             byte is non-zero; a NULL mask clears the filter; n != ntotal is LB_ERR_INVALID_ARG with a last_error text and leaves
 *             the filter as it was.  Rows added after a filter was set are visible.  With a filter, every search* call returns
 *             the exact k-NN among the visible rows: the same distances, the same tie rule (the lowest rows win), labels are
 *             corpus rows.  Fewer than k visible rows: they come first, then label -1 / dist FLT_MAX; no visible row: all padding.
 *             hamming_batch, rerank*, get_codes and the codec address rows directly and ignore the filter.  Any filter, an
 *             all-visible one too, searches the ascending list of visible rows, so the cost follows their number.
 *   limits    dims in 1..LB_MAX_DIM, k in 1..LB_MAX_K, fewer than 2^31 rows per handle: LB_ERR_UNSUPPORTED beyond.
 * Argument checks answer before a device is touched: LB_ERR_INVALID_ARG (NULL handle or pointer, dims <= 0, k <= 0, negative
 * counts, rows outside the stored ones) before LB_ERR_UNSUPPORTED before LB_ERR_NO_DEVICE, the order of lb_gpu_pq_train.  A
 * refused call writes nothing.  Host pointers are borrowed for the call; d_ pointers are device memory.  Searches, reads and
 * rerank are thread-safe against each other and exclusive against reserve, the add calls and the filter calls. */
typedef struct lb_gpu_bq lb_gpu_bq;
lb_gpu_bq *lb_gpu_bq_new(int device, int dims, int *out_status);
void lb_gpu_bq_free(lb_gpu_bq *p);
const char *lb_gpu_bq_last_error(const lb_gpu_bq *p);
int lb_gpu_bq_dims(const lb_gpu_bq *p);
int lb_gpu_bq_words(const lb_gpu_bq *p);
int64_t lb_gpu_bq_ntotal(const lb_gpu_bq *p);
int lb_gpu_bq_reserve(lb_gpu_bq *p, int64_t n_total);
/* append n codes u64[n*W] as they are (pad bits included) */
int lb_gpu_bq_add_codes(lb_gpu_bq *p, int64_t n, const uint64_t *codes);
int lb_gpu_bq_add_codes_device(lb_gpu_bq *p, int64_t n, const uint64_t *d_codes);
/* stored rows [row0, row0+n) -> u64[n*W] */
int lb_gpu_bq_get_codes(lb_gpu_bq *p, int64_t row0, int64_t n, uint64_t *codes);
/* BQEncoder.Encode for n rows of f32[dims] -> u64[n*W]; nothing is stored */
int lb_gpu_bq_encode(lb_gpu_bq *p, int64_t n, const float *vectors, uint64_t *codes);
int lb_gpu_bq_encode_device(lb_gpu_bq *p, int64_t n, const float *d_vectors, uint64_t *d_codes, void *stream);
/* encode n rows and append their codes */
int lb_gpu_bq_add_vectors(lb_gpu_bq *p, int64_t n, const float *vectors);
int lb_gpu_bq_add_vectors_device(lb_gpu_bq *p, int64_t n, const float *d_vectors);
/* BQEncoder.Decode: u64[n*W] -> f32[n*dims] */
int lb_gpu_bq_decode(lb_gpu_bq *p, int64_t n, const uint64_t *codes, float *vectors);
/* BQEncoder.HammingDistanceBatch (binary_quantization.go:56-60) of qcode u64[W] over the stored rows [row0, row0+n) */
int lb_gpu_bq_hamming_batch(lb_gpu_bq *p, const uint64_t *qcode, int64_t row0, int64_t n, int32_t *results);
/* the stored rows rows[0..n): dist = float32(distance), score (nullable) = ScoreToFloat32; rows outside [0, ntotal) report
 * FLT_MAX / 0, as lb_gpu_pq_rerank */
int lb_gpu_bq_rerank(lb_gpu_bq *p, const uint64_t *qcode, const int64_t *rows, int64_t n, float *dist, float *score);
int lb_gpu_bq_rerank_device(lb_gpu_bq *p, const uint64_t *d_qcode, const int64_t *d_rows, int64_t n, float *d_dist, float *d_score,
                            void *stream);
/* k-NN of nq query codes u64[nq*W] -> dist f32[nq*k], labels i64[nq*k] */
int lb_gpu_bq_search_codes(lb_gpu_bq *p, int64_t nq, const uint64_t *qcodes, int k, float *dist, int64_t *labels);
/* k-NN of nq queries f32[nq*dims], which are encoded on the device first.  ctx (nullable) is polled before every launch; one
 * that has already fired returns LB_ERR_CANCELLED / LB_ERR_DEADLINE without launching anything. */
int lb_gpu_bq_search(lb_gpu_bq *p, int64_t nq, const float *queries, int k, float *dist, int64_t *labels);
int lb_gpu_bq_search_ctx(lb_gpu_bq *p, int64_t nq, const float *queries, int k, float *dist, int64_t *labels, const lb_cancel *ctx);
int lb_gpu_bq_search_device_ctx(lb_gpu_bq *p, int64_t nq, const float *d_queries, int k, float *d_dist, int64_t *d_labels, void *stream,
                                const lb_cancel *ctx);
/* the row filter: mask u8[ntotal] of the host (NULL clears it) */
int lb_gpu_bq_set_filter(lb_gpu_bq *p, const uint8_t *mask, int64_t n);
/* a predicate evaluated on the device into the mask: arguments, null rule and combine as lb_gpu_index_filter_int64 / _float32
 * (column has ntotal host values, op is an lb_compare_op, validity an Arrow bitmap read from bit validity_offset on or NULL,
 * nulls never match; combine 0 replaces the mask, 1 ANDs into it bytewise, and on a handle without a filter replaces it) */
int lb_gpu_bq_filter_int64(lb_gpu_bq *p, const int64_t *column, int64_t n, int64_t value, int op, const uint8_t *validity,
                           int64_t validity_offset, int combine);
int lb_gpu_bq_filter_float32(lb_gpu_bq *p, const float *column, int64_t n, float value, int op, const uint8_t *validity,
                             int64_t validity_offset, int combine);
/* rows a search sees: ntotal without a filter; 0 for a NULL handle */
int64_t lb_gpu_bq_nvisible(const lb_gpu_bq *p);

/* ---- scalar quantisation: uint8 codes and exact integer k-NN ----------------------------
 * store.SQ8Encoder (internal/store/scalar_quantization.go) and simd.EuclideanDistanceSQ8 (internal/simd/sq8.go:45-66): one
 * uint8 per dimension between per-dimension bounds.  Codes, integer distances and labels are exact: no tolerance, no fallback.
 *   layout    dims bytes per row, row-major, in every buffer a caller passes or receives (the store pads rows to 16 bytes
 *             with zero bytes internally; get_codes strips them).  Device code pointers are 16-byte aligned.
 *   bounds    train = TrainSQ8Encoder (:89-134): per dimension min and max start at row 0 and later rows replace them through
 *             v < min / v > max, so a NaN in a later row is ignored and a NaN in row 0 stays; min == max becomes
 *             max = min + 1e-7f; then Validate (:29-52): min >= max in any dimension is LB_ERR_INVALID_ARG ("min must be less
 *             than max for all dimensions": a constant column of magnitude 2.0 or more fails), NaN bounds pass.  No rows:
 *             LB_ERR_INVALID_ARG.  Where a column holds both -0 and +0 a zero bound may carry either sign: it compares equal
 *             to the reference's and changes no code and no decoded value.  The result is the same from run to run.
 *             set_bounds = NewSQ8Encoder (:62-86) on given bounds.  scale = 255 / (max - min) and invScale = (max - min) / 255
 *             are f32 divisions.  Bounds cannot change once the handle holds rows.
 *   encode    EncodeInto (:155-170): v clamped by `if v < min: min, else if v > max: max` (a NaN passes both), then
 *             uint8((v - min) * scale), subtraction and product each rounded once in f32, truncated toward zero.  Go leaves
 *             the conversion of a value outside the target type to the platform; a NaN product gives code 0 on amd64 and
 *             arm64 alike, and an infinite product (bounds so close that scale overflows) gives 0 as on amd64.
 *   decode    DecodeInto (:180-184): min + float32(q) * invScale, the product rounded before the sum (the amd64 form).
 *   distance  S = sum (a_i - b_i)^2 as int32 (EuclideanSQ8Generic == SQ8DistanceFast, :208-216); at most 65025 * 8192 < 2^31.
 *             euclid = SQ8EuclideanDistance (:192-203): the sequential f32 sum of diff * diff over the decoded values, then
 *             float32(sqrt(float64(sum))).
 *   search    exact k-NN over all stored codes, ascending by (S, row position): the lowest position wins every tie.  The
 *             reported distance is float32(S) (EuclideanDistanceSQ8Batch, internal/simd/simd.go:170-182): two different S may
 *             round to one float, the order is the integers'.  Fewer than k rows: label -1, dist FLT_MAX.
 *   filter    a row filter on the handle, with the semantics of lb_gpu_index_set_filter / _filter_*: a row is visible iff its mask
 *             byte is non-zero; a NULL mask clears the filter; n != ntotal is LB_ERR_INVALID_ARG with a last_error text and leaves
 *             the filter as it was.  Rows added after a filter was set are visible.  With a filter, every search* call returns
 *             the exact k-NN among the visible rows: the same distances, the same tie rule (the lowest rows win), labels are
 *             corpus rows.  Fewer than k visible rows: they come first, then label -1 / dist FLT_MAX; no visible row: all padding.
 *             distance_batch, rerank*, get_codes and the codec address rows directly and ignore the filter.  Any filter, an
 *             all-visible one too, searches the ascending list of visible rows, so the cost follows their number.
 *   limits    dims in 1..LB_MAX_DIM, k in 1..LB_MAX_K, fewer than 2^31 rows per handle: LB_ERR_UNSUPPORTED beyond.
 * Calls on codes alone (add_codes, get_codes, distance_batch, rerank without euclid, search_codes, the filter calls) work on an
 * untrained handle; whatever encodes or decodes answers LB_ERR_INVALID_ARG ("config must be trained ...") on one.  Argument checks
 * answer before a device is touched, LB_ERR_INVALID_ARG before LB_ERR_UNSUPPORTED before LB_ERR_NO_DEVICE, and a refused call
 * writes nothing.  Host pointers are borrowed for the call; d_ pointers are device memory.  Searches, reads and the codec are
 * thread-safe against each other and exclusive against reserve, the add calls, set_bounds, train and the filter calls. */
typedef struct lb_gpu_sq8 lb_gpu_sq8;
lb_gpu_sq8 *lb_gpu_sq8_new(int device, int dims, int *out_status); /* untrained */
void lb_gpu_sq8_free(lb_gpu_sq8 *p);
const char *lb_gpu_sq8_last_error(const lb_gpu_sq8 *p);
int lb_gpu_sq8_dims(const lb_gpu_sq8 *p);
int64_t lb_gpu_sq8_ntotal(const lb_gpu_sq8 *p);
int lb_gpu_sq8_reserve(lb_gpu_sq8 *p, int64_t n_total);
int lb_gpu_sq8_trained(const lb_gpu_sq8 *p);
int lb_gpu_sq8_set_bounds(lb_gpu_sq8 *p, const float *min, const float *max); /* f32[dims] each */
int lb_gpu_sq8_train(lb_gpu_sq8 *p, int64_t n, const float *vectors);         /* f32[n*dims] */
int lb_gpu_sq8_train_device(lb_gpu_sq8 *p, int64_t n, const float *d_vectors);
int lb_gpu_sq8_get_bounds(lb_gpu_sq8 *p, float *min, float *max);
/* SQ8Encoder.Encode for n rows of f32[dims] -> u8[n*dims]; nothing is stored */
int lb_gpu_sq8_encode(lb_gpu_sq8 *p, int64_t n, const float *vectors, uint8_t *codes);
int lb_gpu_sq8_encode_device(lb_gpu_sq8 *p, int64_t n, const float *d_vectors, uint8_t *d_codes, void *stream);
/* SQ8Encoder.Decode: u8[n*dims] -> f32[n*dims] */
int lb_gpu_sq8_decode(lb_gpu_sq8 *p, int64_t n, const uint8_t *codes, float *vectors);
/* append n codes u8[n*dims] as they are */
int lb_gpu_sq8_add_codes(lb_gpu_sq8 *p, int64_t n, const uint8_t *codes);
int lb_gpu_sq8_add_codes_device(lb_gpu_sq8 *p, int64_t n, const uint8_t *d_codes);
/* encode n rows and append their codes */
int lb_gpu_sq8_add_vectors(lb_gpu_sq8 *p, int64_t n, const float *vectors);
int lb_gpu_sq8_add_vectors_device(lb_gpu_sq8 *p, int64_t n, const float *d_vectors);
/* stored rows [row0, row0+n) -> u8[n*dims] */
int lb_gpu_sq8_get_codes(lb_gpu_sq8 *p, int64_t row0, int64_t n, uint8_t *codes);
/* S of qcode u8[dims] against the stored rows [row0, row0+n) */
int lb_gpu_sq8_distance_batch(lb_gpu_sq8 *p, const uint8_t *qcode, int64_t row0, int64_t n, int32_t *out);
/* the stored rows rows[0..n): s = S, euclid (nullable; needs a trained handle) = SQ8EuclideanDistance; rows outside
 * [0, ntotal) report INT32_MAX / FLT_MAX */
int lb_gpu_sq8_rerank(lb_gpu_sq8 *p, const uint8_t *qcode, const int64_t *rows, int64_t n, int32_t *s, float *euclid);
int lb_gpu_sq8_rerank_device(lb_gpu_sq8 *p, const uint8_t *d_qcode, const int64_t *d_rows, int64_t n, int32_t *d_s, float *d_euclid,
                             void *stream);
/* k-NN of nq query codes u8[nq*dims] -> dist f32[nq*k], labels i64[nq*k] */
int lb_gpu_sq8_search_codes(lb_gpu_sq8 *p, int64_t nq, const uint8_t *qcodes, int k, float *dist, int64_t *labels);
/* k-NN of nq queries f32[nq*dims], which are encoded on the device first (a trained handle).  ctx (nullable) is polled before
 * every launch; one that has already fired returns LB_ERR_CANCELLED / LB_ERR_DEADLINE without launching anything. */
int lb_gpu_sq8_search(lb_gpu_sq8 *p, int64_t nq, const float *queries, int k, float *dist, int64_t *labels);
int lb_gpu_sq8_search_ctx(lb_gpu_sq8 *p, int64_t nq, const float *queries, int k, float *dist, int64_t *labels, const lb_cancel *ctx);
int lb_gpu_sq8_search_device_ctx(lb_gpu_sq8 *p, int64_t nq, const float *d_queries, int k, float *d_dist, int64_t *d_labels, void *stream,
                                 const lb_cancel *ctx);
/* the row filter, as lb_gpu_bq_set_filter / _filter_int64 / _filter_float32 / _nvisible */
int lb_gpu_sq8_set_filter(lb_gpu_sq8 *p, const uint8_t *mask, int64_t n);
int lb_gpu_sq8_filter_int64(lb_gpu_sq8 *p, const int64_t *column, int64_t n, int64_t value, int op, const uint8_t *validity,
                            int64_t validity_offset, int combine);
int lb_gpu_sq8_filter_float32(lb_gpu_sq8 *p, const float *column, int64_t n, float value, int op, const uint8_t *validity,
                              int64_t validity_offset, int combine);
int64_t lb_gpu_sq8_nvisible(const lb_gpu_sq8 *p);

/* ---- IVF-Flat: exact k-NN over the probed lists ---------------------------------------------
 * The index type the reference names and leaves empty: IndexTypeIVFFlat = "ivf_flat" and IVFFlatConfig{NClusters, NProbe}
 * (internal/store/pluggable_index.go:18-25,100-104); its adapter (pluggable_index_adapters.go:116-223) is a stub.  A coarse
 * partition of the rows lets a query skip most of them.  Nothing is approximate except WHICH lists are probed: given the probed
 * lists the result is the exact k-NN among their rows, bit for bit in the reference's distance arithmetic.
 * A handle has a metric (0 L2, 1 cosine, 2 dot, as lb_gpu_index_new), an accumulation order (0 SEQ, 1 UNROLL4, as
 * lb_gpu_index_set_order; fixed at creation because it decides which list a row goes to), nlist centroids C (f32 [nlist][dim],
 * given by the caller) and rows X in insertion order.  Write d(a, b) for the distance lb_gpu_index_search reports for query a and
 * row b under that metric and order (L2 with its square root, 1 - cos, -dot); the canonical order is ascending (distance,
 * position), every NaN after +inf.
 *   list of a row     the label of the k = 1 search of the row, as a query, over an f32 index that holds C: the first c in
 *                     canonical order of (d(x, C_c), c).  Computed when the row is added; it never changes.
 *   probes of a query the labels of the k = min(nprobe, nlist) search of the query over that same index.
 *   result            the first k rows r, in canonical order of (d(q, X_r), r), among the rows whose list is a probe of q; the
 *                     label is ids[r] when ids were given, else r; with fewer than k such rows they come first, then label -1 /
 *                     distance FLT_MAX.  nprobe >= nlist gives lb_gpu_index_search over the same rows, bit for bit: labels,
 *                     order and distances.
 *   ids               given on every add or on none; a call that breaks this is LB_ERR_INVALID_ARG and adds nothing.
 *   add               appends the rows, takes their lists and rebuilds the lists of ALL rows by a stable counting sort (each list
 *                     holds its rows ascending): O(ntotal) per call, so add in large pieces.  The rows become visible only once
 *                     all of it succeeded.
 *   filter            a row filter on the handle, with the mask, null and combine rules of lb_gpu_bq_set_filter / _filter_*: a
 *                     row is visible iff its mask byte is non-zero; a NULL mask clears the filter; n != ntotal is
 *                     LB_ERR_INVALID_ARG with a last_error text and leaves the filter as it was; a predicate's nulls never match;
 *                     combine 0 replaces the mask, 1 ANDs into it and replaces when there is none.  The probes of a query do not
 *                     change: a probed list with no visible row contributes nothing and no other list takes its place.  The
 *                     result is the first k rows in canonical order among the VISIBLE rows whose list is a probe, with the same
 *                     labels, padding and distances, bit for bit; nprobe >= nlist gives lb_gpu_index_search on an index that
 *                     holds the same rows under the same mask (lb_gpu_index_set_filter).  Rows added after a filter was set are
 *                     visible; such an add commits the rows, the lists and the visible lists together or not at all.
 *                     list_sizes, assignments, get_centroids and ntotal ignore the filter; nvisible is the number of rows a search
 *                     can see (ntotal without a filter).  Any filter, an all-visible one too, searches the visible lists (each
 *                     list's visible rows, ascending, built on the device by every filter call and every add under a filter), so
 *                     the cost follows the visible rows of the probed lists, and last_search_stats counts those.
 *   limits            dim in 1..LB_MAX_DIM, nlist in 1..65536, k in 1..LB_MAX_K, fewer than 2^31 rows: LB_ERR_UNSUPPORTED
 *                     beyond.  nprobe <= 0 is LB_ERR_INVALID_ARG, nprobe > nlist is clamped.  Fewer than all lists are at most
 *                     LB_MAX_K probes (the coarse search's k; LB_ERR_UNSUPPORTED beyond); every list probed needs no coarse
 *                     search and works for any nlist.
 * Argument checks answer before a device is touched, LB_ERR_INVALID_ARG before LB_ERR_UNSUPPORTED before LB_ERR_NO_DEVICE, and a
 * refused call writes nothing.  Searches and reads share the handle; adds, reserve and the filter calls take it alone.  ctx
 * (nullable) is polled before every launch.  Host pointers are borrowed for the call; d_ pointers are device memory.
 *   float16 rows      lb_gpu_ivf_new_f16 takes what lb_gpu_ivf_new takes, with the same checks in the same order, and makes a
 *                     handle whose rows are IEEE binary16, 2 bytes an element and no f32 copy of them (simd.VectorTypeFloat16).
 *                     They cross the ABI as uint16_t bit patterns through lb_gpu_ivf_add_f16 / _add_f16_device, as on
 *                     lb_gpu_index_add_f16; lb_gpu_ivf_add / _add_device on such a handle, and the _f16 adds on a float32
 *                     handle, are LB_ERR_INVALID_ARG with a last_error text that names the handle's element type.  The
 *                     centroids, the coarse index and the QUERIES stay f32 on both handle types: a caller with fp16 queries
 *                     widens them, which is exact.  Every element is widened to f32 and enters the f32 arithmetic above (the
 *                     reference's *F16Unrolled4x functions do the same), so every call on such a handle gives what the same call
 *                     gives on a float32 handle that holds the widened rows, bit for bit: labels, distances, assignments, list
 *                     sizes, search stats.  With fp16-representable queries the distances are the reference's F16 functions',
 *                     and nprobe >= nlist gives lb_gpu_index_search of a float16 index (lb_gpu_index_new_f16) over the same
 *                     rows.  Every other lb_gpu_ivf_* entry point works on both handle types.
 *   int8 rows         lb_gpu_ivf_new_i8 makes a handle whose rows are signed int8, one byte an element, row-major in insertion
 *                     order, and no wider copy of them (simd.VectorTypeInt8).  Metrics L2 (0) and dot (2) only: cosine, and dot
 *                     with floor(dim / 4) + dim mod 4 > 1024, are LB_ERR_UNSUPPORTED, the rules of lb_gpu_index_new_i8 for its
 *                     reasons, answered with the other limits (after LB_ERR_INVALID_ARG, before LB_ERR_NO_DEVICE).  Rows go in
 *                     through lb_gpu_ivf_add_i8 / _add_i8_device and the QUERIES are int8 too, through lb_gpu_ivf_search_i8 /
 *                     _search_i8_ctx / _search_i8_device_ctx, each taking what its float32 counterpart takes.  The float32 and
 *                     _f16 adds and the float32 searches on such a handle, and the _i8 adds and searches on a float32 or
 *                     float16 handle, are LB_ERR_INVALID_ARG with a last_error text that names the handle's element type, and
 *                     write nothing.  The centroids and the coarse index stay f32 and `order` is the coarse index's: the list
 *                     of a row and the probes of a query are those of the row / query widened to f32, which is exact, so
 *                     assignments and list sizes equal those of a float32 handle over the widened rows, bit for bit.  `order`
 *                     does not reach the row distances: d(q, x) is the one lb_gpu_index_search_i8 reports, in the reference's
 *                     DataTypeInt8 arithmetic (L2: euclideanInt8AVX2Kernel, the sum over the first 16 floor(dim / 16) elements
 *                     an exact int32 rounded once to f32, the tail added in f32 in order, sqrt correctly rounded; dot:
 *                     dotInt8Unrolled4x, negated).  Result, labels, padding, ids, filters and stats are as stated above, and
 *                     nprobe >= nlist gives lb_gpu_index_search_i8 of an int8 index (lb_gpu_index_new_i8) over the same rows,
 *                     bit for bit.  Every other lb_gpu_ivf_* entry point works on all three handle types.
 *   call bitmap       lb_gpu_ivf_search_bitmap_ctx / _bitmap_device_ctx and, on an int8 handle, _search_i8_bitmap_ctx /
 *                     _i8_bitmap_device_ctx take what their plain counterparts take, and behind nprobe a row filter of THIS CALL
 *                     alone: (bitmap, nbits, stride_bytes).  One bit per row POSITION, as the handle filter's mask is by position,
 *                     least significant bit first as in an Arrow validity buffer: row r is visible to the call iff
 *                     bitmap[r >> 3] >> (r & 7) & 1.  It is read byte by byte: no alignment is owed and no padding beyond
 *                     ceil(nbits / 8) bytes, and nothing past bit nbits - 1 is read as a row.  stride_bytes 0: one bitmap serves
 *                     every query of the call; otherwise query q reads bitmap + q * stride_bytes (a batch of requests that each
 *                     bring their own filter), and stride_bytes >= ceil(nbits / 8).  The result is the exact k-NN among the rows of
 *                     the probed lists that are live, pass the handle's filter if one is set AND have their bit set; order, labels,
 *                     padding and distances as stated above.  It is bit for bit what the same handle answers after set_filter
 *                     (combined with its own filter) with the mask bit(r) != 0, and last_search_stats agrees in all four values.
 *                     The probes do not change; nprobe >= nlist gives lb_gpu_index_search of a flat index under the same mask.
 *                     The handle is not changed and is held shared, like any search: calls with different bitmaps run
 *                     concurrently, and nvisible, the handle's filter and every later call are untouched.  A NULL bitmap is the
 *                     plain search through the plain path; nbits and stride_bytes are then ignored.  A non-NULL bitmap with
 *                     nbits != ntotal (the n != ntotal rule of set_filter), nbits < 0, a negative stride or a stride in
 *                     (0, ceil(nbits / 8)) is LB_ERR_INVALID_ARG with a last_error text, answered before any launch and with
 *                     nothing written; the other checks, their order and the element-type texts are the plain entry points', and
 *                     they come first.  On the device the probed lists of each batch are compacted under the bitmap into lists of
 *                     the call's own (over the handle's visible lists when it has a filter or removed rows, so the AND costs
 *                     nothing), which the plan, the scan and the selection then walk; scratch is sized by the handle's list sizes,
 *                     nothing returns to the host in between, and the cost of the scan and the selection follows the rows that
 *                     pass.  Under one bitmap (stride_bytes 0), when the call's queries times their largest probed lists exceed
 *                     the rows the handle's lists hold, every list is compacted once for the call, in its first batch, and not
 *                     once per query and probe; a host decision from the list sizes, and the result does not depend on it.
 *                     ctx is polled before these launches as before every other; under profiling they fall into ms[1].
 * Not here: fp16 or int8 centroids, fp16 queries, f32 queries on an int8 handle, predicates (filter_int64 / _float32) given per
 * search call, search combining, lb_gpu_comm_*. */
typedef struct lb_gpu_ivf lb_gpu_ivf;
lb_gpu_ivf *lb_gpu_ivf_new(int device, int dim, int metric, int order, int nlist, const float *centroids, int *out_status);
lb_gpu_ivf *lb_gpu_ivf_new_f16(int device, int dim, int metric, int order, int nlist, const float *centroids, int *out_status);
lb_gpu_ivf *lb_gpu_ivf_new_i8(int device, int dim, int metric, int order, int nlist, const float *centroids, int *out_status);
int lb_gpu_ivf_dtype(const lb_gpu_ivf *p); /* 0 float32, 1 float16, 2 int8 (as lb_gpu_index_dtype); 0 on NULL */
void lb_gpu_ivf_free(lb_gpu_ivf *p);
const char *lb_gpu_ivf_last_error(const lb_gpu_ivf *p);
int lb_gpu_ivf_dim(const lb_gpu_ivf *p);
int lb_gpu_ivf_metric(const lb_gpu_ivf *p);
int lb_gpu_ivf_order(const lb_gpu_ivf *p);
int lb_gpu_ivf_nlist(const lb_gpu_ivf *p);
int64_t lb_gpu_ivf_ntotal(const lb_gpu_ivf *p);
int64_t lb_gpu_ivf_hbm_bytes(const lb_gpu_ivf *p); /* rows (4, 2 or 1 bytes an element), ids, lists, the coarse index and what a row filter holds */
int lb_gpu_ivf_get_centroids(lb_gpu_ivf *p, float *out); /* f32[nlist*dim] */
int lb_gpu_ivf_reserve(lb_gpu_ivf *p, int64_t n_total);
int lb_gpu_ivf_add(lb_gpu_ivf *p, int64_t n, const float *vectors, const int64_t *ids);
int lb_gpu_ivf_add_device(lb_gpu_ivf *p, int64_t n, const float *d_vectors, const int64_t *d_ids);
int lb_gpu_ivf_add_f16(lb_gpu_ivf *p, int64_t n, const uint16_t *vectors, const int64_t *ids); /* a float16 handle's add */
int lb_gpu_ivf_add_f16_device(lb_gpu_ivf *p, int64_t n, const uint16_t *d_vectors, const int64_t *d_ids);
int lb_gpu_ivf_add_i8(lb_gpu_ivf *p, int64_t n, const int8_t *vectors, const int64_t *ids); /* an int8 handle's add */
int lb_gpu_ivf_add_i8_device(lb_gpu_ivf *p, int64_t n, const int8_t *d_vectors, const int64_t *d_ids);
int lb_gpu_ivf_list_sizes(lb_gpu_ivf *p, int64_t *sizes); /* [nlist] */
int lb_gpu_ivf_assignments(lb_gpu_ivf *p, int64_t row0, int64_t n, int32_t *lists); /* the lists of rows [row0, row0 + n) */
int lb_gpu_ivf_search(lb_gpu_ivf *p, int64_t nq, const float *queries, int k, int nprobe, float *dist, int64_t *labels);
int lb_gpu_ivf_search_ctx(lb_gpu_ivf *p, int64_t nq, const float *queries, int k, int nprobe, float *dist, int64_t *labels,
                          const lb_cancel *ctx);
int lb_gpu_ivf_search_device_ctx(lb_gpu_ivf *p, int64_t nq, const float *d_queries, int k, int nprobe, float *d_dist, int64_t *d_labels,
                                 void *stream, const lb_cancel *ctx);
/* an int8 handle's searches: int8 queries */
int lb_gpu_ivf_search_i8(lb_gpu_ivf *p, int64_t nq, const int8_t *queries, int k, int nprobe, float *dist, int64_t *labels);
int lb_gpu_ivf_search_i8_ctx(lb_gpu_ivf *p, int64_t nq, const int8_t *queries, int k, int nprobe, float *dist, int64_t *labels,
                             const lb_cancel *ctx);
int lb_gpu_ivf_search_i8_device_ctx(lb_gpu_ivf *p, int64_t nq, const int8_t *d_queries, int k, int nprobe, float *d_dist,
                                    int64_t *d_labels, void *stream, const lb_cancel *ctx);
/* the same searches under a row bitmap given with the call ("call bitmap" above); d_bitmap is device memory */
int lb_gpu_ivf_search_bitmap_ctx(lb_gpu_ivf *p, int64_t nq, const float *queries, int k, int nprobe, const uint8_t *bitmap, int64_t nbits,
                                 int64_t stride_bytes, float *dist, int64_t *labels, const lb_cancel *ctx);
int lb_gpu_ivf_search_bitmap_device_ctx(lb_gpu_ivf *p, int64_t nq, const float *d_queries, int k, int nprobe, const uint8_t *d_bitmap,
                                        int64_t nbits, int64_t stride_bytes, float *d_dist, int64_t *d_labels, void *stream,
                                        const lb_cancel *ctx);
int lb_gpu_ivf_search_i8_bitmap_ctx(lb_gpu_ivf *p, int64_t nq, const int8_t *queries, int k, int nprobe, const uint8_t *bitmap,
                                    int64_t nbits, int64_t stride_bytes, float *dist, int64_t *labels, const lb_cancel *ctx);
int lb_gpu_ivf_search_i8_bitmap_device_ctx(lb_gpu_ivf *p, int64_t nq, const int8_t *d_queries, int k, int nprobe, const uint8_t *d_bitmap,
                                           int64_t nbits, int64_t stride_bytes, float *d_dist, int64_t *d_labels, void *stream,
                                           const lb_cancel *ctx);
/* the row filter, as lb_gpu_bq_set_filter / _filter_int64 / _filter_float32 / _nvisible */
int lb_gpu_ivf_set_filter(lb_gpu_ivf *p, const uint8_t *mask, int64_t n);
int lb_gpu_ivf_filter_int64(lb_gpu_ivf *p, const int64_t *column, int64_t n, int64_t value, int op, const uint8_t *validity,
                            int64_t validity_offset, int combine);
int lb_gpu_ivf_filter_float32(lb_gpu_ivf *p, const float *column, int64_t n, float value, int op, const uint8_t *validity,
                              int64_t validity_offset, int combine);
int64_t lb_gpu_ivf_nvisible(const lb_gpu_ivf *p);
/* telemetry of the last search only: out[0] queries, out[1] rows scanned summed over the queries, out[2] the largest per-query
 * count, out[3] queries whose selection ran from LDS; under a row filter the rows are the visible ones of the probed lists */
int lb_gpu_ivf_last_search_stats(lb_gpu_ivf *p, int64_t out[4]);
/* instrumentation (tools/ivf_bench.py), as lb_gpu_pq_set_profiling: while on, a search records HIP events between its steps and
 * drains the stream after every batch; last_timing gives the last such search's ms summed over its batches: ms[0] the probes
 * (the coarse search), ms[1] the plan (and the query norms, cosine; and the compaction under a call's bitmap), ms[2] the list
 * scan, ms[3] the selection. */
int lb_gpu_ivf_set_profiling(lb_gpu_ivf *p, int enable);
int lb_gpu_ivf_last_timing(lb_gpu_ivf *p, float ms[4]);
/* while profiling is on, a filter call or an add under a filter also records HIP events around the launches that build the
 * visible lists: *ms is the last such build's time (tools/code_filter_bench.py --index ivf) */
int lb_gpu_ivf_last_build_timing(lb_gpu_ivf *p, float *ms);

/* Removal: rows leave the handle, with the semantics of lb_gpu_index_remove* word for word where they apply.  A removed row keeps
 * its position, its list and its HBM until lb_gpu_ivf_compact; it is live no more, and nothing but compaction undoes that.
 *   remove       labels, the values a search returns: ids[row] when the handle holds ids, else the row position.  With ids EVERY
 *                live row whose id is in the set goes.  _device: the labels are in device memory (on a handle with ids they make a
 *                round trip through the host to be sorted).
 *   remove_rows  row POSITIONS whether or not the handle holds ids.
 *   ignored      an unknown label, a position outside [0, ntotal), -1, a label given twice and a row already removed are ignored,
 *                not errors.
 *   n_removed    nullable; the number of rows this call newly removed.
 *   errors       n == 0 is LB_OK; a NULL handle, n < 0, or n > 0 with a null pointer: LB_ERR_INVALID_ARG, answered before a device
 *                is touched and with nothing written.
 *   searches     every lb_gpu_ivf_search* entry point (host and device forms, _ctx, _i8; float32, float16 and int8 handles)
 *                answers the exact k-NN among the rows of the probed lists that are live AND pass the filter, in ascending
 *                (distance, row position) order: bit for bit what a fresh handle with the same centroids holding only the live
 *                rows, in their order, with ids = the old labels and the same filter restricted to them would answer (without ids
 *                its labels are the survivors' new positions, which old_rows takes back).  The probes do not change: they come
 *                from the centroids alone.  nprobe >= nlist gives lb_gpu_index_search of a flat index over the same rows after the
 *                same removals.  Fewer such rows than k: -1 / FLT_MAX padding.  last_search_stats counts the rows scanned, live
 *                and visible ones only.
 *   filters      set_filter / filter_* keep taking ntotal values (positions do not move) and never resurrect a removed row;
 *                set_filter(NULL) leaves exactly the live rows visible; nvisible counts the rows a search can see, live and
 *                filter-visible.  Should a filter call fail on the device after a removal, searches answer LB_ERR_INTERNAL until
 *                a filter call succeeds, rather than show a removed row.
 *   adds         rows added later are live; an add to a handle with removed rows commits rows, lists, live bytes and visible lists
 *                together or not at all.
 *   list_sizes, assignments, ntotal keep counting removed rows until compaction; nlive = ntotal - ndeleted.
 *   cost         a pass over the labels (positions) or over the handle's ids (labels of a handle with ids), then the row list and
 *                the visible lists are rebuilt as after a filter call; searches then cost what they cost under a filter with the
 *                same visible rows.
 * Exclusive against everything else on the handle, as add and the filter calls. */
int lb_gpu_ivf_remove(lb_gpu_ivf *p, int64_t n, const int64_t *labels, int64_t *n_removed);
int lb_gpu_ivf_remove_device(lb_gpu_ivf *p, int64_t n, const int64_t *d_labels, int64_t *n_removed);
int lb_gpu_ivf_remove_rows(lb_gpu_ivf *p, int64_t n, const int64_t *rows, int64_t *n_removed);
/* ntotal - ndeleted; 0 for a NULL handle */
int64_t lb_gpu_ivf_nlive(const lb_gpu_ivf *p);
/* removed rows the handle still holds (ntotal, list_sizes and assignments count them); 0 for a NULL handle */
int64_t lb_gpu_ivf_ndeleted(const lb_gpu_ivf *p);

/* Compaction: the removed rows leave physically and stably, survivor j being the j-th live row of before, in place (rounds through
 * a bounded scratch: no second copy of the rows is ever resident).  Afterwards ntotal == nlive and ndeleted == 0; a handle with ids
 * keeps every label; a handle WITHOUT ids labels by the new positions.  A filter in force survives, its bytes move with the rows.
 * The handle is then what lb_gpu_ivf_add of the survivors would have made: the same assignments, list sizes and lists, the same
 * results on every search entry point, the same visible lists under the surviving filter.  No row is assigned again: the list of
 * a row depends on the row and the centroids alone, so the stored assignments move with the rows.
 *   old_rows  nullable, room for cap >= nlive entries (else LB_ERR_INVALID_ARG with a last_error text and nothing changed):
 *             receives each survivor's former position, ascending.
 *   nothing removed: LB_OK and nothing changes (old_rows: 0, 1, ...).  Everything removed: the handle is empty and takes adds again.
 *   failure   a refusal before the rows move (an allocation, a list count that does not add up) leaves the handle as it was; once
 *             they move nothing but a device fault fails the call.
 * Exclusive against everything else on the handle. */
int lb_gpu_ivf_compact(lb_gpu_ivf *p, int64_t *old_rows, int64_t cap);

/* ---- IVF-PQ: exact ADC k-NN over the codes of the probed lists ---------------------------------
 * The coarse partition of lb_gpu_ivf_* over the codes of lb_gpu_pq_*: a query skips most rows, and a row costs M bytes instead of
 * 4 * dims.  Nothing is approximate beyond the PQ codes themselves and WHICH lists are probed: given the codes and the probed
 * lists the result is the exact ADC k-NN among their rows, bit for bit in the reference's BuildADCTable / ADCDistanceBatch
 * arithmetic.
 * A handle has PQ codebooks (the reference's serialised blob, as for lb_gpu_pq_new and with its limits: K = 256, M * 1024 bytes
 * fit LDS, dims <= LB_MAX_DIM), nlist centroids C (f32 [nlist][dims], given by the caller), an accumulation order for the coarse
 * quantiser (0 SEQ, 1 UNROLL4, as lb_gpu_index_set_order; fixed at creation because it decides which list a row goes to) and
 * rows in insertion order, of which only the codes are kept.  The coarse metric is L2 (metric 0); ADC is an L2 quantity and the
 * handle takes no metric argument.
 *   code of a row     lb_gpu_pq_encode of the row under the handle's codebooks.
 *   list of a row     as on the IVF-Flat handle: the label of the k = 1 L2 search of the f32 row, as a query, over an f32 index
 *                     that holds C, in the handle's order.  Computed from the vector when the row is added, before the vector is
 *                     dropped; it never changes.
 *   probes of a query the labels of the k = min(nprobe, nlist) search of the query over that same index.
 *   distance          float32(sqrt(float64(sum_j table[j * 256 + code[j]]))), table = BuildADCTable(query), the f32 sum in j
 *                     order: what lb_gpu_pq_search reports.  On a handle from lb_gpu_ivfpq_new these are NOT residual codes: a
 *                     row is encoded as it is, not as its difference from its centroid, and the query's one table serves every
 *                     list.  (Residual codes: lb_gpu_ivfpq_new_residual, below.)
 *   result            the first k rows r, in ascending (distance, r) order, every NaN after +inf, among the rows whose list is a
 *                     probe of q; the label is ids[r] when ids were given, else r; with fewer than k such rows they come first,
 *                     then label -1 / distance FLT_MAX.  nprobe >= nlist gives lb_gpu_pq_search over the same codes, bit for
 *                     bit: labels, order and distances.
 *   ids               given on every add or on none; a call that breaks this is LB_ERR_INVALID_ARG and adds nothing.
 *   add               assigns and encodes the vectors (in pieces of at most 64 Mi floats, so the staging of host vectors stays
 *                     below 256 MB; the vectors are not kept), rebuilds the lists of ALL rows by a stable counting sort (each
 *                     list holds its rows ascending) and copies all codes into list order: O(ntotal) per call, so add in large
 *                     pieces.  Codes, lists and the list-major copy are committed together, or nothing is.
 *   filter            a row filter on the handle, with the mask, null and combine rules of lb_gpu_ivf_set_filter / _filter_*: a
 *                     row is visible iff its mask byte is non-zero; a NULL mask clears the filter; n != ntotal is
 *                     LB_ERR_INVALID_ARG with a last_error text and leaves the filter as it was; a predicate's nulls never match;
 *                     combine 0 replaces the mask, 1 ANDs into it and replaces when there is none; op outside 0..5 or a negative
 *                     validity_offset is LB_ERR_INVALID_ARG.  The probes of a query do not change: a probed list with no visible
 *                     row contributes nothing and no other list takes its place.  The result is the first k rows in ascending
 *                     (distance, r) order among the VISIBLE rows whose list is a probe, with the same labels, padding and
 *                     distances, bit for bit; nprobe >= nlist gives lb_gpu_pq_search over the same codes under the same mask
 *                     (lb_gpu_pq_set_filter).  Rows added after a filter was set are visible; such an add commits the codes, the
 *                     lists, the list-major copy, the mask bytes and the visible lists together or not at all.  list_sizes,
 *                     assignments, get_codes, get_centroids and ntotal ignore the filter; nvisible is the number of rows a search
 *                     can see (ntotal without a filter).  Any filter, an all-visible one too, searches the visible lists (of each
 *                     list the positions of its visible rows in the list-major copy, ascending, built on the device by every
 *                     filter call and every add under a filter: a list's reads stay inside its run of codes), so the cost follows
 *                     the visible rows of the probed lists, and last_search_stats counts those.
 *   memory            the codes are held in insertion order (what get_codes returns) and, beside each of the two pairs of lists
 *                     an add alternates between, once more in list order, so that a probed list is one contiguous run of
 *                     size * M bytes: 3 * M bytes a row, plus 12 bytes a row of lists and 8 of ids; from the first filter on 13
 *                     more (the mask byte, the filter's own list, two visible lists).  hbm_bytes reports it.
 *   limits            nlist in 1..65536, k in 1..LB_MAX_K, fewer than 2^31 rows: LB_ERR_UNSUPPORTED beyond.  nprobe <= 0 is
 *                     LB_ERR_INVALID_ARG, nprobe > nlist is clamped.  Fewer than all lists are at most LB_MAX_K probes (the
 *                     coarse search's k; LB_ERR_UNSUPPORTED beyond); every list probed needs no coarse search and works for any
 *                     nlist.
 * Argument checks answer before a device is touched, LB_ERR_INVALID_ARG before LB_ERR_UNSUPPORTED before LB_ERR_NO_DEVICE, and a
 * refused call writes nothing.  Searches and reads share the handle; adds, reserve and the filter calls take it alone.  ctx
 * (nullable) is polled before every launch.  Host pointers are borrowed for the call; d_ pointers are device memory.  Not here:
 * a filter given per search call as predicates (filter_int64 / _float32; as a row bitmap it is here:
 * lb_gpu_ivfpq_search_bitmap_ctx below), adding ready-made codes with caller-given lists, search combining, lb_gpu_comm_*, removing
 * rows, Save / Load, and the Go and C++ mirrors.
 *
 * Residual codes.  lb_gpu_ivfpq_new_residual makes a RESIDUAL handle: its arguments, limits, order of checks and status codes
 * are exactly lb_gpu_ivfpq_new's, lb_gpu_ivfpq_residual answers 1 for it (0 for a plain handle, 0 for no handle), and every
 * lb_gpu_ivfpq_* call, the lists, probes, ids, padding, stats, filters and LB_MAX_K are as above.  Three definitions differ:
 *   res(v, l)         res(v, l)[i] = v[i] - C[l][i]: one IEEE f32 subtraction a component, stored rounded to f32, contracted with
 *                     nothing after it.
 *   code of a row     lb_gpu_pq_encode(res(x, list(x))), list(x) being the same k = 1 coarse search; the vector is dropped after
 *                     the add, as on a plain handle.  The codebooks are meant to be trained on such residuals.
 *   distance          of query q to a row r of probed list l: float32(sqrt(float64(sum_j table_l[j * 256 + code_r[j]]))) with
 *                     table_l = BuildADCTable(res(q, l)): lb_gpu_pq_search's arithmetic over a table per probed list.  The result
 *                     is the first k rows in ascending (distance, r) order among the rows, under a filter the visible rows, of
 *                     the probed lists.  Given the codes and the probed lists nothing is approximate.
 * Consequences: get_codes returns residual codes; "nprobe >= nlist gives lb_gpu_pq_search over the same codes" does NOT hold for
 * a residual handle; it does hold, bit for bit, that a residual handle whose rows all fall in a list with an all-zero centroid
 * equals the plain handle over the same input (x - 0 = x).
 *   memory            a residual handle keeps the centroids once more, as a device f32 [nlist][dims] array of its own (the coarse
 *                     index keeps its rows to itself); hbm_bytes counts it.
 *   scratch           a search holds one table (M * 1024 bytes) per pair (query, probed list) of a batch.  The tables of a batch
 *                     are bounded by 1 GiB: a batch is at most nb queries with nb * np * M * 1024 <= 2^30 (np = min(nprobe,
 *                     nlist); at M = 96 room for 10,922 tables).  Only when ONE query's np tables exceed 1 GiB (at M = 159 from
 *                     6,595 probes) its probed lists are scanned in rounds of as many as fit, all into the query's one run of
 *                     keys, and the selection runs once.  Neither changes a result.
 *   last_timing       ms[2] is the residual queries and their tables, ms[3] the scan; when a query's tables go in several
 *                     rounds, the rounds after the first are whole in ms[3]. */
typedef struct lb_gpu_ivfpq lb_gpu_ivfpq;
lb_gpu_ivfpq *lb_gpu_ivfpq_new(int device, const uint8_t *codebook_blob, size_t len, int order, int nlist, const float *centroids,
                               int *out_status);
lb_gpu_ivfpq *lb_gpu_ivfpq_new_residual(int device, const uint8_t *codebook_blob, size_t len, int order, int nlist,
                                        const float *centroids, int *out_status);
int lb_gpu_ivfpq_residual(const lb_gpu_ivfpq *p); /* 1: residual codes; 0: plain, or no handle */
void lb_gpu_ivfpq_free(lb_gpu_ivfpq *p);
const char *lb_gpu_ivfpq_last_error(const lb_gpu_ivfpq *p);
int lb_gpu_ivfpq_dims(const lb_gpu_ivfpq *p);
int lb_gpu_ivfpq_m(const lb_gpu_ivfpq *p);
int lb_gpu_ivfpq_order(const lb_gpu_ivfpq *p);
int lb_gpu_ivfpq_nlist(const lb_gpu_ivfpq *p);
int64_t lb_gpu_ivfpq_ntotal(const lb_gpu_ivfpq *p);
int64_t lb_gpu_ivfpq_hbm_bytes(const lb_gpu_ivfpq *p); /* codes (three times), ids, lists, codebooks, the coarse index, what a
                                                          row filter holds and a residual handle's copy of the centroids */
int lb_gpu_ivfpq_get_centroids(lb_gpu_ivfpq *p, float *out); /* f32[nlist*dims] */
int lb_gpu_ivfpq_reserve(lb_gpu_ivfpq *p, int64_t n_total);
int lb_gpu_ivfpq_add(lb_gpu_ivfpq *p, int64_t n, const float *vectors, const int64_t *ids); /* assign, encode, append */
int lb_gpu_ivfpq_add_device(lb_gpu_ivfpq *p, int64_t n, const float *d_vectors, const int64_t *d_ids);
int lb_gpu_ivfpq_get_codes(lb_gpu_ivfpq *p, int64_t row0, int64_t n, uint8_t *codes); /* u8[n*M], insertion order */
int lb_gpu_ivfpq_list_sizes(lb_gpu_ivfpq *p, int64_t *sizes); /* [nlist] */
int lb_gpu_ivfpq_assignments(lb_gpu_ivfpq *p, int64_t row0, int64_t n, int32_t *lists); /* the lists of rows [row0, row0 + n) */
int lb_gpu_ivfpq_search(lb_gpu_ivfpq *p, int64_t nq, const float *queries, int k, int nprobe, float *dist, int64_t *labels);
int lb_gpu_ivfpq_search_ctx(lb_gpu_ivfpq *p, int64_t nq, const float *queries, int k, int nprobe, float *dist, int64_t *labels,
                            const lb_cancel *ctx);
int lb_gpu_ivfpq_search_device_ctx(lb_gpu_ivfpq *p, int64_t nq, const float *d_queries, int k, int nprobe, float *d_dist,
                                   int64_t *d_labels, void *stream, const lb_cancel *ctx);
/* Call bitmap: the same searches under a row filter of THIS CALL alone, on a plain and on a residual handle alike.  The statement
 * is lb_gpu_ivf_search_bitmap_ctx's ("call bitmap" above lb_gpu_ivf_new), word for word where it applies: they take what their
 * plain counterparts take, and behind nprobe (bitmap, nbits, stride_bytes).  One bit per row POSITION, as the handle filter's mask
 * is by position, least significant bit first as in an Arrow validity buffer: row r is visible to the call iff
 * bitmap[r >> 3] >> (r & 7) & 1.  It is read byte by byte: no alignment is owed and no padding beyond ceil(nbits / 8) bytes, and
 * nothing past bit nbits - 1 is read as a row.  stride_bytes 0: one bitmap serves every query of the call; otherwise query q reads
 * bitmap + q * stride_bytes, and stride_bytes >= ceil(nbits / 8).  The result is the handle's exact k-NN (ADC on a plain handle,
 * ADC under the table of each probed list on a residual one) among the rows of the probed lists that are live, pass the handle's
 * filter if one is set AND have their bit set; order, labels (the ids where an add gave them), padding and distances as stated
 * above.  It is bit for bit what the same handle answers after set_filter (combined with its own filter) with the mask
 * bit(r) != 0, and last_search_stats agrees in all four values.  The probes do not change, and on a residual handle the table of a
 * probed list is that of the list probed, whatever the bitmap hides.  The handle is not changed and is held shared, like any
 * search: calls with different bitmaps run concurrently, and nvisible, the handle's filter and every later call are untouched.  A
 * NULL bitmap is the plain search through the plain path with no launch added, and so is an empty handle; nbits and stride_bytes
 * are then ignored.  A non-NULL bitmap with nbits != ntotal (the n != ntotal rule of set_filter), nbits < 0, a negative stride or
 * a stride in (0, ceil(nbits / 8)) is LB_ERR_INVALID_ARG with the numbers in last_error, answered under the reader lock before any
 * launch and with nothing written; the plain entry points' checks and their order come first.  A NULL handle is
 * LB_ERR_INVALID_ARG before a device is touched.  On the device the probed lists are compacted under the bitmap into lists of the
 * call's own, which hold POSITIONS into the list-major codes (over the handle's visible lists when it has a filter or removed
 * rows: the bit is then looked up by the row at that position), and the plan, the scan and the selection walk those.  Under one
 * bitmap (stride 0), when the call's queries times their largest probed lists exceed the handle's rows, every list is compacted
 * once for the call and not once per query and probe; the result does not depend on which form ran.  ctx is polled before these
 * launches as before every other; under profiling they fall into ms[1], in the second form into the first batch's. */
int lb_gpu_ivfpq_search_bitmap_ctx(lb_gpu_ivfpq *p, int64_t nq, const float *queries, int k, int nprobe, const uint8_t *bitmap,
                                   int64_t nbits, int64_t stride_bytes, float *dist, int64_t *labels, const lb_cancel *ctx);
int lb_gpu_ivfpq_search_bitmap_device_ctx(lb_gpu_ivfpq *p, int64_t nq, const float *d_queries, int k, int nprobe, const uint8_t *d_bitmap,
                                          int64_t nbits, int64_t stride_bytes, float *d_dist, int64_t *d_labels, void *stream,
                                          const lb_cancel *ctx);
/* the row filter, as lb_gpu_ivf_set_filter / _filter_int64 / _filter_float32 / _nvisible */
int lb_gpu_ivfpq_set_filter(lb_gpu_ivfpq *p, const uint8_t *mask, int64_t n);
int lb_gpu_ivfpq_filter_int64(lb_gpu_ivfpq *p, const int64_t *column, int64_t n, int64_t value, int op, const uint8_t *validity,
                              int64_t validity_offset, int combine);
int lb_gpu_ivfpq_filter_float32(lb_gpu_ivfpq *p, const float *column, int64_t n, float value, int op, const uint8_t *validity,
                                int64_t validity_offset, int combine);
int64_t lb_gpu_ivfpq_nvisible(const lb_gpu_ivfpq *p);
/* telemetry of the last search only, as lb_gpu_ivf_last_search_stats: out[0] queries, out[1] rows scanned summed over the
 * queries, out[2] the largest per-query count, out[3] queries whose selection ran from LDS; under a row filter the rows are the
 * visible ones of the probed lists */
int lb_gpu_ivfpq_last_search_stats(lb_gpu_ivfpq *p, int64_t out[4]);
/* instrumentation (tools/ivfpq_bench.py), as lb_gpu_ivf_set_profiling: ms[0] the probes (the coarse search), ms[1] the plan,
 * ms[2] the ADC tables, ms[3] the scan of the probed lists' codes, ms[4] the selection; summed over the search's batches */
int lb_gpu_ivfpq_set_profiling(lb_gpu_ivfpq *p, int enable);
int lb_gpu_ivfpq_last_timing(lb_gpu_ivfpq *p, float ms[5]);
/* as lb_gpu_ivf_last_build_timing: the last profiled build of the visible lists (tools/code_filter_bench.py --index ivfpq) */
int lb_gpu_ivfpq_last_build_timing(lb_gpu_ivfpq *p, float *ms);

/* Removal and compaction: the statement above lb_gpu_ivf_remove and lb_gpu_ivf_compact holds word for word, "rows" being the
 * handle's codes; plain and residual handles alike.  What differs:
 *   searches     every lb_gpu_ivfpq_search* entry point answers the exact ADC k-NN (on a residual handle under the table of each
 *                probed list) among the rows of the probed lists that are live AND pass the filter: bit for bit what a fresh
 *                handle with the same codebooks and centroids answers when it holds only the survivors' codes, in their order,
 *                with ids = the old labels.  With every list probed a plain handle equals lb_gpu_pq_search over the surviving
 *                codes.  last_search_stats counts live, visible rows only.
 *   codes        are kept, never recomputed: a removed row keeps its position, its list and its M code bytes until compaction, and
 *                get_codes, list_sizes, assignments and ntotal keep counting it.  Compaction moves codes, ids, assignments and a
 *                surviving filter's bytes together and then writes the list-major copy from the moved codes and the new lists; no
 *                row is assigned or encoded again.  A residual code is of the row less ITS list's centroid, and the list moves
 *                with the row, so it stays the code lb_gpu_ivfpq_add of the survivor's vector would produce.  Afterwards
 *                get_codes equals the old codes taken at old_rows. */
int lb_gpu_ivfpq_remove(lb_gpu_ivfpq *p, int64_t n, const int64_t *labels, int64_t *n_removed);
int lb_gpu_ivfpq_remove_device(lb_gpu_ivfpq *p, int64_t n, const int64_t *d_labels, int64_t *n_removed);
int lb_gpu_ivfpq_remove_rows(lb_gpu_ivfpq *p, int64_t n, const int64_t *rows, int64_t *n_removed);
int64_t lb_gpu_ivfpq_nlive(const lb_gpu_ivfpq *p);
int64_t lb_gpu_ivfpq_ndeleted(const lb_gpu_ivfpq *p);
int lb_gpu_ivfpq_compact(lb_gpu_ivfpq *p, int64_t *old_rows, int64_t cap);

/* ---- IVF-SQ8: exact integer k-NN over the codes of the probed lists ----------------------------
 * The coarse partition of lb_gpu_ivf_* over the codes of lb_gpu_sq8_* (FAISS's "IVF...,SQ8"): a query skips most rows, and a row
 * costs dims bytes instead of 4 * dims.  Nothing is approximate beyond the SQ8 codes themselves and WHICH lists are probed: given
 * the codes and the probed lists the result is the exact k-NN among their rows by the integer distance, bit for bit.
 * A handle has dims, SQ8 bounds min and max (f32 [dims] each, given by the caller and fixed at creation), an accumulation order for
 * the coarse quantiser (0 SEQ, 1 UNROLL4, as lb_gpu_index_set_order; fixed at creation because it decides which list a row goes
 * to), nlist centroids C (f32 [nlist][dims], given by the caller) and rows in insertion order, of which only the codes are kept.
 * The coarse metric is L2 (metric 0) and the handle takes no metric argument.
 *   code of a row     lb_gpu_sq8_encode of the row under the handle's bounds: EncodeInto's arithmetic (scalar_quantization.go:
 *                     155-170), scale and invScale by f32 division as NewSQ8Encoder (:75-79).
 *   list of a row     as on the IVF-Flat and IVF-PQ handles: the label of the k = 1 L2 search of the f32 row, as a query, over an
 *                     f32 index that holds C, in the handle's order.  Computed from the vector when the row is added, before the
 *                     vector is dropped; it never changes.
 *   probes of a query the labels of the k = min(nprobe, nlist) search of the f32 query over that same index.
 *   distance          S = sum_i (a_i - b_i)^2 as int32 (simd.EuclideanSQ8Generic), a the code of the query (the query is encoded on
 *                     the device first, as lb_gpu_sq8_search does; a NaN component gives code 0 as there), b the row's code.
 *   result            the first k rows r in ascending (S, r) order OF THE INTEGERS among the rows whose list is a probe of q; the
 *                     reported distance is float32(S); the label is ids[r] when ids were given, else r; with fewer than k such
 *                     rows they come first, then label -1 / distance FLT_MAX.  Two different S above 2^24 can round to one float:
 *                     the row with the larger S still comes second, whatever its position.  nprobe >= nlist gives
 *                     lb_gpu_sq8_search over the same codes, bit for bit: labels, order and distances.
 *   bounds            min[i] >= max[i] in any dimension is LB_ERR_INVALID_ARG (SQ8Config.Validate: "min must be less than max
 *                     for all dimensions"; no handle exists to hold the text, the status is the answer).  NaN bounds pass, as on
 *                     lb_gpu_sq8_set_bounds.
 *   ids               given on every add or on none; a call that breaks this is LB_ERR_INVALID_ARG and adds nothing.
 *   add               assigns and encodes the vectors (in pieces of at most 64 Mi floats, so the staging of host vectors stays
 *                     below 256 MB; the vectors are not kept) and rebuilds the lists of ALL rows by a stable counting sort (each
 *                     list holds its rows ascending): O(ntotal) per call, so add in large pieces.  Codes and lists are committed
 *                     together, or nothing is.
 *   filter            a row filter on the handle, with the mask, null and combine rules of lb_gpu_ivf_set_filter / _filter_*: a
 *                     row is visible iff its mask byte is non-zero; a NULL mask clears the filter; n != ntotal is
 *                     LB_ERR_INVALID_ARG with a last_error text and leaves the filter as it was; a predicate's nulls never match;
 *                     combine 0 replaces the mask, 1 ANDs into it and replaces when there is none; op outside 0..5 or a negative
 *                     validity_offset is LB_ERR_INVALID_ARG.  The probes of a query do not change: a probed list with no visible
 *                     row contributes nothing and no other list takes its place.  The result is the first k rows in ascending
 *                     (S, r) order among the VISIBLE rows whose list is a probe, with the same labels, padding and distances, bit
 *                     for bit; nprobe >= nlist gives lb_gpu_sq8_search over the same codes under the same mask
 *                     (lb_gpu_sq8_set_filter).  Rows added after a filter was set are visible; such an add commits the codes, the
 *                     lists, the mask bytes and the visible lists together or not at all.  list_sizes, assignments, get_codes,
 *                     get_centroids, get_bounds and ntotal ignore the filter; nvisible is the number of rows a search can see
 *                     (ntotal without a filter).  Any filter, an all-visible one too, searches the visible lists (each list's
 *                     visible rows, ascending, built on the device by every filter call and every add under a filter), so the
 *                     cost follows the visible rows of the probed lists, and last_search_stats counts those.
 *   memory            the codes are held once, in insertion order at a stride of dims rounded up to 16 bytes (pad bytes zero; what
 *                     get_codes returns without the pads), plus 12 bytes a row of lists and 8 of ids; from the first filter on
 *                     13 more (the mask byte, the filter's own list, two visible lists).  hbm_bytes reports it.
 *   limits            dims in 1..LB_MAX_DIM, nlist in 1..65536, k in 1..LB_MAX_K, fewer than 2^31 rows: LB_ERR_UNSUPPORTED
 *                     beyond.  nprobe <= 0 is LB_ERR_INVALID_ARG, nprobe > nlist is clamped.  Fewer than all lists are at most
 *                     LB_MAX_K probes (the coarse search's k; LB_ERR_UNSUPPORTED beyond); every list probed needs no coarse
 *                     search and works for any nlist.
 * lb_gpu_ivfsq8_new checks dims <= 0, NULL min / max / centroids, order outside 0..1, nlist <= 0 and the bounds
 * (LB_ERR_INVALID_ARG), then dims > LB_MAX_DIM and nlist > 65536 (LB_ERR_UNSUPPORTED), then the device (LB_ERR_NO_DEVICE).
 * Argument checks answer before a device is touched, LB_ERR_INVALID_ARG before LB_ERR_UNSUPPORTED before LB_ERR_NO_DEVICE, and a
 * refused call writes nothing.  Searches and reads share the handle; adds, reserve and the filter calls take it alone.  ctx
 * (nullable) is polled before every launch.  Host pointers are borrowed for the call; d_ pointers are device memory.  Not here:
 * adding ready-made codes, a list-major copy of the codes, a multi-query tile that shares a list's rows between the queries
 * that probe it, the i8 matrix-core pass, residual SQ8, SQ8EuclideanDistance as a reported distance, search combining,
 * lb_gpu_comm_*, removing rows, Save / Load, and the Go and C++ mirrors. */
typedef struct lb_gpu_ivfsq8 lb_gpu_ivfsq8;
lb_gpu_ivfsq8 *lb_gpu_ivfsq8_new(int device, int dims, const float *min, const float *max, int order, int nlist, const float *centroids,
                                 int *out_status);
void lb_gpu_ivfsq8_free(lb_gpu_ivfsq8 *p);
const char *lb_gpu_ivfsq8_last_error(const lb_gpu_ivfsq8 *p);
int lb_gpu_ivfsq8_dims(const lb_gpu_ivfsq8 *p);
int lb_gpu_ivfsq8_order(const lb_gpu_ivfsq8 *p);
int lb_gpu_ivfsq8_nlist(const lb_gpu_ivfsq8 *p);
int64_t lb_gpu_ivfsq8_ntotal(const lb_gpu_ivfsq8 *p);
int64_t lb_gpu_ivfsq8_hbm_bytes(const lb_gpu_ivfsq8 *p); /* codes, ids, lists, bounds, the coarse index and what a row filter holds */
int lb_gpu_ivfsq8_get_bounds(lb_gpu_ivfsq8 *p, float *min, float *max); /* f32[dims] each */
int lb_gpu_ivfsq8_get_centroids(lb_gpu_ivfsq8 *p, float *out); /* f32[nlist*dims] */
int lb_gpu_ivfsq8_reserve(lb_gpu_ivfsq8 *p, int64_t n_total);
int lb_gpu_ivfsq8_add(lb_gpu_ivfsq8 *p, int64_t n, const float *vectors, const int64_t *ids); /* assign, encode, append */
int lb_gpu_ivfsq8_add_device(lb_gpu_ivfsq8 *p, int64_t n, const float *d_vectors, const int64_t *d_ids);
int lb_gpu_ivfsq8_get_codes(lb_gpu_ivfsq8 *p, int64_t row0, int64_t n, uint8_t *codes); /* u8[n*dims], insertion order, pads stripped */
int lb_gpu_ivfsq8_list_sizes(lb_gpu_ivfsq8 *p, int64_t *sizes); /* [nlist] */
int lb_gpu_ivfsq8_assignments(lb_gpu_ivfsq8 *p, int64_t row0, int64_t n, int32_t *lists); /* the lists of rows [row0, row0 + n) */
int lb_gpu_ivfsq8_search(lb_gpu_ivfsq8 *p, int64_t nq, const float *queries, int k, int nprobe, float *dist, int64_t *labels);
int lb_gpu_ivfsq8_search_ctx(lb_gpu_ivfsq8 *p, int64_t nq, const float *queries, int k, int nprobe, float *dist, int64_t *labels,
                             const lb_cancel *ctx);
int lb_gpu_ivfsq8_search_device_ctx(lb_gpu_ivfsq8 *p, int64_t nq, const float *d_queries, int k, int nprobe, float *d_dist,
                                    int64_t *d_labels, void *stream, const lb_cancel *ctx);
/* Call bitmap: the same searches under a row filter of THIS CALL alone.  The statement is lb_gpu_ivf_search_bitmap_ctx's ("call
 * bitmap" above lb_gpu_ivf_new) and lb_gpu_ivfpq_search_bitmap_ctx's, word for word where it applies: (bitmap, nbits,
 * stride_bytes) behind nprobe, one bit per row POSITION, least significant bit first, read byte by byte at any address;
 * stride_bytes 0 is one bitmap for every query, otherwise query q reads bitmap + q * stride_bytes and stride_bytes >=
 * ceil(nbits / 8).  The result is the exact integer k-NN (ascending keys (S << 32) | row, reported as float32(S)) among the rows
 * of the probed lists that are live, pass the handle's filter if one is set AND have their bit set, bit for bit what the same
 * handle answers after set_filter (combined with its own filter) with the mask bit(r) != 0, labels (ids), distances and all four
 * last_search_stats included.  The handle is not changed and is held shared: calls with different bitmaps run concurrently.  A
 * NULL bitmap is the plain search with no launch added, and so is an empty handle.  nbits != ntotal, nbits < 0, a negative stride
 * or a stride in (0, ceil(nbits / 8)) is LB_ERR_INVALID_ARG with the numbers in last_error, under the reader lock, before any
 * launch, nothing written, behind the plain entry points' own checks; a NULL handle is LB_ERR_INVALID_ARG before a device is
 * touched.  The lists of this handle hold rows and its scan gathers by row, so the compaction is the IVF-Flat handle's, in either
 * of its two forms (per probe slot, or every list once under one bitmap); under profiling it falls into ms[1]. */
int lb_gpu_ivfsq8_search_bitmap_ctx(lb_gpu_ivfsq8 *p, int64_t nq, const float *queries, int k, int nprobe, const uint8_t *bitmap,
                                    int64_t nbits, int64_t stride_bytes, float *dist, int64_t *labels, const lb_cancel *ctx);
int lb_gpu_ivfsq8_search_bitmap_device_ctx(lb_gpu_ivfsq8 *p, int64_t nq, const float *d_queries, int k, int nprobe, const uint8_t *d_bitmap,
                                           int64_t nbits, int64_t stride_bytes, float *d_dist, int64_t *d_labels, void *stream,
                                           const lb_cancel *ctx);
/* the row filter, as lb_gpu_ivf_set_filter / _filter_int64 / _filter_float32 / _nvisible */
int lb_gpu_ivfsq8_set_filter(lb_gpu_ivfsq8 *p, const uint8_t *mask, int64_t n);
int lb_gpu_ivfsq8_filter_int64(lb_gpu_ivfsq8 *p, const int64_t *column, int64_t n, int64_t value, int op, const uint8_t *validity,
                               int64_t validity_offset, int combine);
int lb_gpu_ivfsq8_filter_float32(lb_gpu_ivfsq8 *p, const float *column, int64_t n, float value, int op, const uint8_t *validity,
                                 int64_t validity_offset, int combine);
int64_t lb_gpu_ivfsq8_nvisible(const lb_gpu_ivfsq8 *p);
/* telemetry of the last search only, as lb_gpu_ivf_last_search_stats: out[0] queries, out[1] rows scanned summed over the
 * queries, out[2] the largest per-query count, out[3] queries whose selection ran from LDS; under a row filter the rows are the
 * visible ones of the probed lists */
int lb_gpu_ivfsq8_last_search_stats(lb_gpu_ivfsq8 *p, int64_t out[4]);
/* instrumentation (tools/ivfsq8_bench.py), as lb_gpu_ivf_set_profiling: ms[0] the probes (the coarse search), ms[1] the plan,
 * ms[2] the queries' codes and their norms, ms[3] the scan of the probed lists' rows, ms[4] the selection; summed over the
 * search's batches */
int lb_gpu_ivfsq8_set_profiling(lb_gpu_ivfsq8 *p, int enable);
int lb_gpu_ivfsq8_last_timing(lb_gpu_ivfsq8 *p, float ms[5]);
/* as lb_gpu_ivf_last_build_timing: the last profiled build of the visible lists */
int lb_gpu_ivfsq8_last_build_timing(lb_gpu_ivfsq8 *p, float *ms);

/* Removal and compaction: the statement above lb_gpu_ivf_remove and lb_gpu_ivf_compact holds word for word, "rows" being the
 * handle's codes.  What differs:
 *   searches     every lb_gpu_ivfsq8_search* entry point answers the exact k-NN under the integer S among the rows of the probed
 *                lists that are live AND pass the filter: bit for bit what a fresh handle with the same bounds and centroids
 *                answers when it holds only the survivors' codes, in their order, with ids = the old labels.  With every list
 *                probed it equals lb_gpu_sq8_search over the surviving codes.  last_search_stats counts live, visible rows only.
 *   codes        are kept, never recomputed: a removed row keeps its position, its list and its dims code bytes until compaction,
 *                and get_codes, list_sizes, assignments and ntotal keep counting it.  Compaction moves codes, ids, assignments
 *                and a surviving filter's bytes together; no row is assigned or encoded again.  Afterwards get_codes equals the
 *                old codes taken at old_rows. */
int lb_gpu_ivfsq8_remove(lb_gpu_ivfsq8 *p, int64_t n, const int64_t *labels, int64_t *n_removed);
int lb_gpu_ivfsq8_remove_device(lb_gpu_ivfsq8 *p, int64_t n, const int64_t *d_labels, int64_t *n_removed);
int lb_gpu_ivfsq8_remove_rows(lb_gpu_ivfsq8 *p, int64_t n, const int64_t *rows, int64_t *n_removed);
int64_t lb_gpu_ivfsq8_nlive(const lb_gpu_ivfsq8 *p);
int64_t lb_gpu_ivfsq8_ndeleted(const lb_gpu_ivfsq8 *p);
int lb_gpu_ivfsq8_compact(lb_gpu_ivfsq8 *p, int64_t *old_rows, int64_t cap);

/* ---- IVF-BQ: exact Hamming k-NN over the codes of the probed lists -----------------------------
 * The coarse partition of lb_gpu_ivf_* over the sign-bit codes of lb_gpu_bq_*: a query skips most rows, and a row costs
 * 8 * ceil(dims / 64) bytes instead of 4 * dims.  Nothing is approximate beyond the codes themselves and WHICH lists are probed:
 * given the codes and the probed lists the result is the exact k-NN among their rows by the Hamming distance, bit for bit.
 * A handle has dims, an accumulation order for the coarse quantiser (0 SEQ, 1 UNROLL4, as lb_gpu_index_set_order; fixed at
 * creation because it decides which list a row goes to), nlist centroids C (f32 [nlist][dims], given by the caller) and rows in
 * insertion order, of which only the codes are kept.  The coarse metric is L2 (metric 0) and the handle takes no metric argument.
 *   code of a row     lb_gpu_bq_encode of the row: W = (dims + 63) / 64 little-endian words, bit i % 64 of word i / 64 set iff
 *                     v[i] > 0, compared on the bit pattern (binary_quantization.go:34-45); pad bits are zero.  Only vectors are
 *                     added, so a stored code never has a pad bit set.
 *   list of a row     as on the other IVF handles: the label of the k = 1 L2 search of the f32 row, as a query, over an f32 index
 *                     that holds C, in the handle's order.  Computed from the vector when the row is added, before the vector is
 *                     dropped; it never changes.
 *   probes of a query the labels of the k = min(nprobe, nlist) search of the f32 query over that same index.
 *   distance          h = sum_w popcount(a[w] ^ b[w]) over all W words as int32 (simd.HammingDistance), a the code of the f32 query
 *                     (encoded on the device per batch, as lb_gpu_bq_search does; a NaN component gives bit 0), b the row's code.
 *   result            the first k rows r in ascending (h, r) order among the rows whose list is a probe of q; the reported
 *                     distance is float32(h), exact because h <= 8192; the label is ids[r] when ids were given, else r; with fewer
 *                     than k such rows they come first, then label -1 / distance FLT_MAX.  nprobe >= nlist gives lb_gpu_bq_search
 *                     over the same codes, bit for bit: labels, order and distances.
 *   ids               given on every add or on none; a call that breaks this is LB_ERR_INVALID_ARG and adds nothing.
 *   add               assigns and encodes the vectors (in pieces of at most 64 Mi floats, so the staging of host vectors stays
 *                     below 256 MB; the vectors are not kept) and rebuilds the lists of ALL rows by a stable counting sort (each
 *                     list holds its rows ascending) and the list-major copy of their codes: O(ntotal) per call, so add in large
 *                     pieces.  Codes, lists and list-major codes are committed together, or nothing is.
 *   filter            a row filter on the handle, with the mask, null and combine rules of lb_gpu_ivf_set_filter / _filter_*: a
 *                     row is visible iff its mask byte is non-zero; a NULL mask clears the filter; n != ntotal is
 *                     LB_ERR_INVALID_ARG with a last_error text and leaves the filter as it was; a predicate's nulls never match;
 *                     combine 0 replaces the mask, 1 ANDs into it and replaces when there is none; op outside 0..5 or a negative
 *                     validity_offset is LB_ERR_INVALID_ARG.  The probes of a query do not change: a probed list with no visible
 *                     row contributes nothing and no other list takes its place.  The result is the first k rows in ascending
 *                     (h, r) order among the VISIBLE rows whose list is a probe, with the same labels, padding and distances, bit
 *                     for bit; nprobe >= nlist gives lb_gpu_bq_search over the same codes under the same mask
 *                     (lb_gpu_bq_set_filter).  Rows added after a filter was set are visible; such an add commits the codes, the
 *                     lists, the list-major codes, the mask bytes and the visible lists together or not at all.  list_sizes,
 *                     assignments, get_codes, get_centroids and ntotal ignore the filter; nvisible is the number of rows a search
 *                     can see (ntotal without a filter).  Any filter, an all-visible one too, searches the visible lists (each
 *                     list's visible entries as positions into the lists of all rows, ascending, built on the device by every
 *                     filter call and every add under a filter), so the cost follows the visible rows of the probed lists, and
 *                     last_search_stats counts those.
 *   memory            the codes are held three times: once in insertion order (what get_codes returns, and what every add
 *                     permutes from) and list-major once for each of the two list pairs an add alternates between, so a probed
 *                     list is one contiguous run.  A row costs 24 * W + 12 bytes (codes and lists), 8 more with ids, and from the
 *                     first filter on 13 more (the mask byte, the filter's own list, two visible lists).  hbm_bytes reports it.
 *   limits            dims in 1..LB_MAX_DIM, nlist in 1..65536, k in 1..LB_MAX_K, fewer than 2^31 rows: LB_ERR_UNSUPPORTED
 *                     beyond.  nprobe <= 0 is LB_ERR_INVALID_ARG, nprobe > nlist is clamped.  Fewer than all lists are at most
 *                     LB_MAX_K probes (the coarse search's k; LB_ERR_UNSUPPORTED beyond); every list probed needs no coarse
 *                     search and works for any nlist.
 * lb_gpu_ivfbq_new checks dims <= 0, NULL centroids, order outside 0..1 and nlist <= 0 (LB_ERR_INVALID_ARG), then
 * dims > LB_MAX_DIM and nlist > 65536 (LB_ERR_UNSUPPORTED), then the device (LB_ERR_NO_DEVICE).
 * Argument checks answer before a device is touched, LB_ERR_INVALID_ARG before LB_ERR_UNSUPPORTED before LB_ERR_NO_DEVICE, and a
 * refused call writes nothing.  Searches and reads share the handle; adds, reserve and the filter calls take it alone.  ctx
 * (nullable) is polled before every launch.  Host pointers are borrowed for the call; d_ pointers are device memory.  Not here:
 * adding ready-made codes (a list needs the vector), a multi-query tile that shares a list's rows between the queries that probe
 * it, a counting selection over the at most 8,193 distinct distances, search combining, lb_gpu_comm_*, removing rows,
 * Save / Load, and the Go and C++ mirrors. */
typedef struct lb_gpu_ivfbq lb_gpu_ivfbq;
lb_gpu_ivfbq *lb_gpu_ivfbq_new(int device, int dims, int order, int nlist, const float *centroids, int *out_status);
void lb_gpu_ivfbq_free(lb_gpu_ivfbq *p);
const char *lb_gpu_ivfbq_last_error(const lb_gpu_ivfbq *p);
int lb_gpu_ivfbq_dims(const lb_gpu_ivfbq *p);
int lb_gpu_ivfbq_words(const lb_gpu_ivfbq *p); /* W = (dims + 63) / 64 */
int lb_gpu_ivfbq_order(const lb_gpu_ivfbq *p);
int lb_gpu_ivfbq_nlist(const lb_gpu_ivfbq *p);
int64_t lb_gpu_ivfbq_ntotal(const lb_gpu_ivfbq *p);
int64_t lb_gpu_ivfbq_hbm_bytes(const lb_gpu_ivfbq *p); /* codes three times, ids, lists, the coarse index and what a row filter holds */
int lb_gpu_ivfbq_get_centroids(lb_gpu_ivfbq *p, float *out); /* f32[nlist*dims] */
int lb_gpu_ivfbq_reserve(lb_gpu_ivfbq *p, int64_t n_total);
int lb_gpu_ivfbq_add(lb_gpu_ivfbq *p, int64_t n, const float *vectors, const int64_t *ids); /* assign, encode, append */
int lb_gpu_ivfbq_add_device(lb_gpu_ivfbq *p, int64_t n, const float *d_vectors, const int64_t *d_ids);
int lb_gpu_ivfbq_get_codes(lb_gpu_ivfbq *p, int64_t row0, int64_t n, uint64_t *codes); /* u64[n*W], insertion order */
int lb_gpu_ivfbq_list_sizes(lb_gpu_ivfbq *p, int64_t *sizes); /* [nlist] */
int lb_gpu_ivfbq_assignments(lb_gpu_ivfbq *p, int64_t row0, int64_t n, int32_t *lists); /* the lists of rows [row0, row0 + n) */
int lb_gpu_ivfbq_search(lb_gpu_ivfbq *p, int64_t nq, const float *queries, int k, int nprobe, float *dist, int64_t *labels);
int lb_gpu_ivfbq_search_ctx(lb_gpu_ivfbq *p, int64_t nq, const float *queries, int k, int nprobe, float *dist, int64_t *labels,
                            const lb_cancel *ctx);
int lb_gpu_ivfbq_search_device_ctx(lb_gpu_ivfbq *p, int64_t nq, const float *d_queries, int k, int nprobe, float *d_dist,
                                   int64_t *d_labels, void *stream, const lb_cancel *ctx);
/* the row filter, as lb_gpu_ivf_set_filter / _filter_int64 / _filter_float32 / _nvisible */
int lb_gpu_ivfbq_set_filter(lb_gpu_ivfbq *p, const uint8_t *mask, int64_t n);
int lb_gpu_ivfbq_filter_int64(lb_gpu_ivfbq *p, const int64_t *column, int64_t n, int64_t value, int op, const uint8_t *validity,
                              int64_t validity_offset, int combine);
int lb_gpu_ivfbq_filter_float32(lb_gpu_ivfbq *p, const float *column, int64_t n, float value, int op, const uint8_t *validity,
                                int64_t validity_offset, int combine);
int64_t lb_gpu_ivfbq_nvisible(const lb_gpu_ivfbq *p);
/* telemetry of the last search only, as lb_gpu_ivf_last_search_stats: out[0] queries, out[1] rows scanned summed over the
 * queries, out[2] the largest per-query count, out[3] queries whose selection ran from LDS; under a row filter the rows are the
 * visible ones of the probed lists */
int lb_gpu_ivfbq_last_search_stats(lb_gpu_ivfbq *p, int64_t out[4]);
/* instrumentation (tools/ivfbq_bench.py), as lb_gpu_ivf_set_profiling: ms[0] the probes (the coarse search), ms[1] the plan,
 * ms[2] the queries' codes, ms[3] the scan of the probed lists' codes, ms[4] the selection; summed over the search's batches */
int lb_gpu_ivfbq_set_profiling(lb_gpu_ivfbq *p, int enable);
int lb_gpu_ivfbq_last_timing(lb_gpu_ivfbq *p, float ms[5]);
/* as lb_gpu_ivf_last_build_timing: the last profiled build of the visible lists */
int lb_gpu_ivfbq_last_build_timing(lb_gpu_ivfbq *p, float *ms);

/* ---- cross-shard merge ---------------------------------------------------------
 * store.MergeSortedStreams (internal/store/result_merger.go:34-101) for S shards:
 * inputs [S][nq][k] ascending per (shard, query) (padding label -1 / FLT_MAX allowed),
 * output [nq][k] ascending by (distance, label); padding sorts last, every NaN after +inf.
 * nshards * k <= 16384 (k = 2048 on 8 GPUs).  Device pointers. */
int lb_gpu_merge_topk_device(int device, int nshards, int64_t nq, int k, const float *d_dist_in,
                             const int64_t *d_labels_in, float *d_dist_out, int64_t *d_labels_out,
                             void *stream);

/* Same merge over ONE gathered buffer (a single RCCL all-gather per batch): shard s's block starts at
 * d_packed + s*block_bytes and holds nq*k int64 labels followed by nq*k f32 distances, the block
 * size rounded up to 8 bytes: block_bytes = nq*k*8 + ceil(nq*k*4 / 8)*8. */
int lb_gpu_merge_topk_packed_device(int device, int nshards, int64_t nq, int k, const void *d_packed,
                                    float *d_dist_out, int64_t *d_labels_out, void *stream);

/* ---- multi-GPU search -------------------------------------------------------------------
 * One GPU per shard; per batch: shard search -> ONE all-gather of the packed per-shard top-k (RCCL over xGMI,
 * nq*k*12 bytes per rank) -> device merge.  Semantics of ShardedHNSW.SearchVectors' fan-out + concat + sort
 * (internal/store/sharded_hnsw.go:414-503) / MergeSortedStreams (result_merger.go:34-101); which rows a
 * shard holds is the host's business (store.RingSharder, sharding_strategy.go:40-127).  SURVEY 8(b)'s
 * lb_gpu_comm_init(ndev) is lb_gpu_comm_init_all.  ranks * k <= 16384. */
typedef struct lb_gpu_comm lb_gpu_comm;
/* host-supplied all-gather between HOST buffers: recv holds nranks blocks of `bytes` in rank order; 0 = ok */
typedef int (*lb_allgather_fn)(void *ctx, const void *send, void *recv, size_t bytes);
#define LB_COMM_UNIQUE_ID_BYTES 128
/* ONE process drives ndev GPUs (the Go server): devices NULL = 0..ndev-1.  RCCL (ncclCommInitAll). */
lb_gpu_comm *lb_gpu_comm_init_all(int ndev, const int *devices, int *out_status);
/* one process (or thread) per GPU: rank 0 calls get_unique_id and ships the 128 bytes to the others */
int lb_gpu_comm_get_unique_id(void *out128);
lb_gpu_comm *lb_gpu_comm_init_rank(int device, int nranks, int rank, const void *unique_id, int *out_status);
/* one process per GPU with the exchange done by the host (gloo / MPI / gRPC), staged through pinned memory */
lb_gpu_comm *lb_gpu_comm_init_host(int device, int nranks, int rank, lb_allgather_fn fn, void *ctx, int *out_status);
void lb_gpu_comm_free(lb_gpu_comm *c);
int lb_gpu_comm_nranks(const lb_gpu_comm *c);
int lb_gpu_comm_rank(const lb_gpu_comm *c);
const char *lb_gpu_comm_last_error(const lb_gpu_comm *c);
/* Size the exchange buffers (device blocks, pinned host blocks of the host transport, per-device query buffers of init_all)
 * for searches of up to nq_max queries and k_max results.  NOT collective: each rank calls it on its own, right after init,
 * and acts on its return code before any search is issued.  A search within the prepared size allocates nothing between
 * the shard search and the exchange, so an out-of-memory condition on one rank cannot leave its peers waiting in the
 * all-gather.  (A larger search still grows the buffers on the fly, with that risk.) */
int lb_gpu_comm_prepare(lb_gpu_comm *c, int64_t nq_max, int k_max);
/* init_rank / init_host communicators: this rank's shard h, the same nq queries on every rank (device
 * pointer), global top-k on every rank.  Collective: every rank must call it with the same nq and k. */
int lb_gpu_comm_search_device(lb_gpu_comm *c, lb_gpu_index *h, int64_t nq, const float *d_queries, int k, float *d_dist,
                              int64_t *d_labels, void *stream);
/* init_all communicators: shards[i] lives on the communicator's i-th device; host queries in, host results out */
int lb_gpu_comm_search_all(lb_gpu_comm *c, lb_gpu_index *const *shards, int64_t nq, const float *queries, int k, float *dist,
                           int64_t *labels);

/* ---- Arrow Flight framing (SURVEY f-1 / f-2) -----------------------------------------------------
 * The bytes of the Flight messages in, the bytes of the response out: a Go (or C) host needs no Arrow glue.
 * Return values of the lb_flight_* calls that parse requests are gRPC status codes, as the reference handler
 * returns them (0 OK, 3 InvalidArgument, 5 NotFound, 9 FailedPrecondition, 13 Internal, 14 Unavailable), with
 * the reference's message text in errbuf (nullable). */
typedef struct lb_flight_datasets lb_flight_datasets; /* name -> index (VectorStore.getDataset) */
lb_flight_datasets *lb_flight_datasets_new(void);
void lb_flight_datasets_free(lb_flight_datasets *r);
/* register (h != NULL) or remove (h == NULL) a dataset; the index stays owned by the caller */
int lb_flight_datasets_put(lb_flight_datasets *r, const char *name, lb_gpu_index *h);
/* VectorStore.handleVectorSearchExchange (internal/store/vector_search_exchange.go:31-217): ipc_in = an Arrow
 * IPC stream with ONE request batch {dataset utf8, k int32 (default 10), ef int32 (ignored), query_vector
 * FixedSizeList<float32> | List<float32>}, row 0 only; *ipc_out = an IPC stream with the response batch
 * {id uint64, score float32} (min(k, N) rows), to be released with lb_flight_free_buffer. */
int lb_flight_vector_search_exchange(lb_flight_datasets *reg, const uint8_t *ipc_in, size_t len_in, uint8_t **ipc_out,
                                     size_t *len_out, char *errbuf, size_t errcap);
/* One result batch {id uint64, score float32} as IPC stream bytes (trailing -1 labels trimmed): the per-query
 * flight.Result of DoAction("VectorSearch") (internal/store/vector_search_action.go:180-231).  lb_status. */
int lb_flight_encode_results(const int64_t *ids, const float *scores, int64_t n, uint8_t **ipc_out, size_t *len_out);
void lb_flight_free_buffer(uint8_t *p);
/* Append every record batch of an IPC stream: column "vector" FixedSizeList<float32>[dim] (its values buffer
 * goes to lb_gpu_index_add as it lies in the message body) and optional "id" (uint32 / uint64 / int64,
 * truncated to the reference's uint32 VectorID).  internal/store/store_lifecycle.go:66-76. */
int lb_flight_index_add_ipc(lb_gpu_index *h, const uint8_t *ipc, size_t len, int64_t *rows_added, char *errbuf, size_t errcap);

/* ---- hybrid fusion ---------------------------------------------------------------------
 * store.ReciprocalRankFusion (internal/store/rrf.go:10-51) for nq queries at once: per query a dense
 * ranking ids[kd] and a sparse ranking ids[ks] (best first, -1 = padding, ids unique within a list);
 * score(id) = sum 1/float64(k + rank + 1) (k <= 0 -> 60), narrowed to f32; output limit ids/scores per
 * query, score descending (ties: lower id first), padded with -1 / 0.  kd + ks <= 8192. */
int lb_gpu_rrf_fuse_device(int device, int64_t nq, int kd, const int64_t *d_dense_ids, int ks,
                           const int64_t *d_sparse_ids, int k, int limit, int64_t *d_out_ids,
                           float *d_out_scores, void *stream);
int lb_gpu_rrf_fuse(int device, int64_t nq, int kd, const int64_t *dense_ids, int ks, const int64_t *sparse_ids,
                    int k, int limit, int64_t *out_ids, float *out_scores);

/* ---- synthetic data (bench / tests) ------------------------------------------------
 * Counter-based uniform [0,1) f32 / uniform u8, bit-identical to the oracle's
 * lbo_fill_uniform / lbo_fill_codes. */
int lb_gpu_fill_uniform_device(int device, float *d_dst, int64_t n, uint64_t seed, int64_t offset,
                               void *stream);
int lb_gpu_fill_codes_device(int device, uint8_t *d_dst, int64_t n, uint64_t seed, int64_t offset,
                             void *stream);
/* rows of a global synthetic corpus picked by id: dst[r][j] = uniform(seed, ids[r]*dim + j) -- what a shard of
 * a ring-partitioned corpus holds (bench.py) */
int lb_gpu_fill_uniform_rows_device(int device, float *d_dst, const int64_t *d_ids, int64_t nrows, int dim, uint64_t seed,
                                    void *stream);

/* Shader clock of `device` right now, in MHz: every CU spins for `spin_us` microseconds and compares its cycle counter
 * (s_memtime) with the constant 100 MHz counter (s_memrealtime).  bench.py calls it straight behind its timed steps so a
 * line says at which clock state it was measured (the same search runs 1.67-1.95 ms by clock state on one box).
 * Returns a negative status code (-LB_ERR_*) on failure. */
double lb_gpu_shader_clock_mhz(int device, int spin_us);

/* ---- instrumentation (bench.py roofline leg) ----------------------------------------
 * HIP-event timing of the dominant kernels of the most recent search on this handle,
 * recorded on the stream the kernels ran on.  Enable before the search. */
int lb_gpu_index_set_profiling(lb_gpu_index *h, int enable);
/* ms spent in: [0] candidate GEMM kernels, [1] select kernels (and the three launches that build the view of a call with a
 * row bitmap, "call bitmap" above), [2] re-rank, [3] scan
 * kernels, [4] whole search (device side).  n_launch[i] = launches of that class. */
int lb_gpu_index_last_timing(const lb_gpu_index *h, float ms[5], int n_launch[5]);

#ifdef __cplusplus
}
#endif
#endif
