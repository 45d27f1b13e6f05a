// lb_pq4.h -- what pq4.hip (the host side of lb_gpu_pq4_*) and kernels_pq4.hip share: the layout of a packed 4-bit code row and
// the launchers.  A PQ4 codebook has 16 centroids per subspace; a code is a nibble.
//   across the ABI   a code row is M bytes, one per subspace, each below 16 (what the reference's Encode returns)
//   in HBM           a row is P = ceil(M / 2) bytes at stride P: byte b holds code 2b in its low nibble and code 2b + 1 in its
//                    high nibble; the spare high nibble of an odd M is 0
//   a query's table  float[M * 16], table[j * 16 + c] (pq.BuildADCTable at K = 16; launch_build_adc_table writes stride K)
#pragma once
#include "lb_device.h"

namespace lb {

constexpr int PQ4_K = 16;
constexpr int PQ4_MAX_M = 1024;
constexpr int PQ4_REG_MAX_M = 128; // up to here a query's table sits in M / 4 VGPRs (kernels_pq4.hip); beyond, in LDS
constexpr int PQ4_WAVES = 4;       // waves per workgroup of the scan: a workgroup owns runs of PQ4_WAVES * 64 rows
inline int pq4_row_bytes(int M) { return (M + 1) / 2; }
// queries the scan serves in one pass over the codes: 4 or 2 tables in registers, 2 in LDS
inline int pq4_max_queries_per_pass(int M, bool lds_lookup) { return !lds_lookup && M <= 96 ? 4 : 2; }

// n vectors f32[M * sub] -> their codes (encodeSequential: L2Squared in the UNROLL4 order to the 16 centroids in order, best
// starting at FLT_MAX, strict <, first wins, code 0 when nothing is below FLT_MAX); packed: rows of P bytes, else of M bytes
void launch_pq4_encode(const float *codebooks, int M, int sub, const float *X, int64_t n, uint8_t *out, bool packed, hipStream_t s);
// n rows of M bytes -> n packed rows; *bad (zero before the launch) becomes non-zero when a byte is 16 or more
void launch_pq4_pack(const uint8_t *codes, int M, int64_t n, uint8_t *packed, uint32_t *bad, hipStream_t s);
void launch_pq4_unpack(const uint8_t *packed, int M, int64_t n, uint8_t *codes, hipStream_t s);
// One pass over rows [row_begin, row_end) of the packed codes for the g queries (1 .. pq4_max_queries_per_pass(M)) whose
// tables lie one after the other at `tables` and whose candidate slots are slot .. slot + g - 1:
//   all_out != nullptr (g == 1)   every distance to all_out[row - out_base]
//   boot                          every row's entry to lists[slot + q][row - row_begin], no test and no atomics
//   otherwise                     the entries below the slot's tau are appended (cnt may pass cap: the select reports it)
// lds_lookup: the tables sit in LDS whatever M (always so beyond PQ4_REG_MAX_M)
void launch_pq4_scan(const float *tables, int M, const uint8_t *codes, int64_t row_begin, int64_t row_end, int slot, int g,
                     CandState cs, bool boot, float *all_out, int64_t out_base, bool lds_lookup, hipStream_t s);
// exact entries of `count` evenly spaced rows of [0, n) for one query -> out[count] (as launch_adc_sample)
void launch_pq4_sample(const float *table, int M, const uint8_t *codes, int64_t n, uint32_t count, uint64_t *out, bool lds_lookup,
                       hipStream_t s);

} // namespace lb
