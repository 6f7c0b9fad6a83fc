// The buckets of a query's score histogram (bm25_probe_body.h pb_publish_hist; laid out by bm25.hip bm_expand_one): B equal steps in
// float-BIT space between the query's `lo` and `hi`.  Scores are positive floats, so their bit patterns order like unsigned integers
// and a bucket's edge is a bit pattern too: lo_bits + (b << shift), never computed in float arithmetic -- edge(bucket(s)) <= s holds
// exactly.  Shared by hipcc (__host__ __device__) and plain g++ (tests/hist_threshold_check.cpp): no std::, nothing else included.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define BMH_FN __host__ __device__ inline
#else
#define BMH_FN inline
#endif

constexpr uint32_t BM_HIST_B = 64;             // buckets a query: one counter per lane
constexpr uint32_t BM_HIST_NONE = 0xFFFFFFFFu;  // bucket of a score below `lo`: not counted
// tau line of a query (bm25_dev.h BM_TAU_STRIDE): dword 0 the threshold, 1 the "contradicted the claim" mark, then the bucket rule
constexpr uint32_t BM_TAU_HIST_LO = 2, BM_TAU_HIST_SHIFT = 3;
// A query without a seed (tombstones, NOT terms, filters in force) starts its buckets at this share of `hi` = sum of idf x umax:
// DESIGN section 3.2 has the model's figures for the choice.
constexpr float BM_HIST_SEEDLESS_LO = 0.25f;

// the smallest shift with (hi_bits - lo_bits) >> shift < B (hi_bits >= lo_bits)
BMH_FN uint32_t bm_hist_shift(uint32_t lo_bits, uint32_t hi_bits) {
  uint32_t shift = 0u;
  while (((hi_bits - lo_bits) >> shift) >= BM_HIST_B) shift++;
  return shift;
}
// bucket of a score (its bit pattern): scores at or above `hi` land in the last one
BMH_FN uint32_t bm_hist_bucket(uint32_t bits, uint32_t lo_bits, uint32_t shift) {
  if (bits < lo_bits) return BM_HIST_NONE;
  const uint32_t b = (bits - lo_bits) >> shift;
  return b < BM_HIST_B - 1u ? b : BM_HIST_B - 1u;
}
// lower edge of bucket b as a bit pattern (b <= the bucket of some score: then it cannot overflow)
BMH_FN uint32_t bm_hist_edge(uint32_t b, uint32_t lo_bits, uint32_t shift) { return lo_bits + (b << shift); }
