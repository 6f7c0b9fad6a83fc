// Rank select inside a 64-bit word (facet.hip's compaction of a match bitmap, browse.hip's doc-id selection).  Internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// position of the r-th (0-based) set bit of m; r < popcount(m)
__device__ __forceinline__ uint32_t facet_select64(unsigned long long m, uint32_t r) {
  uint32_t pos = 0, c = (uint32_t)__popc((uint32_t)m);
  if (r >= c) { r -= c; m >>= 32; pos = 32; }
  uint32_t x = (uint32_t)m;
  c = (uint32_t)__popc(x & 0xFFFFu); if (r >= c) { r -= c; x >>= 16; pos += 16; }
  c = (uint32_t)__popc(x & 0xFFu); if (r >= c) { r -= c; x >>= 8; pos += 8; }
  c = (uint32_t)__popc(x & 0xFu); if (r >= c) { r -= c; x >>= 4; pos += 4; }
  c = (uint32_t)__popc(x & 3u); if (r >= c) { r -= c; x >>= 2; pos += 2; }
  if (r >= (x & 1u)) pos += 1;
  return pos;
}
