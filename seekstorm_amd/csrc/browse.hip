// The empty query of a shard (ss_docs_search; search_iterator_shard, iterator.rs:316-358): no term, so no posting list is read and
// nothing is scored.  The match set is "every live doc that passes the facet filter" -- all ones below n_docs AND NOT the exclusion
// bitmap in force -- and the rank of a doc is its id (min_heap.rs:535-536, 1043-1044: the larger id is the better one).
//
// A page by doc id needs no heap: with the popcount of every 256-word slice of the bitmap known, one workgroup scans the slice counts
// in rank order (from the last slice down for descending ids) and leaves every slice the rank of its first doc; a slice whose ranks
// overlap [skip, skip + take) then emits its part of the page -- a popcount prefix over its words in LDS, a binary search for the word
// of rank i and a rank select inside the word -- so a top-10 touches one slice and a page of any depth costs one pass over the bitmap
// (8 bytes per 64 docs).  The same selection lists the two doc sets ssi_sort_select leaves of a sorted browse (facet.hip).
#include "browse.h"
#include "bit_select.h"

namespace {
constexpr uint32_t BR_THREADS = BROWSE_SLICE;  // one thread per word of a slice
constexpr uint32_t BR_SCAN = 1024;             // threads of the one-block scan over the slice counts

// sum of v over the workgroup (blockDim.x = NT, a multiple of 64); every thread gets it
template <uint32_t NT>
__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t* s_wave) {
  for (uint32_t o = 32u; o > 0u; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63u) == 0u) s_wave[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t t = 0;
  for (uint32_t w = 0; w < NT / 64u; w++) t += s_wave[w];
  __syncthreads();  // (s_wave may be written again)
  return t;
}
// exclusive prefix of v over the workgroup in thread order; *total = the sum
template <uint32_t NT>
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* s_wave, uint32_t* total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t inc = v;
  for (uint32_t o = 1u; o < 64u; o <<= 1) {
    const uint32_t y = __shfl_up(inc, o);
    if (lane >= o) inc += y;
  }
  if (lane == 63u) s_wave[wave] = inc;
  __syncthreads();
  uint32_t base = 0, t = 0;
  for (uint32_t w = 0; w < NT / 64u; w++) { if (w < wave) base += s_wave[w]; t += s_wave[w]; }
  __syncthreads();
  *total = t;
  return base + inc - v;
}
}  // namespace

// bits[g] = (ones below n_docs) & ~excl; excl = the 32-bit-word bitmap of tombstones | facet filter, del_words words (a bitmap shorter
// than the image excludes nobody beyond its end; nullptr: nobody is excluded).  blockIdx.x = the slice.
__global__ void __launch_bounds__(BR_THREADS) browse_bits_kernel(unsigned long long* __restrict__ bits, unsigned long long groups,
                                                                 unsigned long long n_docs, const uint32_t* __restrict__ del,
                                                                 unsigned long long del_words, uint32_t* __restrict__ slice_cnt,
                                                                 unsigned long long* __restrict__ total) {
  __shared__ uint32_t s_wave[BR_THREADS / 64];
  const unsigned long long g = (unsigned long long)blockIdx.x * BR_THREADS + threadIdx.x;
  unsigned long long m = 0ull;
  if (g < groups) {
    const unsigned long long d0 = g * 64ull;
    if (d0 < n_docs) {
      m = n_docs - d0 >= 64ull ? ~0ull : ((1ull << (n_docs - d0)) - 1ull);  // no doc at or beyond n_docs: the padded tail stays zero
      if (del) {
        const unsigned long long lo = 2ull * g < del_words ? del[2ull * g] : 0u, hi = 2ull * g + 1ull < del_words ? del[2ull * g + 1ull] : 0u;
        m &= ~(lo | (hi << 32));
      }
    }
    bits[g] = m;
  }
  const uint32_t t = block_sum<BR_THREADS>((uint32_t)__popcll(m), s_wave);
  if (threadIdx.x == 0) {
    slice_cnt[blockIdx.x] = t;
    if (t) atomicAdd(total, (unsigned long long)t);
  }
}

// the popcount of every slice of a bitmap somebody else wrote (the two doc sets of a sorted browse)
__global__ void __launch_bounds__(BR_THREADS) browse_count_kernel(const unsigned long long* __restrict__ bits, unsigned long long groups,
                                                                  uint32_t* __restrict__ slice_cnt) {
  __shared__ uint32_t s_wave[BR_THREADS / 64];
  const unsigned long long g = (unsigned long long)blockIdx.x * BR_THREADS + threadIdx.x;
  const uint32_t t = block_sum<BR_THREADS>(g < groups ? (uint32_t)__popcll(bits[g]) : 0u, s_wave);
  if (threadIdx.x == 0) slice_cnt[blockIdx.x] = t;
}

// ONE workgroup: slice_begin[s] = the rank of slice s's first doc -- the docs of the slices that come before it in rank order (the
// slices after it in memory for descending ids) -- and *out_n = min(take, matches - skip), the number of docs the page holds
__global__ void __launch_bounds__(BR_SCAN) browse_locate_kernel(const uint32_t* __restrict__ slice_cnt, unsigned long long n_slices,
                                                                uint32_t descending, unsigned long long skip, unsigned long long take,
                                                                unsigned long long* __restrict__ slice_begin, uint32_t* __restrict__ out_n) {
  __shared__ uint32_t s_wave[BR_SCAN / 64];
  unsigned long long carry = 0ull;
  for (unsigned long long j0 = 0; j0 < n_slices; j0 += BR_SCAN) {  // (uniform trip count: the barriers inside the scan are met by all)
    const unsigned long long j = j0 + threadIdx.x;
    const unsigned long long s = descending ? n_slices - 1ull - j : j;
    const uint32_t v = j < n_slices ? slice_cnt[s] : 0u;
    uint32_t t;
    const uint32_t e = block_exclusive_scan<BR_SCAN>(v, s_wave, &t);
    if (j < n_slices) slice_begin[s] = carry + e;
    carry += t;
  }
  if (threadIdx.x == 0) {
    const unsigned long long left = carry > skip ? carry - skip : 0ull;
    *out_n = (uint32_t)(left < take ? left : take);  // (doc ids are 32-bit: fewer than 2^32 matches)
  }
}

// blockIdx.x = the slice: its docs of rank [skip, skip + *out_n) go to out_doc[rank - skip]; a slice outside the page returns at once
__global__ void __launch_bounds__(BR_THREADS) browse_emit_kernel(const unsigned long long* __restrict__ bits, unsigned long long groups,
                                                                 const uint32_t* __restrict__ slice_cnt,
                                                                 const unsigned long long* __restrict__ slice_begin, uint32_t descending,
                                                                 unsigned long long skip, const uint32_t* __restrict__ out_n,
                                                                 uint32_t* __restrict__ out_doc) {
  __shared__ unsigned long long s_word[BR_THREADS];
  __shared__ uint32_t s_pre[BR_THREADS + 1];
  __shared__ uint32_t s_wave[BR_THREADS / 64];
  const unsigned long long begin = slice_begin[blockIdx.x], end = skip + (unsigned long long)*out_n;
  const uint32_t cnt = slice_cnt[blockIdx.x];
  if (cnt == 0u || begin + cnt <= skip || begin >= end) return;  // (the whole workgroup)
  // thread p holds the slice's p-th word in RANK order: the last word first for descending ids
  const uint32_t p = threadIdx.x;
  const unsigned long long w0 = (unsigned long long)blockIdx.x * BR_THREADS;
  const unsigned long long g = descending ? w0 + (BR_THREADS - 1u - p) : w0 + p;
  const unsigned long long m = g < groups ? bits[g] : 0ull;
  s_word[p] = m;
  uint32_t T;
  s_pre[p] = block_exclusive_scan<BR_THREADS>((uint32_t)__popcll(m), s_wave, &T);
  if (p == 0) s_pre[BR_THREADS] = T;
  __syncthreads();
  // ranks of this slice inside the page, as indices into the slice's own docs (T = cnt: the counts were taken from these words)
  const uint32_t i0 = skip > begin ? (uint32_t)(skip - begin) : 0u;
  const uint32_t i1 = end - begin < (unsigned long long)T ? (uint32_t)(end - begin) : T;
  for (uint32_t i = i0 + p; i < i1; i += BR_THREADS) {
    uint32_t lo = 0, hi = BR_THREADS;  // s_pre[lo] <= i < s_pre[hi]: the word that holds the slice's i-th doc
    while (hi - lo > 1u) {
      const uint32_t mid = (lo + hi) >> 1;
      if (s_pre[mid] <= i) lo = mid; else hi = mid;
    }
    const unsigned long long w = s_word[lo];
    const uint32_t r = i - s_pre[lo];  // < popcount(w)
    const uint32_t bit = facet_select64(w, descending ? (uint32_t)__popcll(w) - 1u - r : r);
    const unsigned long long gw = descending ? w0 + (BR_THREADS - 1u - lo) : w0 + lo;
    out_doc[begin + i - skip] = (uint32_t)(gw * 64ull + bit);  // begin + i < end: inside the page
  }
}

__global__ void browse_clear_kernel(unsigned long long* __restrict__ bits, unsigned long long groups, const uint32_t* __restrict__ docs,
                                    uint32_t n, unsigned long long* __restrict__ count) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const uint32_t d = docs[i];
    if ((unsigned long long)(d >> 6) < groups) atomicAnd(&bits[d >> 6], ~(1ull << (d & 63u)));
  }
  if (i == 0) *count -= *count < n ? *count : n;
}

int ssi_browse_bits(ss_shard* s, unsigned long long* d_bits, uint32_t* d_slice_cnt, unsigned long long* d_total, hipStream_t st) {
  const unsigned long long groups = (unsigned long long)s->bm_n_sub * (BM_SUB / 64);
  if (groups == 0) return SS_OK;
  browse_bits_kernel<<<(unsigned)browse_slices(groups), BR_THREADS, 0, st>>>(d_bits, groups, (unsigned long long)s->bm_n_docs,
                                                                             s->n_deleted ? s->d_deleted : nullptr,
                                                                             (unsigned long long)s->deleted_words, d_slice_cnt, d_total);
  SS_HIP(hipGetLastError());
  return SS_OK;
}

int ssi_browse_select(ss_shard* s, const unsigned long long* d_bits, bool descending, uint64_t skip, uint64_t take, uint32_t* d_slice_cnt,
                      unsigned long long* d_slice_begin, bool slices_counted, uint32_t* d_out_doc, uint32_t* d_out_n, hipStream_t st) {
  const unsigned long long groups = (unsigned long long)s->bm_n_sub * (BM_SUB / 64);
  const unsigned long long n_slices = browse_slices(groups);
  if (n_slices == 0) { SS_HIP(hipMemsetAsync(d_out_n, 0, sizeof(uint32_t), st)); return SS_OK; }
  if (!slices_counted) browse_count_kernel<<<(unsigned)n_slices, BR_THREADS, 0, st>>>(d_bits, groups, d_slice_cnt);
  browse_locate_kernel<<<1, BR_SCAN, 0, st>>>(d_slice_cnt, n_slices, descending ? 1u : 0u, (unsigned long long)skip, (unsigned long long)take,
                                              d_slice_begin, d_out_n);
  browse_emit_kernel<<<(unsigned)n_slices, BR_THREADS, 0, st>>>(d_bits, groups, d_slice_cnt, d_slice_begin, descending ? 1u : 0u,
                                                                (unsigned long long)skip, d_out_n, d_out_doc);
  SS_HIP(hipGetLastError());
  return SS_OK;
}

int ssi_browse_clear(ss_shard* s, unsigned long long* d_bits, const uint32_t* d_docs, uint32_t n, unsigned long long* d_count, hipStream_t st) {
  if (n == 0) return SS_OK;
  const unsigned long long groups = (unsigned long long)s->bm_n_sub * (BM_SUB / 64);
  browse_clear_kernel<<<(n + 255u) / 256u, 256, 0, st>>>(d_bits, groups, d_docs, n, d_count);
  SS_HIP(hipGetLastError());
  return SS_OK;
}
