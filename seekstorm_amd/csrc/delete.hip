// delete_documents_by_query on the device (delete.h): the whole match sets of a chunk ORed into the call's pending bitmap, and the one
// kernel that takes the tombstones off it, counts what is left and -- for real -- writes the live bitmap.
#include <algorithm>

#include "delete.h"

static_assert((BM_SUB / 64) % 2 == 0, "a match-set row is a whole number of 16-byte pairs");

constexpr uint32_t DEL_THREADS = 256;

// One lane owns a PAIR of u64 groups (16 bytes): consecutive lanes take consecutive pairs, a row is read with one 16-byte load per
// lane and the pending pair is read and written once -- no atomics.  The row loop is uniform over the grid (the mask is a kernel
// argument), so the loads of the rows of one pair are independent and stay in flight together.
__global__ void __launch_bounds__(DEL_THREADS) delete_collect_kernel(ulonglong2* __restrict__ pending, const ulonglong2* __restrict__ bits,
                                                                     unsigned long long pairs, unsigned long long row_mask) {
  for (unsigned long long p = (unsigned long long)blockIdx.x * DEL_THREADS + threadIdx.x; p < pairs; p += (unsigned long long)gridDim.x * DEL_THREADS) {
    ulonglong2 acc = pending[p];
    for (unsigned long long m = row_mask; m; m &= m - 1ull) {
      const uint32_t r = (uint32_t)__ffsll((long long)m) - 1u;
      const ulonglong2 v = bits[(unsigned long long)r * pairs + p];
      acc.x |= v.x;
      acc.y |= v.y;
    }
    pending[p] = acc;
  }
}

// One lane per u32 word and trip.  popc(fresh) is reduced per wave (shuffles), per workgroup (LDS) and leaves as ONE 64-bit atomic add
// per workgroup.  The image's last u64 group may have only its low u32 word inside the tombstone bitmap: every access of `deleted` is
// guarded by del_words, every access of `pending` by pend_words.
__global__ void __launch_bounds__(DEL_THREADS) delete_commit_kernel(uint32_t* __restrict__ pending, unsigned long long pend_words,
                                                                    uint32_t* __restrict__ deleted, unsigned long long del_words, uint32_t commit,
                                                                    unsigned long long* __restrict__ count) {
  __shared__ uint32_t s_wave[DEL_THREADS / 64];
  uint32_t n = 0;
  for (unsigned long long w = (unsigned long long)blockIdx.x * DEL_THREADS + threadIdx.x; w < pend_words; w += (unsigned long long)gridDim.x * DEL_THREADS) {
    const uint32_t have = pending[w];
    if (have == 0u) continue;
    const bool inside = w < del_words;
    const uint32_t old = inside ? deleted[w] : 0u;
    const uint32_t fresh = have & ~old;
    if (fresh != have) pending[w] = fresh;
    if (commit && inside && fresh) deleted[w] = old | fresh;
    n += (uint32_t)__popc(fresh);
  }
  for (int o = 32; o > 0; o >>= 1) n += __shfl_down(n, o);
  if ((threadIdx.x & 63u) == 0u) s_wave[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
    for (uint32_t i = 0; i < DEL_THREADS / 64; i++) t += s_wave[i];
    if (t) atomicAdd(count, t);
  }
}

int ssi_delete_collect(unsigned long long* d_pending, const unsigned long long* d_bits, uint64_t groups, uint64_t row_mask, hipStream_t st) {
  if (groups == 0 || row_mask == 0) return SS_OK;
  const unsigned long long pairs = groups / 2;
  const unsigned grid = (unsigned)std::min<unsigned long long>((pairs + DEL_THREADS - 1) / DEL_THREADS, 4096ull);
  delete_collect_kernel<<<grid, DEL_THREADS, 0, st>>>((ulonglong2*)d_pending, (const ulonglong2*)d_bits, pairs, (unsigned long long)row_mask);
  SS_HIP(hipGetLastError());
  return SS_OK;
}

int ssi_delete_commit(uint32_t* d_pending, uint64_t pend_words, uint32_t* d_deleted, uint64_t del_words, bool commit, unsigned long long* d_count,
                      hipStream_t st) {
  if (pend_words == 0) return SS_OK;
  const unsigned grid = (unsigned)std::min<unsigned long long>((pend_words + DEL_THREADS - 1) / DEL_THREADS, 4096ull);
  delete_commit_kernel<<<grid, DEL_THREADS, 0, st>>>(d_pending, (unsigned long long)pend_words, d_deleted, d_deleted ? (unsigned long long)del_words : 0ull,
                                                     commit ? 1u : 0u, d_count);
  SS_HIP(hipGetLastError());
  return SS_OK;
}
