// Kernels of the facet commit seam (facet_commit.h) for gfx950: the rank column of a string facet, gathered once per commit or table
// so that a sort reads a plain u32 key instead of chasing id -> rank in every radix pass; and the tombstone scatter of ss_add_deleted.
#include <map>
#include <memory>
#include <mutex>

#include "facet_commit.h"

static std::mutex g_side_mu;
static std::map<const ss_shard*, std::unique_ptr<ss_facet_side>> g_side;
ss_facet_side* ssi_facet_side(const ss_shard* s, bool create) {
  std::lock_guard<std::mutex> g(g_side_mu);
  auto it = g_side.find(s);
  if (it != g_side.end()) return it->second.get();
  if (!create) return nullptr;
  return (g_side[s] = std::make_unique<ss_facet_side>()).get();
}
void ssi_facet_side_drop(const ss_shard* s) {
  std::lock_guard<std::mutex> g(g_side_mu);
  auto it = g_side.find(s);
  if (it == g_side.end()) return;
  for (uint32_t i = 0; i < it->second->n_ranks; i++) {
    if (it->second->ranks[i].d_rank) (void)hipFree(it->second->ranks[i].d_rank);
    if (it->second->ranks[i].d_col) (void)hipFree(it->second->ranks[i].d_col);
  }
  g_side.erase(it);
}
const uint32_t* ssi_facet_rank_column(const ss_shard* s, uint32_t offset, uint32_t type) {
  const ss_facet_side* S = ssi_facet_side(s, false);
  if (!S) return nullptr;
  for (uint32_t i = 0; i < S->n_ranks; i++)
    if (S->ranks[i].offset == offset && S->ranks[i].type == type) return S->ranks[i].d_col;
  return nullptr;
}

// one thread per record; the id is read byte by byte (a facet sits at any offset of its record)
__global__ void facet_rank_gather_kernel(const uint8_t* __restrict__ records, uint32_t record_size, uint32_t offset, uint32_t bytes,
                                         unsigned long long n, const uint32_t* __restrict__ rank, uint32_t n_ids, uint32_t* __restrict__ col,
                                         unsigned long long* __restrict__ bad) {
  const unsigned long long d = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  bool is_bad = false;
  if (d < n) {
    const uint8_t* p = records + d * record_size + offset;
    uint32_t id = 0;
    for (uint32_t b = 0; b < bytes; b++) id |= (uint32_t)p[b] << (8u * b);
    is_bad = id >= n_ids;
    col[d] = is_bad ? 0xFFFFFFFFu : rank[id];
  }
  const unsigned long long m = __ballot(is_bad);
  if (m && (threadIdx.x & 63u) == 0u) atomicAdd(bad, (unsigned long long)__popcll(m));
}
int ssi_facet_rank_gather(const uint8_t* records, uint32_t record_size, uint32_t offset, uint32_t type, uint64_t n, const uint32_t* d_rank,
                          uint32_t n_ids, uint32_t* d_col, unsigned long long* d_bad, hipStream_t st) {
  if (n == 0) return SS_OK;
  facet_rank_gather_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(records, record_size, offset, ssi_facet_width(type), (unsigned long long)n,
                                                                       d_rank, n_ids, d_col, d_bad);
  SS_HIP(hipGetLastError());
  return SS_OK;
}

__global__ void facet_rank_read_kernel(const uint32_t* __restrict__ col, unsigned long long n_docs, const uint32_t* __restrict__ docs, uint32_t n,
                                       uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = docs[i] < n_docs ? col[docs[i]] : 0xFFFFFFFFu;
}
int ssi_facet_rank_read(const uint32_t* d_col, uint64_t n_docs, const uint32_t* d_docs, uint32_t n, uint32_t* d_out, hipStream_t st) {
  if (n == 0) return SS_OK;
  facet_rank_read_kernel<<<(n + 255) / 256, 256, 0, st>>>(d_col, (unsigned long long)n_docs, d_docs, n, d_out);
  SS_HIP(hipGetLastError());
  return SS_OK;
}

// one thread per id.  atomicOr returns the word as it was: of several threads that bring the same doc exactly one sees its bit clear,
// so the sum counts DISTINCT docs that were not deleted before.
__global__ void deleted_scatter_kernel(uint32_t* __restrict__ bits, const uint32_t* __restrict__ ids, unsigned long long n,
                                       unsigned long long* __restrict__ n_new) {
  const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  bool fresh = false;
  if (i < n) {
    const uint32_t id = ids[i], b = 1u << (id & 31u);
    fresh = (atomicOr(&bits[id >> 5], b) & b) == 0u;
  }
  const unsigned long long m = __ballot(fresh);
  if (m && (threadIdx.x & 63u) == 0u) atomicAdd(n_new, (unsigned long long)__popcll(m));
}
int ssi_deleted_scatter(uint32_t* d_bits, const uint32_t* d_ids, uint64_t n, unsigned long long* d_new, hipStream_t st) {
  if (n == 0) return SS_OK;
  deleted_scatter_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(d_bits, d_ids, (unsigned long long)n, d_new);
  SS_HIP(hipGetLastError());
  return SS_OK;
}
