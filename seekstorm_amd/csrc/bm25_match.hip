// Match sets of queries that name SPARSE-tier terms, as bitmaps on the device (bm25_match.h): what facet counts, the sort pivot and
// result sorts walk.  ssi_bm25_match_bits (bm25.hip) answers from the probe index's bit records, which only dense lists have; a
// sparse list is a plain sorted array of 8-byte postings (bm25_sparse.hip).  Three pieces put the two together:
//   * a query's dense part (BmTierPlan::sub) through ssi_bm25_match_bits as it is, into the query's slot of d_bits;
//   * mt_clear_kernel: the sparse NOT lists take their docs out of that part (atomicAnd);
//   * mt_set_kernel: a union's sparse lists add their docs (atomicOr) unless the doc is excluded -- bitmap in force, dense NOT lists
//     by a bit test in their probe rows, sparse NOT lists by binary search; an intersection's (or single term's) shortest sparse list
//     drives: a posting survives when every other term holds its doc (dense: bit test; sparse: binary search) in a listed field.
// Counts stay exact without a recount: the value an atomic returns says whether the bit changed; a lane sums its changes, a wave
// adds them to d_total once.  Sparse lists are short, so these are latency-bound gather / scatter kernels: four postings in flight
// per lane, plain vector loads, device-scope atomics, no LDS.
#include <algorithm>

#include "bm25_match.h"
#include "bm25_find.h"

namespace {

constexpr int MT_THREADS = 256, MT_UNROLL = 4;

struct MtParams {
  const ss_bm25_query* q;
  const unsigned long long* sp_base;
  const unsigned long long* sp_post;
  const uint2* probe;         // bit records: row r, group g at probe[r * n_groups + g]
  const uint32_t* probe_row;  // [dense lists + 1]
  const uint32_t* del;        // exclusion bitmap in force (32-bit words), or null
  unsigned long long* bits;   // [nq][n_groups]
  unsigned long long* total;  // [nq]
  uint32_t del_words, n_dense, n_lists, n_fields /* indexed fields: n_lists less the merged list */, n_groups, n_rows, n_docs;
};

// what the query is to the tiers (the same rules as ssi_bm25_tier_plan)
struct MtRole {
  uint32_t nt, n_not, filt;
  bool sparse_pos, dense_pos, sparse_not, driven;
};
__device__ __forceinline__ MtRole mt_role(const MtParams& P, const ss_bm25_query* __restrict__ Q) {
  MtRole R;
  R.nt = Q->n_terms;
  R.n_not = bm_q_nnot(Q->op);
  R.filt = P.n_fields > 1u ? bm_q_field_filter(Q->op) : 0u;
  R.sparse_pos = R.dense_pos = R.sparse_not = false;
  for (uint32_t t = 0; t < R.nt + R.n_not && t < (uint32_t)SS_MAX_QUERY_TERMS; t++) {
    const bool sp = Q->term[t] >= P.n_dense;
    if (t < R.nt) { R.sparse_pos |= sp; R.dense_pos |= !sp; } else R.sparse_not |= sp;
  }
  R.driven = R.sparse_pos && ((bm_q_op(Q->op) == SS_OP_INTERSECTION && R.nt > 1u) || R.nt == 1u || R.filt != 0u);
  return R;
}

__device__ __forceinline__ bool mt_excluded(const MtParams& P, uint32_t doc) {
  return P.del && (doc >> 5) < P.del_words && ((P.del[doc >> 5] >> (doc & 31u)) & 1u);
}
// doc in a DENSE term: one bit test per list the query reads of it -- the merged (or only) list without a field filter, else the
// lists of the fields in `fields`
__device__ __forceinline__ bool mt_dense_has(const MtParams& P, uint32_t term, uint32_t filt, uint32_t fields, uint32_t doc) {
  const uint32_t f_begin = filt ? 0u : P.n_lists - 1u, f_end = filt ? P.n_fields : P.n_lists;
  bool has = false;
  for (uint32_t f = f_begin; f < f_end; f++) {
    if (filt && !((fields >> f) & 1u)) continue;
    const uint32_t row = P.probe_row[term * P.n_lists + f];
    if (row >= P.n_rows) continue;  // (no row: the host refused the query; an absent list reads the all-zero row)
    const uint2 r = P.probe[(size_t)row * P.n_groups + (doc >> 6)];
    has |= (((doc & 32u) ? r.y : r.x) >> (doc & 31u)) & 1u;
  }
  return has;
}
// doc in a SPARSE list, in one of the fields of `fields` (0 = any)
__device__ __forceinline__ bool mt_sparse_has(const MtParams& P, uint32_t term, uint32_t fields, uint32_t doc) {
  const uint32_t j = term - P.n_dense;
  const unsigned long long b1 = P.sp_base[j + 1], p = sp_find(P.sp_post, P.sp_base[j], b1, doc);
  if (p >= b1) return false;
  const unsigned long long e = P.sp_post[p];
  return (uint32_t)e == doc && (!fields || (((uint32_t)(e >> 32) >> BM_SP_FIELD_SHIFT) & fields));
}
// a NOT term holds the doc in any field (add_result.rs:3440-3497), as the sparse kernel and the bit-record pass read them
__device__ __forceinline__ bool mt_in_not(const MtParams& P, const ss_bm25_query* __restrict__ Q, const MtRole& R, uint32_t doc) {
  bool hit = false;
  for (uint32_t t = R.nt; t < R.nt + R.n_not && !hit; t++) {
    const uint32_t term = Q->term[t];
    hit = term >= P.n_dense ? mt_sparse_has(P, term, 0u, doc) : mt_dense_has(P, term, R.filt, ~0u, doc);
  }
  return hit;
}
__device__ __forceinline__ uint32_t mt_wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// blockIdx.y = query; the workgroups of a query share its lists, MT_UNROLL postings per lane and step
__global__ void __launch_bounds__(MT_THREADS) mt_set_kernel(MtParams P, uint32_t nq) {
  const uint32_t qi = blockIdx.y;
  if (qi >= nq) return;
  const ss_bm25_query* __restrict__ Q = P.q + qi;
  const MtRole R = mt_role(P, Q);
  if (!R.sparse_pos) return;
  unsigned long long* __restrict__ bits = P.bits + (size_t)qi * P.n_groups;
  // the driver lists: a union walks every sparse list of the query, an intersection (single term) only its shortest one
  uint32_t first = 0, last = R.nt;
  if (R.driven) {
    unsigned long long best = ~0ull;
    for (uint32_t t = 0; t < R.nt; t++)
      if (Q->term[t] >= P.n_dense) {
        const uint32_t i = Q->term[t] - P.n_dense;
        const unsigned long long len = P.sp_base[i + 1] - P.sp_base[i];
        if (len < best) { best = len; first = t; }
      }
    last = first + 1;
  }
  uint32_t changed = 0;
  const unsigned long long step = (unsigned long long)gridDim.x * MT_THREADS;
  for (uint32_t s = first; s < last; s++) {
    if (Q->term[s] < P.n_dense) continue;
    const uint32_t si = Q->term[s] - P.n_dense;
    const unsigned long long b0 = P.sp_base[si], b1 = P.sp_base[si + 1];
    for (unsigned long long x0 = b0 + (unsigned long long)blockIdx.x * MT_THREADS + threadIdx.x; x0 < b1; x0 += step * MT_UNROLL) {
      unsigned long long e[MT_UNROLL];
#pragma unroll
      for (int u = 0; u < MT_UNROLL; u++) e[u] = x0 + step * u < b1 ? P.sp_post[x0 + step * u] : ~0ull;
#pragma unroll
      for (int u = 0; u < MT_UNROLL; u++) {
        const uint32_t doc = (uint32_t)e[u];
        bool live = x0 + step * u < b1 && doc < P.n_docs && (doc >> 6) < P.n_groups;
        if (live && R.driven) {
          if (R.filt && !(((uint32_t)(e[u] >> 32) >> BM_SP_FIELD_SHIFT) & R.filt)) live = false;
          for (uint32_t t = 0; t < R.nt && live; t++) {
            if (t == s) continue;
            const uint32_t term = Q->term[t];
            live = term >= P.n_dense ? mt_sparse_has(P, term, R.filt, doc) : mt_dense_has(P, term, R.filt, R.filt, doc);
          }
        }
        if (live && mt_excluded(P, doc)) live = false;
        if (live && R.n_not && mt_in_not(P, Q, R, doc)) live = false;
        if (live) {
          const unsigned long long b = 1ull << (doc & 63u);
          changed += (atomicOr(bits + (doc >> 6), b) & b) ? 0u : 1u;
        }
      }
    }
  }
  changed = mt_wave_sum(changed);
  if ((threadIdx.x & 63) == 0 && changed) atomicAdd(P.total + qi, (unsigned long long)changed);
}

// the sparse NOT lists of a query whose dense part the bit records answered: their docs leave the set
__global__ void __launch_bounds__(MT_THREADS) mt_clear_kernel(MtParams P, uint32_t nq) {
  const uint32_t qi = blockIdx.y;
  if (qi >= nq) return;
  const ss_bm25_query* __restrict__ Q = P.q + qi;
  const MtRole R = mt_role(P, Q);
  if (!R.sparse_not || !R.dense_pos || R.driven) return;
  unsigned long long* __restrict__ bits = P.bits + (size_t)qi * P.n_groups;
  uint32_t changed = 0;
  const unsigned long long step = (unsigned long long)gridDim.x * MT_THREADS;
  for (uint32_t t = R.nt; t < R.nt + R.n_not; t++) {
    if (Q->term[t] < P.n_dense) continue;
    const uint32_t si = Q->term[t] - P.n_dense;
    const unsigned long long b0 = P.sp_base[si], b1 = P.sp_base[si + 1];
    for (unsigned long long x0 = b0 + (unsigned long long)blockIdx.x * MT_THREADS + threadIdx.x; x0 < b1; x0 += step * MT_UNROLL) {
      unsigned long long e[MT_UNROLL];
#pragma unroll
      for (int u = 0; u < MT_UNROLL; u++) e[u] = x0 + step * u < b1 ? P.sp_post[x0 + step * u] : ~0ull;
#pragma unroll
      for (int u = 0; u < MT_UNROLL; u++) {
        const uint32_t doc = (uint32_t)e[u];
        if (x0 + step * u < b1 && doc < P.n_docs && (doc >> 6) < P.n_groups) {
          const unsigned long long b = 1ull << (doc & 63u);
          changed += (atomicAnd(bits + (doc >> 6), ~b) & b) ? 1u : 0u;
        }
      }
    }
  }
  changed = mt_wave_sum(changed);
  if ((threadIdx.x & 63) == 0 && changed) atomicAdd(P.total + qi, 0ull - (unsigned long long)changed);
}

struct Tiers { bool sparse_pos = false, dense_pos = false, sparse_not = false, driven = false; };
Tiers tiers_of(const ss_shard* s, const ss_bm25_query& q) {
  const uint32_t n_dense = s->bm_n_terms / s->bm_n_fields, n_not = bm_q_nnot(q.op);
  Tiers T;
  for (uint32_t t = 0; t < q.n_terms + n_not; t++) {
    const bool sp = q.term[t] >= n_dense;
    if (t < q.n_terms) { T.sparse_pos |= sp; T.dense_pos |= !sp; } else T.sparse_not |= sp;
  }
  const bool filt = bm_real_fields(s) > 1 && bm_q_field_filter(q.op) != 0u;
  T.driven = T.sparse_pos && ((bm_q_op(q.op) == SS_OP_INTERSECTION && q.n_terms > 1) || q.n_terms == 1 || filt);
  return T;
}

}  // namespace

int ssi_bm25_tier_plan(const ss_shard* s, uint32_t nq, const ss_bm25_query* q, BmTierPlan* plan) {
  const uint32_t n_dense = s->bm_n_terms / std::max<uint32_t>(s->bm_n_fields, 1u);
  plan->sub.assign(nq, ss_bm25_query{});
  plan->has_sub.assign(nq, 0);
  plan->tiered.assign(nq, 0);
  plan->any_tiered = false;
  if (!s->sp_n) return SS_OK;
  for (uint32_t i = 0; i < nq; i++) {
    const uint32_t op = bm_q_op(q[i].op), n_not = bm_q_nnot(q[i].op), all = q[i].n_terms + n_not;
    if (q[i].n_terms == 0 || all > (uint32_t)SS_MAX_QUERY_TERMS) return SS_EINVAL;
    bool any_sparse = false;
    for (uint32_t t = 0; t < all; t++) {
      if (q[i].term[t] >= n_dense + s->sp_n) return SS_EINVAL;
      any_sparse |= q[i].term[t] >= n_dense;
    }
    if (!any_sparse) {  // (check_queries has the rest to say about it)
      plan->sub[i] = q[i];
      plan->has_sub[i] = 1;
      continue;
    }
    for (uint32_t t = 0; t < all; t++) {
      if (t < q[i].n_terms && !(q[i].idf[t] > 0.0f)) return SS_EINVAL;
      for (uint32_t u = 0; u < t; u++)
        if (q[i].term[u] == q[i].term[t]) return SS_EINVAL;
    }
    if (op != SS_OP_INTERSECTION && op != SS_OP_UNION && op != SS_OP_PHRASE) return SS_EINVAL;
    if (bm_q_field_filter(q[i].op) >> bm_real_fields(s)) return SS_EINVAL;  // a field the image does not have
    if (s->bm_n_fields != 1 && !s->bm_merged) return SS_ENOTSUP;            // (the sparse tier holds merged weights)
    if (op == SS_OP_PHRASE || bm_q_all_frequent(q[i].op)) return SS_ENOTSUP;
    const bool filtered = bm_real_fields(s) > 1 && bm_q_field_filter(q[i].op) != 0u;
    if (filtered && op == SS_OP_UNION && q[i].n_terms > 1) return SS_ENOTSUP;  // the reference's sub-queries, not a per-doc test
    plan->tiered[i] = 1;
    plan->any_tiered = true;
    const Tiers T = tiers_of(s, q[i]);
    if (!T.dense_pos || T.driven) continue;
    ss_bm25_query d = q[i];  // the dense scored terms and the dense NOT terms, in their order
    uint32_t n = 0, nn = 0;
    for (uint32_t t = 0; t < q[i].n_terms; t++)
      if (q[i].term[t] < n_dense) { d.term[n] = q[i].term[t]; d.idf[n] = q[i].idf[t]; n++; }
    for (uint32_t t = q[i].n_terms; t < all; t++)
      if (q[i].term[t] < n_dense) { d.term[n + nn] = q[i].term[t]; nn++; }
    for (uint32_t t = n; t < (uint32_t)SS_MAX_QUERY_TERMS; t++) d.idf[t] = 0.f;
    for (uint32_t t = n + nn; t < (uint32_t)SS_MAX_QUERY_TERMS; t++) d.term[t] = 0;
    d.n_terms = n;
    d.op = (q[i].op & ~0xFF00u) | (nn << 8);
    plan->sub[i] = d;
    plan->has_sub[i] = 1;
  }
  return SS_OK;
}

int ssi_bm25_match_bits_tiered(ss_shard* s, const BmTierPlan& plan, const ss_bm25_query* h_q, const ss_bm25_query* d_q, ss_bm25_query* d_sub,
                               unsigned long long* d_bits, unsigned long long* d_total, hipStream_t st, uint32_t nq) {
  if (!s->d_post || !s->d_sp_base || !s->d_sp_post) return SS_ESTATE;
  if (!s->d_probe || !s->d_probe_row) return SS_ENOTSUP;
  if (nq == 0 || nq > 64 || plan.sub.size() != nq) return SS_EINVAL;
  const uint32_t L = s->bm_n_fields, RF = bm_real_fields(s), n_dense = s->bm_n_terms / L;
  const uint32_t n_groups = s->bm_n_sub * (BM_SUB / 64);
  bool any_set = false, any_clear = false;
  uint64_t longest = 0;
  for (uint32_t i = 0; i < nq; i++) {
    if (!plan.tiered[i]) continue;
    const ss_bm25_query& Q = h_q[i];
    const Tiers T = tiers_of(s, Q);
    any_set |= T.sparse_pos;
    any_clear |= T.sparse_not && T.dense_pos && !T.driven;
    const bool filt = RF > 1 && bm_q_field_filter(Q.op) != 0u;
    for (uint32_t t = 0; t < Q.n_terms + bm_q_nnot(Q.op); t++) {
      if (Q.term[t] >= n_dense) {
        const uint32_t j = Q.term[t] - n_dense;
        longest = std::max<uint64_t>(longest, s->h_sp_base[j + 1] - s->h_sp_base[j]);
        continue;
      }
      for (uint32_t f = filt ? 0u : L - 1u; f < (filt ? RF : L); f++) {  // the lists the kernels test: each needs its bit records
        const uint32_t v = Q.term[t] * L + f;
        if (s->h_probe_row[v] == BM_NO_PROBE_ROW && s->h_df[v] != 0) return SS_ENOTSUP;
      }
    }
  }
  SS_HIP(hipMemcpyAsync(d_sub, plan.sub.data(), (size_t)nq * sizeof(ss_bm25_query), hipMemcpyHostToDevice, st));
  SS_HIP(hipMemsetAsync(d_total, 0, (size_t)nq * 8, st));
  for (uint32_t i = 0; i < nq;) {  // runs of queries with / without a dense part: the bit-record pass, or an empty set to start from
    uint32_t j = i + 1;
    while (j < nq && plan.has_sub[j] == plan.has_sub[i]) j++;
    if (plan.has_sub[i]) {
      const int rc = ssi_bm25_match_bits(s, d_sub + i, d_bits + (size_t)i * n_groups, d_total + i, st, j - i);
      if (rc != SS_OK) return rc;
    } else {
      SS_HIP(hipMemsetAsync(d_bits + (size_t)i * n_groups, 0, (size_t)(j - i) * n_groups * 8, st));
    }
    i = j;
  }
  MtParams P{};
  P.q = d_q;
  P.sp_base = (const unsigned long long*)s->d_sp_base;
  P.sp_post = (const unsigned long long*)s->d_sp_post;
  P.probe = s->d_probe;
  P.probe_row = s->d_probe_row;
  P.del = s->n_deleted ? s->d_deleted : nullptr;
  P.del_words = (uint32_t)s->deleted_words;
  P.bits = d_bits;
  P.total = d_total;
  P.n_dense = n_dense;
  P.n_lists = L;
  P.n_fields = RF;
  P.n_groups = n_groups;
  P.n_rows = s->bm_probe_rows + 1u;
  P.n_docs = (uint32_t)std::min<uint64_t>(s->bm_n_docs, (uint64_t)n_groups * 64u);
  // a workgroup step takes MT_THREADS * MT_UNROLL postings: enough workgroups for the longest list in one step, at most 16 per query
  const uint32_t gx = (uint32_t)std::min<uint64_t>(16u, std::max<uint64_t>(1u, (longest + MT_THREADS * MT_UNROLL - 1) / (MT_THREADS * MT_UNROLL)));
  if (any_clear) mt_clear_kernel<<<dim3(gx, nq), MT_THREADS, 0, st>>>(P, nq);
  if (any_set) mt_set_kernel<<<dim3(gx, nq), MT_THREADS, 0, st>>>(P, nq);
  SS_HIP(hipGetLastError());
  return SS_OK;
}
