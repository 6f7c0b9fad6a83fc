// Internal to the C ABI layer (include/seekstorm_hip.h is the contract): what its files share.  Included by them only.
//   ss_api.hip        shard life, lexical search and its routing, match sets with sorts, facets and browse, the sharded searches, merge,
//                     profile hooks
//   api_vec.hip       the vector side: f32 and i8 images, their appends and side data, the host- and device-pointer searches
//   api_image.hip     the lexical and facet images built and committed: uploads, level and sparse-tier commits, tombstones, string ranks
//   api_coalesce.hip  the futex coalescer of concurrent callers, its SS_CO_TRACE report and its stats
//   api_deep.hip      deep pages: lexical and vector searches of more than SS_MAX_K results, in passes
//   api_delete.hip    delete_documents_by_query: match sets and pages of a batch into the tombstones (ss_bm25_delete_by_query)
//   ref_decode_dev.hip  index.bin opened level by level, its blocks decoded on the device (ss_bm25_open_index_bin_levels)
// A function that one file defines and another calls is declared here, once, with its default arguments, under the ssi_ prefix and with
// C++ linkage (as in ss_common.h); everything else is static in its file.  The helpers defined here are static too: every file gets its
// own copy and the library exports none of them.
#pragma once
#include <algorithm>
#include <chrono>
#include <type_traits>

#include "ss_common.h"
#include "facet_commit.h"
#include "bm25_match.h"

#define SS_TRY(x)          \
  do {                     \
    int _rc = (x);         \
    if (_rc) return _rc;   \
  } while (0)

// The shard's exclusion bitmap (d_deleted / deleted_words / n_deleted: its tombstones, as a rule) replaced by another one for the life
// of the object; n_deleted = 1 says "some doc may be excluded": the kernels take their filtered instantiations.  per_query() /
// vec_stride(): the bitmap is one of `words` words PER QUERY of the lexical / vector batch in flight; both flags are restored with the
// bitmap and otherwise left as they stand (0 outside such a batch: no guard nests inside one).  The caller holds the shard lock.
struct ExclSwap {
  ss_shard* s;
  uint32_t* del; uint64_t dw, nd; uint32_t pq, stride;
  ExclSwap(ss_shard* s_, uint32_t* bits, uint64_t words)
      : s(s_), del(s_->d_deleted), dw(s_->deleted_words), nd(s_->n_deleted), pq(s_->del_per_query), stride(s_->vec_del_stride) {
    s->d_deleted = bits; s->deleted_words = words; s->n_deleted = 1;
  }
  ExclSwap(const ExclSwap&) = delete;
  ~ExclSwap() { s->d_deleted = del; s->deleted_words = dw; s->n_deleted = nd; s->del_per_query = pq; s->vec_del_stride = stride; }
  void per_query() { s->del_per_query = 1; }
  void vec_stride(uint32_t words) { s->vec_del_stride = words; }
};

// Grow-only device workspace: *ptr holds at least `need` units (bytes behind a void*, elements else); a hipMalloc / hipFree pair per
// call would synchronise the device.  Growing waits for s->stream first -- work still queued may read the old block --, frees it and
// allocates `alloc` units (where a caller keeps slack against the next growth).  hipFree waits for the device anyway, so the explicit
// wait costs the call sites that had none nothing, and the steady state (need <= *cap) does not touch the device at all.  On
// failure *ptr = nullptr and *cap = 0.
template <typename T>
static int reserve(ss_shard* s, T** ptr, size_t* cap, size_t need, size_t alloc = 0) {
  if (need <= *cap) return SS_OK;
  alloc = std::max(alloc, need);
  SS_HIP(hipStreamSynchronize(s->stream));
  if (*ptr) (void)hipFree(*ptr);
  *ptr = nullptr;
  *cap = 0;
  SS_HIP(hipMalloc((void**)ptr, alloc * sizeof(std::conditional_t<std::is_void<T>::value, char, T>)));
  *cap = alloc;
  return SS_OK;
}

// device staging of host-pointer queries
static inline int ensure_qstage(ss_shard* s, size_t bytes) {
  return reserve(s, &s->d_qstage, &s->qstage_cap, bytes);
}
// the device lists of nq queries x k results (s->d_out_*)
static inline int ensure_out(ss_shard* s, size_t nq, size_t k) {
  size_t need = nq * std::max<size_t>(k, 1);
  if (need <= s->out_cap && nq <= s->q_cap) return SS_OK;
  void* ptrs[] = {s->d_out_doc, s->d_out_score, s->d_out_count, s->d_out_total};
  for (void* p : ptrs) if (p) (void)hipFree(p);
  s->d_out_doc = nullptr; s->d_out_score = nullptr; s->d_out_count = nullptr; s->d_out_total = nullptr;
  s->out_cap = 0; s->q_cap = 0;
  SS_HIP(hipMalloc(&s->d_out_doc, need * sizeof(uint32_t)));
  SS_HIP(hipMalloc(&s->d_out_score, need * sizeof(float)));
  SS_HIP(hipMalloc(&s->d_out_count, nq * sizeof(uint32_t)));
  SS_HIP(hipMalloc(&s->d_out_total, nq * sizeof(uint64_t)));
  s->out_cap = need; s->q_cap = nq;
  return SS_OK;
}

// The shard mutex, as everybody but the coalescer's lane path takes it: with the lane streams drained (ss_common.h lstream) -- whoever
// holds it may write the lexical image or enqueue writers on s->stream, and no lane kernel is in flight to meet them.
struct ShardLock {
  std::unique_lock<std::mutex> g;
  explicit ShardLock(ss_shard* s) : g(s->mu) {
    s->main_dirty = true;  // (whatever this section enqueues on s->stream: the next lane launch waits for it)
    if (s->lanes_inflight) {
      for (hipStream_t st : s->lstream)
        if (st) (void)hipStreamSynchronize(st);
      s->lanes_inflight = false;
    }
  }
};

// ---- ss_api.hip: the searches up to the device lists (s->d_out_*; the caller holds s->mu), the direct calls and the coalesced lanes
int ssi_bm25_search_host_queries(ss_shard* s, uint32_t nq, const ss_bm25_query* q, uint32_t kk, uint32_t rt, uint32_t n_filters,
                                 const ss_facet_filter* filters, bool filter_prebuilt = false);
int ssi_bm25_search_direct(ss_shard* s, uint32_t nq, const ss_bm25_query* q, uint32_t k, uint32_t rt, uint32_t n_filters,
                           const ss_facet_filter* filters, uint32_t* out_doc, float* out_score, uint32_t* out_count, uint64_t* out_total);
int ssi_bm25_search_direct_lane(ss_shard* s, uint32_t nq, const ss_bm25_query* q, uint32_t k, uint32_t rt, uint32_t* out_doc, float* out_score,
                                uint32_t* out_count, uint64_t* out_total, hipEvent_t ev, uint32_t lane_slot, std::vector<uint32_t>& row_of);
// A chunk of <= 64 queries planned for the MATCH-SET STEP (ss_api.hip: match_prepare / match_enqueue, where the contract stands): the
// tiers planned and the phrases in intersection form.  The staged forms are read by asynchronous copies: a MatchChunk lives until the
// call's synchronisation.
struct MatchChunk {
  BmTierPlan tier;
  std::vector<ss_bm25_query> staged;
  bool any_phrase() const { return !staged.empty(); }
  const ss_bm25_query* form(const ss_bm25_query* qc) const { return staged.empty() ? qc : staged.data(); }
};
// match_prepare without `info` (a union under a field filter is SS_ENOTSUP) and match_enqueue with the filter's bitmap built inside
int ssi_match_prepare(ss_shard* s, uint32_t nb, const ss_bm25_query* qc, MatchChunk* mc);
int ssi_match_enqueue(ss_shard* s, uint32_t nb, const ss_bm25_query* qc, const MatchChunk& mc, uint32_t n_filters, const ss_facet_filter* filters,
                      ss_bm25_query* d_q, ss_bm25_query* d_sub, ss_bm25_query* d_ph, unsigned long long* d_bits, unsigned long long* d_total);
int ssi_bm25_search_deep_filtered_locked(ss_shard* s, uint32_t nq, const ss_bm25_query* q, uint32_t k, uint32_t rt, uint32_t n_filters,
                                         const ss_facet_filter* filters, uint32_t* out_doc, float* out_score, uint32_t* out_count, uint64_t* out_total);
struct QueryFacets;  // (the query_facets of a sorted search: ss_api.hip)
// a batch whose queries each carry their OWN facet filters (ss_bm25_search_each): query i's are filters[filter_begin[i] .. filter_begin[i + 1]),
// checked by ssi_filter_rows (filter_rows.h) and free of SS_FACET_IDS_EXTERN sets
struct EachSets { const uint32_t* filter_begin; const ss_facet_filter* filters; };
int ssi_bm25_search_sorted_locked(ss_shard* s, uint32_t nq, const ss_bm25_query* queries, uint32_t n_sorts, const ss_result_sort* sorts,
                                  const ss_sort_sources& src, uint32_t k, uint32_t n_filters, const ss_facet_filter* filters,
                                  uint32_t* out_doc, float* out_score, uint32_t* out_count, uint64_t* out_total, const QueryFacets* qf = nullptr,
                                  const EachSets* each = nullptr);

// ---- api_vec.hip: the image released (ss_shard_destroy; the shard's streams are idle), the host-pointer search as one call, up to the
// device lists (the caller holds s->mu) and as a coalesced lane's pass
void ssi_vec_free(ss_shard* s);
int ssi_vec_search_host(ss_shard* s, uint32_t nq, const void* queries, size_t elem, const float* query_scale, uint32_t k,
                        float thr, const ss_ann_mode* mode, uint32_t* out_doc, float* out_score, uint32_t* out_count,
                        uint64_t* out_total, uint32_t* out_clusters, const float* query_norm = nullptr);
int ssi_vec_search_host_lists(ss_shard* s, uint32_t nq, const void* queries, size_t elem, const float* query_scale, uint32_t k,
                              float thr, const ss_ann_mode* mode, uint32_t* h_count, uint32_t** d_ncl_out,
                              const float* query_norm = nullptr, bool want_clusters = false, size_t out_slot = 0);
int ssi_vec_search_host_lane(ss_shard* s, uint32_t nq, const void* queries, size_t elem, const float* query_scale, uint32_t k, float thr,
                             uint32_t* out_doc, float* out_score, uint32_t* out_count, uint64_t* out_total);

// ---- api_image.hip: the lexical image released (ss_shard_destroy).  keep_tier: the dense image goes (a commit swaps in its successor),
// the sparse tier stays
void ssi_bm25_free(ss_shard* s, bool keep_tier = false);

// the positions of a level's postings as raw_level_upload (bm25_image.h) takes them, prepared on the host: what a commit with positions
// and the open level by level share
struct LevelPositions { std::vector<uint16_t> npos; std::vector<uint32_t> prel; std::vector<uint64_t> tpos; };
int ssi_level_positions_prepare(uint32_t n_terms, const uint64_t* offs, const uint16_t* tfs, const uint16_t* npos, const uint16_t* positions,
                                uint64_t n_positions, LevelPositions* out);
// levels + length bytes + the image built from them (+ a sparse tier that takes levels) become the shard's, in one lock section
struct ss_sparse_tier_built;  // sparse_levels.h
int ssi_bm25_install_levels(ss_shard* s, std::vector<ss_raw_level>& levels, std::vector<uint8_t>& doclen, ss_shard* img, ss_sparse_tier_built* tier,
                            double rebuild_ms, double open_ms);

// ... of an image of SEVERAL indexed fields: the levels become ssi_mf_levels(s)->raw, with their boosts (the caller holds commit_mu)
struct ss_raw_level_mf;  // bm25_image.h
int ssi_bm25_install_levels_fields(ss_shard* s, std::vector<ss_raw_level_mf>& levels, const std::vector<float>& boost, ss_shard* img, double rebuild_ms,
                                   double open_ms);

// ---- comm.hip: ssi_comm_exchange (ss_common.h) with the hybrid fusion on the host when host_fuse
int ssi_comm_exchange_hf(ss_comm* c, uint32_t nq, int n_lists, const ss_dev_list* L, const uint64_t* d_tot_a, const uint64_t* d_tot_b,
                         int local_rc, bool hybrid, uint32_t offset, uint32_t length, uint64_t* out_doc, float* out_score,
                         uint8_t* out_source, uint32_t* out_count, uint64_t* out_total, hipStream_t st, bool host_fuse);

// ---- api_deep.hip
int ssi_bm25_search_deep_locked(ss_shard* s, uint32_t nq, const ss_bm25_query* q, uint32_t k, uint32_t rt, uint32_t* out_doc, float* out_score,
                                uint32_t* out_count, uint64_t* out_total);
int ssi_vec_search_deep_locked(ss_shard* s, uint32_t nq, const void* queries, size_t elem, const float* query_scale, uint32_t k, float thr,
                               const ss_ann_mode* mode, uint32_t* out_doc, float* out_score, uint32_t* out_count, uint64_t* out_total,
                               uint32_t* out_clusters, const float* query_norm);
int ssi_bm25_search_sorted_deep_locked(ss_shard* s, uint32_t nq, const ss_bm25_query* queries, uint32_t n_sorts, const ss_result_sort* sorts,
                                       const ss_sort_sources& src, uint32_t k, uint32_t n_filters, const ss_facet_filter* filters,
                                       uint32_t* out_doc, float* out_score, uint32_t* out_count, uint64_t* out_total);

// ---- api_coalesce.hip
int ssi_co_submit(ss_shard* s, ss_coalescer& co, bool lexical, ss_co_req* me);
// A FACETED request (ss_bm25_search_filtered with filters, _facets, _sorted, _sorted_facets).  kind = the caller's entry (SS_CO_*), to run
// it alone; k_own / rt_own as the caller gave them.  Everything else is the request in ss_bm25_search_each's terms -- the base's k = 0 for
// SS_RT_COUNT, rt = SS_RT_TOPKCOUNT for ss_bm25_search_sorted, no sorts / no facets where the entry has none -- which is what a batch runs
// and what makes two requests compatible.  The pointers are the caller's; n_bounds / stride as QueryFacets counts them.
struct ss_co_fac_req : ss_co_req {
  uint32_t kind = 0, k_own = 0, rt_own = 0, n_sorts = 0, n_filters = 0, n_facets = 0;
  const ss_result_sort* sorts = nullptr;
  const ss_facet_filter* filters = nullptr;
  const uint32_t *facet_offset = nullptr, *facet_type = nullptr, *n_buckets = nullptr;
  const uint64_t* range_lower_bounds = nullptr;
  const ss_facet_point* bases = nullptr;
  size_t n_bounds = 0, stride = 0;
  uint64_t* out_facet_counts = nullptr;
};
enum { SS_CO_PLAIN = 0, SS_CO_FILTERED, SS_CO_FACETS, SS_CO_SORTED, SS_CO_SORTED_FACETS };
// What ss_shard_create allocates: the shard and, behind it, the state only the ABI layer knows -- the FACETED kind's coalescer, co_fac,
// next to co_lex and co_vec (one lane, batches of <= 64 through ss_bm25_search_each).  It stands here and not in ss_shard because
// ss_common.h is one of the kernel sources whose hash ties profiles/pmc_traffic.json to the tree (bench.py kernel_source_hash): host-only
// state must not move that hash.  Every ss_shard* that crosses the ABI came from ss_shard_create and is one of these; the scratch
// images the builders make with `new ss_shard` never reach an entry point.
// (the default batch: profiles/faceted_callers_time.json has the figures it follows)
#define SS_CO_FACETED_DEFAULT 64u
struct ss_shard_abi : ss_shard {
  ss_coalescer co_fac;
  void* d_delete_ws = nullptr;  // ss_bm25_delete_by_query's workspace (api_delete.hip), grow-only
  size_t delete_ws_cap = 0;
};
static inline ss_coalescer& ssi_co_fac(ss_shard* s) { return static_cast<ss_shard_abi*>(s)->co_fac; }
// the faceted kind.  *submitted = the call went through the coalescer and the return value is its answer; false -- the kind
// is off, the call is not one it takes (more than SS_CO_FACETED_MAX_REQUEST queries, a deep page, an SS_FACET_IDS_EXTERN filter, arguments the entry
// itself must judge) or this thread IS the coalescer running a request alone: the entry goes on as it always has
#define SS_CO_FACETED_MAX_REQUEST 16u
int ssi_co_fac_try(ss_shard* s, uint32_t kind, uint32_t nq, const ss_bm25_query* queries, uint32_t n_sorts, const ss_result_sort* sorts, uint32_t k, uint32_t rt,
                   uint32_t n_filters, const ss_facet_filter* filters, uint32_t n_facets, const uint32_t* facet_offset, const uint32_t* facet_type,
                   const uint32_t* n_buckets, const uint64_t* range_lower_bounds, const ss_facet_point* bases, uint32_t* out_doc, float* out_score,
                   uint32_t* out_count, uint64_t* out_total, uint64_t* out_facet_counts, bool* submitted);
// SS_CO_TRACE: where a coalesced batch spends its time.  _lane: a lexical lane batch's enqueue and device-wait times (ns);
// _report: what was collected, to stderr (ss_shard_destroy)
bool ssi_co_trace_on();
void ssi_co_trace_lane(uint64_t enqueue_ns, uint64_t wait_ns);
void ssi_co_trace_report();
static inline uint64_t co_now_us() { return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
