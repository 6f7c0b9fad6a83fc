// Internal to the C ABI layer (include/seekstorm_hip.h is the contract): what its files share.  Included by them only.
//   ss_api.hip        shard life, image uploads and commits, lexical search and its routing, match sets with sorts, facets and browse, the
//                     vector side, merge, profile hooks
//   api_coalesce.hip  the futex coalescer of concurrent callers, its SS_CO_TRACE report and its stats
//   api_deep.hip      deep pages: lexical and vector searches of more than SS_MAX_K results, in passes
// A function that one file defines and another calls is declared here, once, with its default arguments, under the ssi_ prefix and with
// C++ linkage (as in ss_common.h); everything else is static in its file.  The helpers defined here are static too: every file gets its
// own copy and the library exports none of them.
#pragma once
#include <algorithm>
#include <chrono>
#include <type_traits>

#include "ss_common.h"
#include "facet_commit.h"

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
struct QueryFacets;  // (the query_facets of a sorted search: ss_api.hip)
int ssi_bm25_search_sorted_locked(ss_shard* s, uint32_t nq, const ss_bm25_query* queries, uint32_t n_sorts, const ss_result_sort* sorts,
                                  const ss_sort_sources& src, uint32_t k, uint32_t n_filters, const ss_facet_filter* filters,
                                  uint32_t* out_doc, float* out_score, uint32_t* out_count, uint64_t* out_total, const QueryFacets* qf = nullptr);
int ssi_vec_search_host(ss_shard* s, uint32_t nq, const void* queries, size_t elem, const float* query_scale, uint32_t k,
                        float thr, const ss_ann_mode* mode, uint32_t* out_doc, float* out_score, uint32_t* out_count,
                        uint64_t* out_total, uint32_t* out_clusters, const float* query_norm = nullptr);
int ssi_vec_search_host_lists(ss_shard* s, uint32_t nq, const void* queries, size_t elem, const float* query_scale, uint32_t k,
                              float thr, const ss_ann_mode* mode, uint32_t* h_count, uint32_t** d_ncl_out,
                              const float* query_norm = nullptr, bool want_clusters = false, size_t out_slot = 0);
int ssi_vec_search_host_lane(ss_shard* s, uint32_t nq, const void* queries, size_t elem, const float* query_scale, uint32_t k, float thr,
                             uint32_t* out_doc, float* out_score, uint32_t* out_count, uint64_t* out_total);

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
// SS_CO_TRACE: where a coalesced batch spends its time.  _lane: a lexical lane batch's enqueue and device-wait times (ns);
// _report: what was collected, to stderr (ss_shard_destroy)
bool ssi_co_trace_on();
void ssi_co_trace_lane(uint64_t enqueue_ns, uint64_t wait_ns);
void ssi_co_trace_report();
static inline uint64_t co_now_us() { return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
