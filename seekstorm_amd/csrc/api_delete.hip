// C ABI, delete_documents_by_query (index.rs:5147-5205): the docs a lexical search selects become tombstones in one call
// (ss_bm25_delete_by_query; the contract stands in include/seekstorm_hip.h, the kernels in delete.hip).
//
// The call's state is a PENDING bitmap in workspace, zeroed per call, of the image's match-set width.  Three steps fill and use it:
//   1. per chunk of <= 64 queries the match-set step of the facet entries (ssi_match_prepare / ssi_match_enqueue) gives every query's
//      match set and its count, under the filter's exclusion bitmap.  A query whose page IS its match set has its row ORed into pending
//      (delete_collect_kernel); nothing else happens for it.  A chunk the step refuses (SS_ENOTSUP) is tried query by query; a query
//      it refuses alone is counted by the ordinary search (SS_RT_COUNT) and takes the page path.
//   2. every other query with something to select runs the search entries' locked internals with k = min(offset + length, matched);
//      the page comes home as they deliver it, goes up again and is scattered into pending (ssi_deleted_scatter on the u32 view).
//   Up to here the live tombstones were only READ: every match set and page is the shard's as the call found it.
//   3. delete_commit_kernel takes the tombstones off pending and counts what is left; the count is checked against doc_cap, the docs
//      are listed (ssi_browse_select, ascending), and only then the bitmap is grown as ss_add_deleted grows it and the same kernel
//      writes it.
#include <cstring>

#include "api_internal.h"
#include "browse.h"
#include "delete.h"
#include "filter_rows.h"

namespace {
struct DelWs {
  ss_bm25_query *d_q, *d_sub, *d_ph;
  unsigned long long *d_total, *d_bits, *d_pending, *d_count, *d_slice_begin;
  uint32_t *d_out_n, *d_slice_cnt;
  uint64_t groups;
};
struct DelCall {
  ss_shard* s;
  uint32_t n_sorts, n_filters;
  const ss_result_sort* sorts;
  const ss_facet_filter* filters;
  uint64_t offset, length;
  DelWs w;
  std::vector<uint64_t> matched;
  std::vector<uint8_t> known, whole;  // matched[i] is known from the match-set step; query i's page is its match set
};

// queries [0, nb) at qc (their slots in the call: c0 ..) through the match-set step; the rows that are whole pages into pending
int del_segment(DelCall& c, uint32_t c0, uint32_t nb, const ss_bm25_query* qc) {
  ss_shard* s = c.s;
  MatchChunk mc;
  const int rp = ssi_match_prepare(s, nb, qc, &mc);
  if (rp == SS_ENOTSUP) {
    if (nb == 1) return SS_OK;  // (known stays 0: the page path counts and answers it, or refuses it)
    for (uint32_t i = 0; i < nb; i++) SS_TRY(del_segment(c, c0 + i, 1, qc + i));
    return SS_OK;
  }
  SS_TRY(rp);
  const DelWs& w = c.w;
  SS_HIP(hipMemsetAsync(w.d_total, 0, (size_t)((char*)(w.d_bits + (size_t)nb * w.groups) - (char*)w.d_total), s->stream));
  int rc = ssi_match_enqueue(s, nb, qc, mc, c.n_filters, c.filters, w.d_q, w.d_sub, w.d_ph, w.d_bits, w.d_total);
  if (rc == SS_OK && hipMemcpyAsync(c.matched.data() + c0, w.d_total, (size_t)nb * 8, hipMemcpyDeviceToHost, s->stream) != hipSuccess) rc = SS_EDEVICE;
  if (hipStreamSynchronize(s->stream) != hipSuccess && rc == SS_OK) rc = SS_EDEVICE;  // (also on an error: mc's staged forms are being read)
  SS_TRY(rc);
  uint64_t mask = 0;
  for (uint32_t i = 0; i < nb; i++) {
    c.known[c0 + i] = 1;
    const bool all = c.offset == 0 && c.length >= c.matched[c0 + i] && !(qc[i].op & SS_OP_ALL_TERMS_FREQUENT);
    c.whole[c0 + i] = all ? 1 : 0;
    if (all && c.matched[c0 + i]) mask |= 1ull << i;
  }
  return ssi_delete_collect(w.d_pending, w.d_bits, w.groups, mask, s->stream);
}

// the page of ONE query: the search entry's list for k results, its entries from `offset` on into pending; *selected = their number
int del_page(DelCall& c, const ss_bm25_query* q, const ss_sort_sources& src, uint32_t k, uint64_t* selected) {
  ss_shard* s = c.s;
  std::vector<uint32_t> h_doc(k);
  std::vector<float> h_score(k);
  uint32_t cnt = 0;
  uint64_t tot = 0;
  if (c.n_sorts) {
    if (k <= SS_MAX_K) SS_TRY(ssi_bm25_search_sorted_locked(s, 1, q, c.n_sorts, c.sorts, src, k, c.n_filters, c.filters, h_doc.data(), h_score.data(), &cnt, &tot));
    else SS_TRY(ssi_bm25_search_sorted_deep_locked(s, 1, q, c.n_sorts, c.sorts, src, k, c.n_filters, c.filters, h_doc.data(), h_score.data(), &cnt, &tot));
  } else if (k <= SS_MAX_K) {
    SS_TRY(ssi_bm25_search_host_queries(s, 1, q, k, SS_RT_TOPKCOUNT, c.n_filters, c.filters));
    SS_HIP(hipMemcpyAsync(h_doc.data(), s->d_out_doc, (size_t)k * 4, hipMemcpyDeviceToHost, s->stream));
    SS_HIP(hipMemcpyAsync(&cnt, s->d_out_count, 4, hipMemcpyDeviceToHost, s->stream));
    SS_HIP(hipStreamSynchronize(s->stream));
  } else {
    SS_TRY(ssi_bm25_search_deep_filtered_locked(s, 1, q, k, SS_RT_TOPKCOUNT, c.n_filters, c.filters, h_doc.data(), h_score.data(), &cnt, &tot));
  }
  cnt = std::min(cnt, k);
  *selected = 0;
  if (cnt <= c.offset) return SS_OK;
  const uint32_t n = cnt - (uint32_t)c.offset;
  const uint32_t* ids = h_doc.data() + c.offset;
  for (uint32_t i = 0; i < n; i++)
    if (ids[i] >= s->bm_n_docs) return SS_EDEVICE;  // (the scatter trusts its ids: no doc of a list lies outside the image)
  SS_TRY(ensure_qstage(s, (size_t)n * 4));
  SS_HIP(hipMemcpyAsync(s->d_qstage, ids, (size_t)n * 4, hipMemcpyHostToDevice, s->stream));
  SS_HIP(hipMemsetAsync(c.w.d_count, 0, 8, s->stream));
  SS_TRY(ssi_deleted_scatter((uint32_t*)c.w.d_pending, (const uint32_t*)s->d_qstage, n, c.w.d_count, s->stream));
  SS_HIP(hipStreamSynchronize(s->stream));  // (h_doc is read by the copy)
  *selected = n;
  return SS_OK;
}
}  // namespace

extern "C" {

int ss_bm25_delete_by_query(ss_shard* s, uint32_t n_queries, const ss_bm25_query* queries, uint32_t n_sorts, const ss_result_sort* sorts,
                            uint64_t offset, uint64_t length, uint32_t n_filters, const ss_facet_filter* filters, uint32_t flags,
                            uint64_t* out_matched, uint64_t* out_selected, uint64_t* out_deleted, uint32_t* out_doc, uint64_t doc_cap) {
  if (out_deleted) *out_deleted = 0;
  if (!s || (n_queries && !queries)) return SS_EINVAL;
  if (flags & ~SS_DELETE_DRY_RUN) return SS_EINVAL;
  if ((n_sorts && !sorts) || (n_filters && !filters)) return SS_EINVAL;
  for (uint32_t i = 0; i < n_queries; i++) {
    if (out_matched) out_matched[i] = 0;
    if (out_selected) out_selected[i] = 0;
  }
  if (n_queries == 0) return SS_OK;
  if (n_sorts > SS_MAX_SORT_FIELDS) return SS_ENOTSUP;
  for (uint32_t f = 0; f < n_sorts; f++)
    if (sorts[f].facet_type > SS_FACET_POINT) return SS_EINVAL;
  const bool dry = (flags & SS_DELETE_DRY_RUN) != 0;
  ShardLock g(s);
  if (s->vstream) (void)hipStreamSynchronize(s->vstream);  // (a coalesced scan in flight reads what this call writes; none starts while mu is ours)
  SS_HIP(hipSetDevice(s->device));
  SS_HIP(hipStreamSynchronize(s->stream));
  ss_sort_sources src{};
  if (n_sorts) SS_TRY(ssi_sort_resolve(s, n_sorts, sorts, &src));  // SS_ENOTSUP: a string field without a rank table
  if (!s->d_post) return SS_ESTATE;
  if (n_sorts) {  // (what the sorted entry asks of the records, for the queries that never reach it too)
    if (!s->d_facets || s->facet_docs < s->bm_n_docs) return SS_ESTATE;
    for (uint32_t f = 0; f < n_sorts; f++)
      if ((uint64_t)sorts[f].facet_offset + ssi_facet_width(sorts[f].facet_type) > s->facet_record_size) return SS_ESTATE;
  }

  DelCall c{s, n_sorts, n_filters, sorts, filters, offset, length, {}, {}, {}, {}};
  c.matched.assign(n_queries, 0);
  c.known.assign(n_queries, 0);
  c.whole.assign(n_queries, 0);
  const uint64_t groups = (uint64_t)s->bm_n_sub * (BM_SUB / 64), n_slices = browse_slices(groups);
  const uint32_t CH = std::min<uint32_t>(n_queries, 64u);  // (tier plans are made for batches of <= 64, ssi_bm25_match_bits takes as many)
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t o_q = 0, o_sub = o_q + al((size_t)CH * sizeof(ss_bm25_query)), o_ph = o_sub + al((size_t)CH * sizeof(ss_bm25_query)),
               o_tot = o_ph + al((size_t)CH * sizeof(ss_bm25_query)), o_bits = o_tot + al((size_t)CH * 8), o_pend = o_bits + al((size_t)CH * groups * 8),
               o_cnt = o_pend + al((size_t)groups * 8), o_scnt = o_cnt + 256, o_sbeg = o_scnt + al((size_t)n_slices * 4),
               need = o_sbeg + al((size_t)n_slices * 8);
  ss_shard_abi* sa = static_cast<ss_shard_abi*>(s);
  SS_TRY(reserve(s, &sa->d_delete_ws, &sa->delete_ws_cap, need));
  char* W = (char*)sa->d_delete_ws;
  c.w = DelWs{(ss_bm25_query*)(W + o_q), (ss_bm25_query*)(W + o_sub), (ss_bm25_query*)(W + o_ph), (unsigned long long*)(W + o_tot),
              (unsigned long long*)(W + o_bits), (unsigned long long*)(W + o_pend), (unsigned long long*)(W + o_cnt),
              (unsigned long long*)(W + o_sbeg), (uint32_t*)(W + o_cnt + 8), (uint32_t*)(W + o_scnt), groups};
  SS_HIP(hipMemsetAsync(c.w.d_pending, 0, (size_t)groups * 8, s->stream));

  // 1. match sets, whole pages collected
  for (uint32_t c0 = 0; c0 < n_queries; c0 += CH) SS_TRY(del_segment(c, c0, std::min<uint32_t>(CH, n_queries - c0), queries + c0));
  // 2. pages
  std::vector<uint64_t> selected(n_queries, 0);
  for (uint32_t i = 0; i < n_queries; i++) {
    if (c.known[i] && c.whole[i]) { selected[i] = c.matched[i]; continue; }
    if (!c.known[i]) {  // the match-set step leaves the query to the searches: their count
      SS_TRY(ssi_bm25_search_host_queries(s, 1, queries + i, 0, SS_RT_COUNT, n_filters, filters));
      SS_HIP(hipMemcpyAsync(&c.matched[i], s->d_out_total, 8, hipMemcpyDeviceToHost, s->stream));
      SS_HIP(hipStreamSynchronize(s->stream));
    }
    if (length == 0 || offset >= c.matched[i]) continue;
    const uint64_t want = offset + length < offset ? ~0ull : offset + length;  // (the sum saturates)
    SS_TRY(del_page(c, queries + i, src, (uint32_t)std::min<uint64_t>(want, c.matched[i]), &selected[i]));
  }
  // 3. count, list, commit
  const uint64_t old_words = s->d_deleted ? s->deleted_words : 0;
  unsigned long long fresh = 0;
  SS_HIP(hipMemsetAsync(c.w.d_count, 0, 8, s->stream));
  SS_TRY(ssi_delete_commit((uint32_t*)c.w.d_pending, groups * 2, s->d_deleted, old_words, false, c.w.d_count, s->stream));
  SS_HIP(hipMemcpyAsync(&fresh, c.w.d_count, 8, hipMemcpyDeviceToHost, s->stream));
  SS_HIP(hipStreamSynchronize(s->stream));
  if (out_deleted) *out_deleted = fresh;
  if (out_doc && doc_cap < fresh) return SS_EINVAL;
  if (out_doc && fresh) {
    SS_TRY(ensure_qstage(s, (size_t)fresh * 4));
    SS_TRY(ssi_browse_select(s, c.w.d_pending, false, 0, fresh, c.w.d_slice_cnt, c.w.d_slice_begin, false, (uint32_t*)s->d_qstage, c.w.d_out_n, s->stream));
    SS_HIP(hipMemcpyAsync(out_doc, s->d_qstage, (size_t)fresh * 4, hipMemcpyDeviceToHost, s->stream));
    SS_HIP(hipStreamSynchronize(s->stream));
  }
  if (!dry && fresh) {
    // every fresh doc lies below bm_n_docs: a bitmap that covers the image has their words; a shorter one (or none) grows as
    // ss_add_deleted grows it, to cover every doc of the images
    uint64_t words = old_words;
    uint32_t* grown = nullptr;
    if (old_words < ((uint64_t)s->bm_n_docs + 31) / 32) {
      const uint64_t docs = std::max<uint64_t>(std::max<uint64_t>(s->bm_n_docs, s->facet_docs), s->n_rows);
      words = (docs + 31) / 32;
      SS_HIP(hipMalloc((void**)&grown, (size_t)words * 4));
      if ((old_words && hipMemcpyAsync(grown, s->d_deleted, (size_t)old_words * 4, hipMemcpyDeviceToDevice, s->stream) != hipSuccess) ||
          hipMemsetAsync(grown + old_words, 0, (size_t)(words - old_words) * 4, s->stream) != hipSuccess) {
        (void)hipStreamSynchronize(s->stream);
        (void)hipFree(grown);
        return SS_EDEVICE;
      }
    }
    // (Without growth the kernel writes the live bitmap: should the wait below fail, bits stand that n_deleted does not count -- harmless
    // for the reason given in ss_add_deleted.)
    int rc = hipMemsetAsync(c.w.d_count, 0, 8, s->stream) == hipSuccess ? SS_OK : SS_EDEVICE;
    if (rc == SS_OK) rc = ssi_delete_commit((uint32_t*)c.w.d_pending, groups * 2, grown ? grown : s->d_deleted, words, true, c.w.d_count, s->stream);
    if (hipStreamSynchronize(s->stream) != hipSuccess && rc == SS_OK) rc = SS_EDEVICE;
    if (rc != SS_OK) {
      if (grown) (void)hipFree(grown);
      return rc;
    }
    if (grown) {
      if (s->d_deleted) (void)hipFree(s->d_deleted);
      s->d_deleted = grown;
    }
    s->deleted_words = words;
    s->n_deleted = (old_words ? s->n_deleted : 0) + fresh;
  }
  for (uint32_t i = 0; i < n_queries; i++) {
    if (out_matched) out_matched[i] = c.matched[i];
    if (out_selected) out_selected[i] = selected[i];
  }
  return SS_OK;
}

}  // extern "C"
