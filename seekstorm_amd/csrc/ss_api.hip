// C ABI of the MI355X-native SeekStorm query hot path (see include/seekstorm_hip.h for the contract and the
// reference seams each entry point replaces): shard life, lexical search and its routing, match sets with sorts, facets and browse, the
// sharded searches, merge and the profile hooks.  Host-side plumbing only; the kernels live in bm25*.hip.
// The vector side stands in api_vec.hip, the lexical and facet images (uploads and commits) in api_image.hip, the coalescer of concurrent
// callers in api_coalesce.hip, the deep pages in api_deep.hip, delete_documents_by_query in api_delete.hip; api_internal.h is what they share.
#include <sched.h>
#include <time.h>
#include <unistd.h>

#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <new>
#include <type_traits>
#include <unordered_map>

#include "ss_common.h"
#include "facet_point.h"
#include "bm25_image.h"
#include "bm25_match.h"
#include "bm25_pack.h"
#include "browse.h"
#include "facet_commit.h"
#include "api_internal.h"

namespace {
// runs `search` with the shard's tombstone bitmap replaced by the filter's exclusion bitmap (built on `st` first; `prebuilt`: the caller
// has built THESE filters' bitmap on `st` already and nothing has written d_filter_bits since -- ss_bm25_search_facets builds it once)
template <typename F>
int with_facet_filter(ss_shard* s, uint32_t n_filters, const ss_facet_filter* filters, hipStream_t st, F search, bool prebuilt = false) {
  if (n_filters == 0) return search();
  if (!s->d_facets || s->facet_docs < s->bm_n_docs) return SS_ESTATE;  // a record for every doc of the lexical image
  int rc = prebuilt ? SS_OK : ssi_facet_build(s, n_filters, filters, st);
  if (rc) return rc;
  ExclSwap sw(s, s->d_filter_bits, (s->facet_docs + 31) / 32);
  return search();
}
}  // namespace

extern "C" {

int ss_abi_version(void) { return SS_ABI_VERSION; }

const char* ss_strerror(int code) {
  switch (code) {
    case SS_OK: return "ok";
    case SS_EINVAL: return "invalid argument";
    case SS_ENOMEM: return "out of memory";
    case SS_EDEVICE: return "HIP device/runtime error";
    case SS_ENOTSUP: return "not answered by the device path: the caller's own (CPU) path applies (INTEGRATION.md section 4)";
    case SS_ESTATE: return "image not uploaded";
    case SS_EPEER: return "a collective search failed on another rank";
    default: return "unknown error";
  }
}

int ss_device_count(int* out) {
  if (!out) return SS_EINVAL;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) { *out = 0; return SS_EDEVICE; }
  *out = n;
  return SS_OK;
}

int ss_shard_create(int device, ss_shard** out) {
  if (!out) return SS_EINVAL;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return SS_EDEVICE;  // fail loudly: no CPU fallback exists
  if (device < 0 || device >= n) return SS_EINVAL;
  SS_HIP(hipSetDevice(device));
  ss_shard_abi* s = new (std::nothrow) ss_shard_abi();  // (api_internal.h: the shard and the ABI layer's own state behind it)
  if (!s) return SS_ENOMEM;
  s->device = device;
  s->co_lex.max_batch = 1024;
  s->co_vec.max_batch = SS_VEC_BATCH;
  s->co_fac.max_batch = SS_CO_FACETED_DEFAULT;
  // Lexical batches in flight: ONE, and a second lane while ~96 or more callers seem to be around (adaptive; SS_COALESCE_LANES=1 / 2 force
  // one / two, =autoN moves the threshold).  History: two unconditional lanes halve the batches, and the device's fixed cost per batch is
  // what bounds small ones (round 4: T = 8 54 K -> 25 K q/s; profiles/r4k_lanes.log); opening the lane from ~32 callers on gained 7 % at
  // T = 64 and cost hybrid callers their tail (round 5, profiles/r5_lanes.log) -- while the followers' 30 us spin still ate the box's CPU
  // quota.  Round 6, spin gone, hybrid tail fixed elsewhere: one lane against the adaptive form at a threshold of 96 -- T = 64 equal
  // (300 - 330 K q/s), T = 128 336 - 356 K -> 535 K, T = 192 419 - 448 K -> 550 - 604 K, T = 256 404 - 425 K -> 508 - 511 K (p99 0.56 -
  // 0.64 ms), T = 512 534 - 600 K -> 615 K; below the threshold nothing changes; a threshold of 48 halves the batches of 64 callers
  // for nothing (profiles/r6_lanes_from.log, r6_lanes_small.log).
  // Round 6, later: all of the above was measured with both lanes feeding the shard's ONE stream -- their kernels ran one behind the other,
  // and a second lane could only overlap host work with device work.  Each lane's one-launch kernels now run on a stream of the lane's own
  // (ss_common.h lstream; bm25_small_try): two batches of ~22 callers overlap ON THE DEVICE, and the threshold is 32 -- T = 64 300 - 330 K ->
  // 430 - 454 K q/s (p50 210 -> 142 us, p99 290 -> 195 us), T = 96 -> 490 - 500 K, T = 128 535 -> 570 - 720 K, T = 192 -> 570 - 620 K, T = 256 /
  // 512 unchanged (500 / 600 K: batches of 48 queries or more fill the chip alone and share lane 0's stream), T = 8 91 -> 100 - 110 K;
  // hybrid and vector callers unchanged (profiles/r6_lane_streams*.log).
  {
    const char* e = getenv("SS_COALESCE_LANES");
    const bool one = e && atoi(e) == 1, two = e && atoi(e) == 2, adaptive = !one && !two;
    s->co_lex.n_lanes = one ? 1u : 2u;
    s->co_lex.lanes_forced = two;
    if (adaptive && e && strncmp(e, "auto", 4) == 0 && e[4]) s->co_lex.lanes_from = (uint32_t)std::max(2, atoi(e + 4));
  }
  // the shard's stream carries the latency-bound work (lexical searches: tens of microseconds a launch) at the device's HIGHEST priority;
  // the coalesced vector scans (milliseconds a pass) run on vstream at the lowest: a lexical kernel that arrives during a scan is
  // dispatched as the scan's workgroups retire instead of waiting for the pass to end
  int pr_least = 0, pr_greatest = 0;
  (void)hipDeviceGetStreamPriorityRange(&pr_least, &pr_greatest);
  if (hipStreamCreateWithPriority(&s->stream, hipStreamNonBlocking, pr_greatest) != hipSuccess) { delete s; return SS_EDEVICE; }
  if (hipStreamCreateWithPriority(&s->vstream, hipStreamNonBlocking, pr_least) != hipSuccess) { (void)hipStreamDestroy(s->stream); delete s; return SS_EDEVICE; }
  *out = s;
  return SS_OK;
}

int ss_shard_destroy(ss_shard* s) {
  if (!s) return SS_EINVAL;
  ssi_co_trace_report();
  (void)hipSetDevice(s->device);
  (void)hipStreamSynchronize(s->stream);
  if (s->vstream) (void)hipStreamSynchronize(s->vstream);
  for (hipStream_t st : s->lstream)
    if (st) (void)hipStreamSynchronize(st);
  ssi_vec_free(s);
  ssi_bm25_free(s);
  ssi_mf_levels_drop(s);
  ssi_facet_side_drop(s);
  for (void* p_ : {(void*)s->d_vq, (void*)s->d_vdoc, (void*)s->d_vscore, (void*)s->d_vcount, (void*)s->d_vtotal}) if (p_) (void)hipFree(p_);
  if (static_cast<ss_shard_abi*>(s)->d_delete_ws) (void)hipFree(static_cast<ss_shard_abi*>(s)->d_delete_ws);
  void* ptrs[] = {s->d_qstage, s->d_out_doc, s->d_out_score, s->d_out_count, s->d_out_total, s->d_bq, s->d_deleted, s->d_facets, s->d_filter_bits, s->d_facet_ws, s->d_pool_stage, s->d_tier_ws, s->d_tier_hold, s->d_excl_bits, s->d_sort_ws, s->d_route_ws, s->d_peel_bits, s->d_gate_ws};
  for (void* p : ptrs) if (p) (void)hipFree(p);
  (void)hipDeviceSynchronize();  // searches queued on the callers' own streams may still use their workspaces
  for (auto& kv : s->bm_ws) {
    if (kv.second.d_vq) (void)hipFree(kv.second.d_vq);
    if (kv.second.d_part) (void)hipFree(kv.second.d_part);
  }
  for (int kx = 0; kx < 2; kx++)
    for (auto& pr : s->prof.pending[kx]) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
  for (ss_coalescer* co : {&s->co_lex, &s->co_vec})
    for (auto& ln : co->lane) {
      if (ln.h_pin) (void)hipHostFree(ln.h_pin);
      if (ln.ev) (void)hipEventDestroy(ln.ev);
    }
  if (s->h_bq) (void)hipHostFree(s->h_bq);
  if (s->bq_ev) (void)hipEventDestroy(s->bq_ev);
  if (s->d_small_ws) (void)hipFree(s->d_small_ws);
  for (int i = 0; i < 2; i++) {
    if (s->lstream[i]) { (void)hipStreamSynchronize(s->lstream[i]); (void)hipStreamDestroy(s->lstream[i]); }
    if (s->d_small_ws_l[i]) (void)hipFree(s->d_small_ws_l[i]);
  }
  if (s->ev_main) (void)hipEventDestroy(s->ev_main);
  if (s->h_small) (void)hipHostFree(s->h_small);
  if (s->h_ans) (void)hipHostFree(s->h_ans);
  if (s->d_ans_done) (void)hipFree(s->d_ans_done);
  (void)hipStreamDestroy(s->stream);
  if (s->vev) (void)hipEventDestroy(s->vev);
  if (s->vstream) (void)hipStreamDestroy(s->vstream);
  delete static_cast<ss_shard_abi*>(s);
  return SS_OK;
}

int ss_shard_sync(ss_shard* s) {
  if (!s) return SS_EINVAL;
  SS_HIP(hipSetDevice(s->device));
  SS_HIP(hipStreamSynchronize(s->stream));
  if (s->vstream) SS_HIP(hipStreamSynchronize(s->vstream));
  for (hipStream_t st : s->lstream)
    if (st) SS_HIP(hipStreamSynchronize(st));
  return SS_OK;
}

// What the pass over a batch that is about to be uploaded collects besides its verdict (ssi_bm25_search_host_queries): the batch in the packed
// form (bm25_pack.h; given up when a phrase query turns up -- those need phrase_seq / phrase_len), and the postings its scored terms
// name in all (the pruned kernel's partition rule, ss_common.h bm_batch_postings).
struct bm_batch_sink {
  bm_packer pack;
  const std::vector<uint64_t>* df = nullptr;  // postings per public term
  uint64_t postings = 0;
};

// nt_max: largest n_terms + NOT terms of the batch (what the scan kernels are specialised on); np_max: largest n_terms
// any_filter: some query carries a field filter (on an image with merged lists the others read one list per term)
// sink: filled with every query that passed, in the same pass
static int check_queries(const ss_shard* s, uint32_t nq, const ss_bm25_query* q, bool* has_and, bool* has_or, uint32_t* nt_max,
                         uint32_t* np_max, bool* all_probed, bool* any_frequent, bool* phrase = nullptr, bool* any_filter = nullptr,
                         bool* uniform = nullptr, bool* gated = nullptr, uint32_t* nn_max = nullptr, bm_batch_sink* sink = nullptr) {
  uint32_t n_phrase = 0, np_min = 0xFFFFFFFFu, most_not = 0;
  bool some_gated = false;
  const uint32_t L = s->bm_n_fields, RF = bm_real_fields(s);  // lists per term, indexed fields
  bool some_filter = false;
  *any_frequent = false;
  *all_probed = s->bm_probe_rows != 0;
  *has_and = false;
  *has_or = false;
  *nt_max = 0;
  *np_max = 0;
  bool any_not = false;
  for (uint32_t i = 0; i < nq; i++) {
    const uint32_t op = bm_q_op(q[i].op), n_not = bm_q_nnot(q[i].op), all = q[i].n_terms + n_not;
    if (q[i].n_terms == 0 || all > SS_MAX_QUERY_TERMS) return SS_EINVAL;
    if (op != SS_OP_INTERSECTION && op != SS_OP_UNION && op != SS_OP_PHRASE) return SS_EINVAL;
    if (op == SS_OP_PHRASE) {  // QueryType::Phrase: unique terms + the words in order (non_unique_query_list)
      if (!phrase) return SS_ENOTSUP;
      if (q[i].phrase_len < 2 || q[i].phrase_len > SS_MAX_PHRASE) return SS_EINVAL;
      // every place names a unique term, or SS_PHRASE_SKIP: a place inside an n-gram key, whose entry stands at the key's first word
      // (the key's other component terms are scored with the rest, they are no words of the phrase)
      if (q[i].phrase_seq[0] >= q[i].n_terms) return SS_EINVAL;
      for (uint32_t j = 1; j < q[i].phrase_len; j++)
        if (q[i].phrase_seq[j] >= q[i].n_terms && q[i].phrase_seq[j] != SS_PHRASE_SKIP) return SS_EINVAL;
      if (q[i].n_terms > 6) return SS_ENOTSUP;  // (NOT terms: their lists are probed by the phrase kernel like everywhere else)
      // several indexed fields: over the merged lists and their field-tagged positions (a corpus whose boosts kept the merged
      // lists from being built has no phrase path)
      if (s->bm_n_fields > 1 && !s->bm_merged) return SS_ENOTSUP;
      if (s->bm_n_fields > 1 ? !s->d_pos32 : !s->d_pos) return SS_ESTATE;  // the image carries no positions (ss_bm25_upload[_fields]_positions)
      n_phrase++;
    }
    // field_filter: bits of indexed fields; an image with one indexed field has nothing to filter (the reference's set then
    // holds that field or nothing, search.rs:2483-2492).  Unions of several terms: the reference applies the filter inside
    // union_docid_3's sub-queries, not per doc -- not offered.
    if (bm_q_field_filter(q[i].op) >> RF) return SS_EINVAL;  // a field the image does not have
    const uint32_t filt = RF > 1 ? bm_q_field_filter(q[i].op) : 0u;
    if (filt && op == SS_OP_UNION && q[i].n_terms > 1) {  // a union under a field filter: per-term gating in the scan kernels (BM_AND_GATED)
      if (q[i].n_terms > 7 || !gated) return SS_ENOTSUP;
      some_gated = true;
    }
    some_filter |= filt != 0u && op != SS_OP_PHRASE;  // (a phrase's filter is a test on its positions: no (term, field) lists)
    const bool use_merged = s->bm_merged && (!filt || op == SS_OP_PHRASE);  // this query reads the merged lists: one list per term
    const uint32_t eff_fields = use_merged ? 1u : RF, f_begin = use_merged ? L - 1u : 0u, f_end = use_merged ? L : RF;
    // all_terms_frequent: an intersection of 2..7 terms over one indexed field (the mark takes bit 7 of the match byte);
    // on anything else the reference's flag has no effect we model (single terms, unions) or is not offered
    // (several indexed fields: over the merged lists, whose codes carry the multi-field form of the per-posting rule; under a field
    // filter the reference switches the shortcut off -- add_result.rs:3116 "all_terms_frequent && field_filter_set.is_empty()" --
    // and so does the expansion)
    if (bm_q_all_frequent(q[i].op) && op == SS_OP_INTERSECTION && q[i].n_terms > 1 && !filt) {
      if (q[i].n_terms > 7 || (L > 1 && !s->bm_merged)) return SS_ENOTSUP;
      *any_frequent = true;
    }
    if (eff_fields > 1) {  // (term, field) posting lists: at most BM_MAX_VTERMS of them, match masks of 8 bits
      if (all * eff_fields > (uint32_t)BM_MAX_VTERMS) return SS_ENOTSUP;
      if (op == SS_OP_INTERSECTION && q[i].n_terms > 8) return SS_ENOTSUP;
    }
    for (uint32_t t = 0; t < all; t++) {
      if (q[i].term[t] >= s->bm_n_terms / L) return SS_EINVAL;
      if (*all_probed && s->bm_probe_rows < s->bm_n_terms)  // rows were rationed: does every list this query reads have one?
        for (uint32_t f = f_begin; f < f_end; f++) {
          const uint32_t v = q[i].term[t] * L + f;
          if (s->h_probe_row[v] == BM_NO_PROBE_ROW && s->h_df[v] != 0) *all_probed = false;
        }
      if (t < q[i].n_terms && !(q[i].idf[t] > 0.0f)) return SS_EINVAL;
      for (uint32_t u = 0; u < t; u++)
        if (q[i].term[u] == q[i].term[t]) return SS_EINVAL;  // unique terms only (search.rs:3023 unique_terms)
    }
    if (((op == SS_OP_INTERSECTION || op == SS_OP_PHRASE) && q[i].n_terms > 1) || filt) *has_and = true;
    else if (q[i].n_terms > 1) *has_or = true;  // a single-term query is both: its exact count is its posting count
    *nt_max = std::max(*nt_max, all);
    *np_max = std::max(*np_max, q[i].n_terms);
    np_min = std::min(np_min, q[i].n_terms);
    any_not |= n_not != 0;
    most_not = std::max(most_not, n_not);
    if (sink) {
      if (op == SS_OP_PHRASE) sink->pack.give_up();
      else sink->pack.add(q[i], all);
      for (uint32_t t = 0; t < q[i].n_terms; t++)
        if (q[i].term[t] < sink->df->size()) sink->postings += (*sink->df)[q[i].term[t]];
    }
  }
  if (nn_max) *nn_max = most_not;  // the most NOT terms any query of the batch has (nt_max - np_max says only that there are some)
  if (uniform) *uniform = np_min == *np_max;  // every query with the same number of terms
  if (gated) *gated = some_gated;
  // "the batch holds NOT terms" travels as nt_max > np_max (the kernels' filtered variants are chosen by it): keep that true
  // when the query with the NOT terms is not the one with the most terms
  if (any_not && *nt_max == *np_max) *nt_max = *np_max + 1;
  if (n_phrase && n_phrase != nq) return SS_ENOTSUP;  // a batch holds phrase queries only
  if (phrase) *phrase = n_phrase != 0;
  if (any_filter) *any_filter = some_filter;
  return SS_OK;
}

int ss_bm25_search(ss_shard* s, uint32_t nq, const ss_bm25_query* q, uint32_t k, uint32_t rt, uint32_t* out_doc,
                   float* out_score, uint32_t* out_count, uint64_t* out_total) {
  return ss_bm25_search_filtered(s, nq, q, k, rt, 0, nullptr, out_doc, out_score, out_count, out_total);
}

// rows of a batch that ran in another order back to the callers' order: row i of the src arrays -> row perm[i] of the dst arrays
__global__ void bm25_unpermute_kernel(const uint32_t* __restrict__ perm, uint32_t nq, uint32_t kk, const uint32_t* __restrict__ src_doc,
                                      const float* __restrict__ src_score, const uint32_t* __restrict__ src_count,
                                      const unsigned long long* __restrict__ src_total, uint32_t* __restrict__ dst_doc,
                                      float* __restrict__ dst_score, uint32_t* __restrict__ dst_count, unsigned long long* __restrict__ dst_total) {
  const uint32_t i = blockIdx.x;
  if (i >= nq) return;
  const uint32_t o = perm[i];
  for (uint32_t j = threadIdx.x; j < kk; j += blockDim.x) {
    dst_doc[(size_t)o * kk + j] = src_doc[(size_t)i * kk + j];
    dst_score[(size_t)o * kk + j] = src_score[(size_t)i * kk + j];
  }
  if (threadIdx.x == 0) {
    dst_count[o] = src_count[i];
    dst_total[o] = src_total[i];
  }
}

// ---- probe rows on demand.  A rationed vocabulary keeps a pool of rows (alloc_probe); before a host-pointer batch runs, the
// row-less lists it touches get pool rows -- least recently used rows first, never one this batch needs -- built from the
// list's own postings: one wave per (list, sub-block) ORs the doc bits of the segment into 64 group masks and writes them
// with the rank of each group's first posting (what the image builders write for the fixed rows).  A row costs its own
// bytes once (1.9 MB at 10 M docs) and nothing while it stays in the pool; lists that found no row leave their queries to
// the scan kernels as before.
__global__ void probe_row_evict_kernel(const uint32_t* __restrict__ lists, uint32_t n, uint32_t* __restrict__ probe_row) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) probe_row[lists[i]] = BM_NO_PROBE_ROW;
}
__global__ void probe_row_fill_kernel(const uint32_t* __restrict__ pairs /* (list, row) */, uint32_t n_pairs, uint32_t n_sub,
                                      const uint32_t* __restrict__ sub_off, const unsigned long long* __restrict__ term_base,
                                      const uint32_t* __restrict__ post, uint2* __restrict__ probe, uint32_t* __restrict__ probe_z,
                                      uint32_t* __restrict__ probe_row) {
  __shared__ unsigned long long masks[4][BM_SUB / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long gw = (unsigned long long)blockIdx.x * 4u + (unsigned)w;
  if (gw >= (unsigned long long)n_pairs * n_sub) return;
  const uint32_t pair = (uint32_t)(gw / n_sub), sb = (uint32_t)(gw % n_sub);
  const uint32_t t = pairs[2 * pair], r = pairs[2 * pair + 1];
  const uint32_t u0 = sub_off[(size_t)t * (n_sub + 1) + sb], u1 = sub_off[(size_t)t * (n_sub + 1) + sb + 1];
  const unsigned long long base = (term_base[t] + u0) * 4ull;
  masks[w][lane] = 0ull;
  __builtin_amdgcn_wave_barrier();
  for (uint32_t i = (uint32_t)lane; i < (u1 - u0) * 4u; i += 64u) {
    const uint32_t p = post[base + i];
    if (p) {  // 0 = the segment's NULL padding
      const uint32_t d = bm_doc_field(p) - 1u;
      atomicOr(&masks[w][d >> 6], 1ull << (d & 63u));
    }
  }
  __builtin_amdgcn_wave_barrier();
  const unsigned long long m = masks[w][lane];
  uint32_t run = (uint32_t)__popcll(m);  // exclusive prefix over the 64 groups
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t v = __shfl_up(run, o);
    if (lane >= o) run += v;
  }
  run -= (uint32_t)__popcll(m);
  const size_t gi = ((size_t)r * n_sub + sb) * (BM_SUB / 64) + (uint32_t)lane;
  probe[gi] = make_uint2((uint32_t)m, (uint32_t)(m >> 32));
  probe_z[gi] = u0 * 4u + run;
  if (sb == 0 && lane == 0) probe_row[t] = r;
}

// the FIXED probe rows of a host-built image, from the image itself (ssi_bm25_build_from_host_merged): the rows used to be assembled on
// the host and copied -- 188 KB per list and million docs, 4.5 GB for the 23 760 lists of a 1 M-doc 3-field index: 1.0 s of zeroing
// and bit setting + 0.45 s of pageable copies, against a pass over the uploaded postings here
extern "C++" int ssi_bm25_fill_fixed_probe_rows(ss_shard* s, hipStream_t st) {
  if (!s->d_probe || !s->bm_probe_rows) return SS_OK;
  std::vector<uint32_t> pairs;
  for (uint32_t t = 0; t < s->bm_n_terms; t++)
    // (an EMPTY list may own a row as well -- alloc_probe deals rows before it points the row-less empty lists at the zero row: built too, as zeros)
    if (s->h_probe_row[t] != BM_NO_PROBE_ROW && s->h_probe_row[t] < s->bm_probe_rows) { pairs.push_back(t); pairs.push_back(s->h_probe_row[t]); }
  const uint32_t n = (uint32_t)(pairs.size() / 2);
  if (!n) return SS_OK;
  uint32_t* d_pairs = nullptr;
  SS_HIP(hipMalloc(&d_pairs, pairs.size() * sizeof(uint32_t)));
  int rc = hipMemcpyAsync(d_pairs, pairs.data(), pairs.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st) == hipSuccess ? SS_OK : SS_EDEVICE;
  if (rc == SS_OK) {
    const unsigned long long waves = (unsigned long long)n * s->bm_n_sub;
    probe_row_fill_kernel<<<(unsigned)((waves + 3) / 4), 256, 0, st>>>(d_pairs, n, s->bm_n_sub, s->d_sub_off, (const unsigned long long*)s->d_term_base,
                                                                     s->d_post, s->d_probe, s->d_probe_z, s->d_probe_row);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) rc = SS_EDEVICE;
  }
  (void)hipFree(d_pairs);
  return rc;
}

// the lists of a term that a query reads: the merged list alone without a field filter (bm_merged images), else the fields'
static inline void query_list_range(const ss_shard* s, const ss_bm25_query& q, uint32_t* f_begin, uint32_t* f_end) {
  const uint32_t L = s->bm_n_fields, RF = bm_real_fields(s);
  const bool use_merged = s->bm_merged && (!(RF > 1 && bm_q_field_filter(q.op)) || bm_q_op(q.op) == SS_OP_PHRASE);  // (a phrase always reads the merged lists)
  *f_begin = use_merged ? L - 1u : 0u;
  *f_end = use_merged ? L : RF;
}
static inline bool list_needs_row(const ss_shard* s, uint32_t v) { return s->h_probe_row[v] == BM_NO_PROBE_ROW && s->h_df[v] != 0; }

// caller holds s->mu (with or without the lane streams drained: see below)
static int ssi_bm25_ensure_probe_rows(ss_shard* s, uint32_t nq, const ss_bm25_query* q, hipStream_t st) {
  if (s->probe_pool_rows == 0 || !s->d_probe) return SS_OK;
  const uint32_t n_lists_per_term = s->bm_n_fields, n_public = s->bm_n_terms / s->bm_n_fields;
  const uint64_t now = ++s->pool_clock;
  // phrase queries first: without rows for all of their lists they have no kernel at all (the others fall back to the scans)
  std::vector<uint32_t> missing, missing_phrase;
  for (uint32_t i = 0; i < nq; i++) {
    const bool is_phrase = bm_q_op(q[i].op) == SS_OP_PHRASE;
    const uint32_t all = std::min<uint32_t>(q[i].n_terms + bm_q_nnot(q[i].op), SS_MAX_QUERY_TERMS);
    uint32_t f_begin, f_end;
    query_list_range(s, q[i], &f_begin, &f_end);
    for (uint32_t t = 0; t < all; t++) {
      if (q[i].term[t] >= n_public) continue;  // check_queries reports it
      for (uint32_t f = f_begin; f < f_end; f++) {
        const uint32_t v = q[i].term[t] * n_lists_per_term + f, r = s->h_probe_row[v];
        if (r != BM_NO_PROBE_ROW && r >= s->probe_pool_begin && r < s->probe_pool_begin + s->probe_pool_rows)
          s->pool_tick[r - s->probe_pool_begin] = now;  // a pool row this batch needs: not a victim
        else if (list_needs_row(s, v))
          (is_phrase ? missing_phrase : missing).push_back(v);
      }
    }
  }
  if (missing.empty() && missing_phrase.empty()) return SS_OK;
  std::sort(missing_phrase.begin(), missing_phrase.end());
  missing_phrase.erase(std::unique(missing_phrase.begin(), missing_phrase.end()), missing_phrase.end());
  std::sort(missing.begin(), missing.end());
  missing.erase(std::unique(missing.begin(), missing.end()), missing.end());
  {
    std::vector<uint32_t> rest;
    std::set_difference(missing.begin(), missing.end(), missing_phrase.begin(), missing_phrase.end(), std::back_inserter(rest));
    missing = missing_phrase;
    missing.insert(missing.end(), rest.begin(), rest.end());
  }
  // victims: free rows first, then the least recently used ones, never a row of this batch
  std::vector<uint32_t> victims;
  for (uint32_t i = 0; i < s->probe_pool_rows; i++)
    if (s->pool_tick[i] != now) victims.push_back(i);
  std::sort(victims.begin(), victims.end(), [&](uint32_t a, uint32_t b) {
    const bool fa = s->pool_list[a] == BM_NO_PROBE_ROW, fb = s->pool_list[b] == BM_NO_PROBE_ROW;
    if (fa != fb) return fa;
    return s->pool_tick[a] != s->pool_tick[b] ? s->pool_tick[a] < s->pool_tick[b] : a < b;
  });
  const uint32_t n = (uint32_t)std::min(missing.size(), victims.size());
  if (n == 0) return SS_OK;
  std::vector<uint32_t> stage;  // [evicted lists | (list, row) pairs]
  for (uint32_t i = 0; i < n; i++)
    if (s->pool_list[victims[i]] != BM_NO_PROBE_ROW) stage.push_back(s->pool_list[victims[i]]);
  const uint32_t n_evict = (uint32_t)stage.size();
  for (uint32_t i = 0; i < n; i++) {
    stage.push_back(missing[i]);
    stage.push_back(s->probe_pool_begin + victims[i]);
  }
  SS_HIP(hipSetDevice(s->device));
  // Rows are about to change hands.  (1) A coalescer lane's one-launch kernel may be in flight on the lane's own stream (ss_common.h
  // lstream) and reading a victim row -- and this call may itself come from the other lane's leader, who holds s->mu but not a ShardLock:
  // drain the lane streams.  (2) The next lane launch has to wait for the fill on `st`: main_dirty.  (3) A lane leader does not
  // synchronise `st` before it lets go of s->mu, so the previous fill may still be reading d_pool_stage: wait for it before overwriting.
  s->main_dirty = true;
  if (s->lanes_inflight) {
    for (hipStream_t ls : s->lstream)
      if (ls) (void)hipStreamSynchronize(ls);
    s->lanes_inflight = false;
  }
  SS_HIP(hipStreamSynchronize(st));
  if (stage.size() * sizeof(uint32_t) > s->pool_stage_cap) {
    if (s->d_pool_stage) (void)hipFree(s->d_pool_stage);
    s->d_pool_stage = nullptr; s->pool_stage_cap = 0;
    const size_t cap = std::max<size_t>(stage.size() * sizeof(uint32_t), 4096) * 2;
    SS_HIP(hipMalloc(&s->d_pool_stage, cap));
    s->pool_stage_cap = cap;
  }
  SS_HIP(hipMemcpy(s->d_pool_stage, stage.data(), stage.size() * sizeof(uint32_t), hipMemcpyHostToDevice));  // small; `stage` dies here
  // A row about to change hands may still be read by *_dev searches queued on the callers' OWN streams (they vouched for their
  // rows through ss_bm25_term_probed): the evict / fill kernels on `st` wait for everything those streams hold so far.
  if (n_evict)
    for (auto& kv : s->bm_ws) {
      if (kv.first == st) continue;
      hipEvent_t ev = nullptr;
      SS_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
      const bool ok = hipEventRecord(ev, kv.first) == hipSuccess && hipStreamWaitEvent(st, ev, 0) == hipSuccess;
      (void)hipEventDestroy(ev);  // released once the wait has been satisfied
      if (!ok) return SS_EDEVICE;
    }
  // the host tables change only now that nothing above can fail any more: host and device views stay in step
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t slot = victims[i], v = missing[i];
    if (s->pool_list[slot] != BM_NO_PROBE_ROW) s->h_probe_row[s->pool_list[slot]] = BM_NO_PROBE_ROW;
    s->pool_list[slot] = v;
    s->pool_tick[slot] = now;
    s->h_probe_row[v] = s->probe_pool_begin + slot;
  }
  if (n_evict) probe_row_evict_kernel<<<(n_evict + 255) / 256, 256, 0, st>>>(s->d_pool_stage, n_evict, s->d_probe_row);
  const unsigned long long waves = (unsigned long long)n * s->bm_n_sub;
  probe_row_fill_kernel<<<(unsigned)((waves + 3) / 4), 256, 0, st>>>(s->d_pool_stage + n_evict, n, s->bm_n_sub, s->d_sub_off,
                                                                   (const unsigned long long*)s->d_term_base, s->d_post, s->d_probe,
                                                                   s->d_probe_z, s->d_probe_row);
  SS_HIP(hipGetLastError());
  return SS_OK;
}

static bool query_lists_probed(const ss_shard* s, const ss_bm25_query& q) {
  const uint32_t all = q.n_terms + bm_q_nnot(q.op);
  uint32_t f_begin, f_end;
  query_list_range(s, q, &f_begin, &f_end);
  for (uint32_t t = 0; t < all && t < SS_MAX_QUERY_TERMS; t++) {
    if (q.term[t] >= s->bm_n_terms / s->bm_n_fields) return false;  // check_queries reports it
    for (uint32_t f = f_begin; f < f_end; f++) {
      const uint32_t v = q.term[t] * s->bm_n_fields + f;
      if (s->h_probe_row[v] == BM_NO_PROBE_ROW && s->h_df[v] != 0) return false;
    }
  }
  return true;
}

// ... of its DENSE terms (the one-launch path takes terms of either tier: a sparse list has no row and needs none)
static bool query_lists_probed_dense(const ss_shard* s, const ss_bm25_query& q) {
  const uint32_t all = q.n_terms + bm_q_nnot(q.op), L = s->bm_n_fields, n_dense = s->bm_n_terms / L;
  for (uint32_t t = 0; t < all && t < SS_MAX_QUERY_TERMS; t++) {
    if (q.term[t] >= n_dense) continue;
    const uint32_t v = q.term[t] * L + (L - 1u);  // (no field filter on this path: the only / merged list)
    if (s->h_probe_row[v] == BM_NO_PROBE_ROW && s->h_df[v] != 0) return false;
  }
  return true;
}

// A vocabulary larger than the probe budget has rows for its longest lists only (ss_bm25_set_probe_budget).  One query
// that touches a list without a row must not send its whole batch to the scan kernels: the batch is run as two -- the
// queries whose lists all have rows (pruned strategy), then the others -- and the answers are put back in the callers' order.
static int bm25_search_split_batch(ss_shard* s, uint32_t nq, const ss_bm25_query* q, uint32_t kk, uint32_t rt, uint32_t n_filters,
                                   const ss_facet_filter* filters, const std::vector<uint8_t>& probed, uint32_t n_probed) {
  // staging that outlives this call: the asynchronous copies below read it until the caller's stream synchronisation (every
  // caller synchronises s->stream before it returns, under s->mu)
  static thread_local std::vector<uint32_t> perm;
  static thread_local std::vector<ss_bm25_query> qs;
  perm.resize(nq);
  qs.resize(nq);
  uint32_t a = 0, b = n_probed;
  for (uint32_t i = 0; i < nq; i++) {
    const uint32_t at = probed[i] ? a++ : b++;
    perm[at] = i;
    qs[at] = q[i];
  }
  struct Part { bool has_and, has_or, all_probed, any_frequent, phrase, any_filter, uniform, gated; uint32_t nt_max, np_max, nn_max; } part[2];
  const uint32_t begin[2] = {0, n_probed}, count[2] = {n_probed, nq - n_probed};
  for (int h = 0; h < 2; h++)
    SS_TRY(check_queries(s, count[h], qs.data() + begin[h], &part[h].has_and, &part[h].has_or, &part[h].nt_max, &part[h].np_max,
                         &part[h].all_probed, &part[h].any_frequent, &part[h].phrase, &part[h].any_filter, &part[h].uniform, &part[h].gated, &part[h].nn_max));
  SS_HIP(hipSetDevice(s->device));
  const uint32_t kw = std::max<uint32_t>(kk, 1);
  SS_TRY(ensure_out(s, 2 * (size_t)nq, kw));  // upper half: the answers in the order they ran in
  const size_t qbytes = (size_t)nq * sizeof(ss_bm25_query) + (size_t)nq * sizeof(uint32_t);
  if (qbytes > s->bq_cap) {
    if (s->d_bq) (void)hipFree(s->d_bq);
    s->d_bq = nullptr; s->bq_cap = 0;
    SS_HIP(hipMalloc(&s->d_bq, qbytes));
    s->bq_cap = qbytes;
  }
  ss_bm25_query* d_q = (ss_bm25_query*)s->d_bq;
  uint32_t* d_perm = (uint32_t*)(d_q + nq);
  SS_HIP(hipMemcpyAsync(d_q, qs.data(), (size_t)nq * sizeof(ss_bm25_query), hipMemcpyHostToDevice, s->stream));
  SS_HIP(hipMemcpyAsync(d_perm, perm.data(), (size_t)nq * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
  uint32_t* t_doc = s->d_out_doc + (size_t)nq * kw;
  float* t_score = s->d_out_score + (size_t)nq * kw;
  uint32_t* t_count = s->d_out_count + nq;
  uint64_t* t_total = s->d_out_total + nq;
  SS_TRY(with_facet_filter(s, n_filters, filters, s->stream, [&]() {
    for (int h = 0; h < 2; h++) {
      const int rc = ssi_bm25_search(s, count[h], d_q + begin[h], kk, rt, t_doc + (size_t)begin[h] * kw, t_score + (size_t)begin[h] * kw,
                                     t_count + begin[h], t_total + begin[h], part[h].has_and, part[h].has_or, part[h].nt_max,
                                     part[h].np_max, part[h].all_probed, s->stream, part[h].any_frequent, part[h].phrase, part[h].any_filter, part[h].uniform, part[h].gated, part[h].nn_max);
      if (rc != SS_OK) return rc;
    }
    return (int)SS_OK;
  }));
  bm25_unpermute_kernel<<<nq, 64, 0, s->stream>>>(d_perm, nq, kk, t_doc, t_score, t_count, (const unsigned long long*)t_total, s->d_out_doc,
                                                   s->d_out_score, s->d_out_count, (unsigned long long*)s->d_out_total);
  SS_HIP(hipGetLastError());
  return SS_OK;
}

// A UNION that excludes a SPARSE term, or an intersection of dense terms that does (add_result.rs:3440-3497 applies NOT lists to every
// query type): the dense kernels probe NOT lists through directory rows a sparse list does not have.  Such a query -- rare: a rare word after a minus sign -- is answered on
// its own with the docs of its sparse NOT lists added to the exclusion bitmap the kernels already honour (tombstones, or a facet
// filter's bitmap): top-k and exact counts then follow from the paths that serve a shard with deleted docs.  The other queries of
// the batch run together as always; the single answers are put back into their rows.
static int bm25_search_tiered_excl(ss_shard* s, uint32_t nq, const ss_bm25_query* q, uint32_t kk, uint32_t rt, const std::vector<uint32_t>& special) {
  const uint32_t kw = std::max<uint32_t>(kk, 1), n_sp = (uint32_t)special.size(), n_dense = s->bm_n_terms / s->bm_n_fields;
  const size_t words = ((size_t)s->bm_n_docs + 31) / 32;
  SS_TRY(ensure_out(s, nq, kw));
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t h_doc = 0, h_sc = h_doc + al((size_t)n_sp * kw * 4), h_cnt = h_sc + al((size_t)n_sp * kw * 4), h_tot = h_cnt + al((size_t)n_sp * 4),
               h_need = h_tot + al((size_t)n_sp * 8);
  SS_TRY(reserve(s, &s->d_tier_hold, &s->tier_hold_cap, h_need, h_need * 2));
  SS_TRY(reserve(s, &s->d_excl_bits, &s->excl_words_cap, words));
  char* H = (char*)s->d_tier_hold;
  std::vector<ss_bm25_query> rest(q, q + nq);
  for (uint32_t j = 0; j < n_sp; j++) {
    const ss_bm25_query& Q = q[special[j]];
    const uint32_t np = Q.n_terms, n_not = bm_q_nnot(Q.op);
    ss_bm25_query R = Q;  // the query without its sparse NOT terms
    uint32_t lists[SS_MAX_QUERY_TERMS], n_lists = 0, kept = 0;
    for (uint32_t t = 0; t < n_not; t++) {
      const uint32_t term = Q.term[np + t];
      if (term >= n_dense) lists[n_lists++] = term - n_dense;
      else R.term[np + kept++] = term;
    }
    for (uint32_t t = np + kept; t < (uint32_t)SS_MAX_QUERY_TERMS; t++) R.term[t] = 0;
    R.op = (Q.op & ~0xFF00u) | SS_OP_NOT_TERMS(kept);
    rest[special[j]] = R;  // keeps the row's place in the batch below; its answer is overwritten
    const bool had = s->n_deleted != 0;
    SS_TRY(ssi_bm25_sparse_excl_bits(s, had ? s->d_deleted : nullptr, had ? (uint32_t)s->deleted_words : 0u, lists, n_lists, s->d_excl_bits, (uint32_t)words, s->stream));
    {
      ExclSwap sw(s, s->d_excl_bits, words);
      SS_TRY(ssi_bm25_search_host_queries(s, 1, &R, kk, rt, 0, nullptr));
    }
    if (nq == 1) return SS_OK;  // the answer stands in row 0 already
    if (kk) {
      SS_HIP(hipMemcpyAsync(H + h_doc + (size_t)j * kw * 4, s->d_out_doc, (size_t)kw * 4, hipMemcpyDeviceToDevice, s->stream));
      SS_HIP(hipMemcpyAsync(H + h_sc + (size_t)j * kw * 4, s->d_out_score, (size_t)kw * 4, hipMemcpyDeviceToDevice, s->stream));
    }
    SS_HIP(hipMemcpyAsync(H + h_cnt + (size_t)j * 4, s->d_out_count, 4, hipMemcpyDeviceToDevice, s->stream));
    SS_HIP(hipMemcpyAsync(H + h_tot + (size_t)j * 8, s->d_out_total, 8, hipMemcpyDeviceToDevice, s->stream));
  }
  SS_TRY(ssi_bm25_search_host_queries(s, nq, rest.data(), kk, rt, 0, nullptr));
  for (uint32_t j = 0; j < n_sp; j++) {
    const size_t i = special[j];
    if (kk) {
      SS_HIP(hipMemcpyAsync(s->d_out_doc + i * kw, H + h_doc + (size_t)j * kw * 4, (size_t)kw * 4, hipMemcpyDeviceToDevice, s->stream));
      SS_HIP(hipMemcpyAsync(s->d_out_score + i * kw, H + h_sc + (size_t)j * kw * 4, (size_t)kw * 4, hipMemcpyDeviceToDevice, s->stream));
    }
    SS_HIP(hipMemcpyAsync(s->d_out_count + i, H + h_cnt + (size_t)j * 4, 4, hipMemcpyDeviceToDevice, s->stream));
    SS_HIP(hipMemcpyAsync(s->d_out_total + i, H + h_tot + (size_t)j * 8, 8, hipMemcpyDeviceToDevice, s->stream));
  }
  return SS_OK;
}

// A UNION of several terms under a field filter that the gated scan does not take: one that names a term of the sparse tier (the dense
// tier gates every term's unlisted (term, field) lists inside the scan, BM_AND_GATED; the sparse tier keeps one merged list per term),
// or one of 8 .. 10 terms (the match byte holds 7 term bits).  The
// query is answered the way the reference itself answers it (union.rs:1168-1305, 1330-1425: union_docid_3 queues the intersection
// of all terms and every subset down to pairs, union_docid_2 runs a pair as its intersection plus the two single terms; the filter
// applies to the terms of the sub-query that finds the doc, add_result.rs:3124-3136; a doc found again keeps its better score,
// min_heap.rs:1193-1260): the 2^n - 1 filtered intersections as ONE batch through both tiers, merged per doc by the maximum -- a doc
// of the union's top-k is in the top-k of the sub-query that gives it its score.  Totals as the reference reports them: two terms
// |pass(X) u pass(Y)| (union_docid_2's count), more the UNFILTERED union (union_scan counts a doc before the filter sees it,
// union.rs:552-553).  Rare (a rare word in a multi-word query under a field filter, or 8+ words under one); <= 10 terms -- the range
// of union_docid_3 (search.rs:3497-3520) -- i.e. <= 1023 sub-queries in one batch (the sub-queries the specialised kernels do not take
// run on bm25_gallop.hip); the merge is the host's.
// A UNION of MORE than 10 terms under a field filter.  The reference leaves union_docid_3's range here (search.rs:3497-3520) and runs
// union_blockid -> union_scan_32 (union.rs:598-805), whose candidates meet the filter inside add_result_multiterm_multifield
// (add_result.rs:3124-3136) -- ANOTHER rule than the sub-queries' above: the loop over the doc's PRESENT terms returns at the first one
// that stands in no listed field, so a doc is an answer iff EVERY term it holds passes the filter, and then scores with all of them (all
// fields of each, as ever); union_scan has counted it before the filter saw it (union.rs:760-761), so result_count_total is the
// UNFILTERED union's.  With  R = U_t { docs of t that hold t in unlisted fields only }  that is: the plain union of the merged lists under
// the exclusion bitmap  tombstones | R.  R comes from the probe index's bit records: the match sets M_t (term t, no filter) and P_t (term
// t under the filter) of the 2 n single-term queries in ONE ssi_bm25_match_bits call, R |= M_t & ~P_t.  Then the ordinary many-list
// union runs under that bitmap (every kernel family honours it), its count under the tombstones alone.  Dense terms with probe rows.
__global__ void gate_rule_bits_kernel(const unsigned long long* __restrict__ sets /*[2 n][groups]: M_0, P_0, M_1, P_1, ...*/, uint32_t n, size_t groups,
                                      const uint32_t* __restrict__ base, uint32_t base_words, uint32_t* __restrict__ out, uint32_t words) {
  for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g * 2 < words; g += (size_t)gridDim.x * blockDim.x) {
    unsigned long long r = 0ull;
    if (g < groups)
      for (uint32_t t = 0; t < n; t++) r |= sets[(size_t)(2 * t) * groups + g] & ~sets[(size_t)(2 * t + 1) * groups + g];
    const size_t w0 = g * 2, w1 = g * 2 + 1;
    out[w0] = (uint32_t)r | ((base && w0 < base_words) ? base[w0] : 0u);
    if (w1 < words) out[w1] = (uint32_t)(r >> 32) | ((base && w1 < base_words) ? base[w1] : 0u);
  }
}
static int bm25_search_gated_scan_rule(ss_shard* s, const ss_bm25_query& Q, uint32_t kk, uint32_t rt, uint32_t* a_doc, float* a_score, uint32_t* a_cnt,
                                       unsigned long long* a_tot) {
  const uint32_t n = Q.n_terms, nn = bm_q_nnot(Q.op), n_dense = s->bm_n_terms / s->bm_n_fields, kw = std::max<uint32_t>(kk, 1);
  if (!s->bm_merged || !s->d_probe || 2 * n > 64) return SS_ENOTSUP;
  SS_HIP(hipSetDevice(s->device));
  // dense terms: M_t and P_t from the bit records; sparse-tier terms: their postings carry their fields (marked below)
  std::vector<ss_bm25_query> subs;
  uint32_t sp_lists[SS_MAX_QUERY_TERMS], n_sp = 0;
  for (uint32_t t = 0; t < n; t++) {
    if (Q.term[t] >= n_dense) { sp_lists[n_sp++] = Q.term[t] - n_dense; continue; }
    for (int f = 0; f < 2; f++) {
      ss_bm25_query S;
      memset(&S, 0, sizeof(S));
      S.n_terms = 1; S.term[0] = Q.term[t]; S.idf[0] = Q.idf[t];
      S.op = SS_OP_INTERSECTION | (f ? SS_OP_FIELD_FILTER(bm_q_field_filter(Q.op)) : 0u);
      subs.push_back(S);
    }
  }
  const uint32_t nd2 = (uint32_t)subs.size();  // 2 x the dense terms
  if (nd2) {
    bool has_and, has_or, all_probed, any_frequent, phrase = false, any_filter = false, uniform = false, gated = false;
    uint32_t nt_max, np_max, nn_max = 0;
    SS_TRY(ssi_bm25_ensure_probe_rows(s, nd2, subs.data(), s->stream));
    SS_TRY(check_queries(s, nd2, subs.data(), &has_and, &has_or, &nt_max, &np_max, &all_probed, &any_frequent, &phrase, &any_filter, &uniform, &gated, &nn_max));
    if (!all_probed) return SS_ENOTSUP;  // (a rationed vocabulary: the match sets are read from the bit records)
  }
  const size_t groups = (size_t)s->bm_n_sub * (BM_SUB / 64), words = ((size_t)s->bm_n_docs + 31) / 32;
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t o_q = 0, o_tot = o_q + al(64 * sizeof(ss_bm25_query)), o_sets = o_tot + al(64 * 8), need = o_sets + al(2 * (size_t)n * groups * 8);
  SS_TRY(reserve(s, &s->d_gate_ws, &s->gate_ws_cap, need));
  SS_TRY(reserve(s, &s->d_excl_bits, &s->excl_words_cap, words));
  char* W = (char*)s->d_gate_ws;
  if (nd2) {
    SS_HIP(hipMemcpy(W + o_q, subs.data(), subs.size() * sizeof(ss_bm25_query), hipMemcpyHostToDevice));  // (synchronous: `subs` is a local)
    SS_TRY(ssi_bm25_match_bits(s, (const ss_bm25_query*)(W + o_q), (unsigned long long*)(W + o_sets), (unsigned long long*)(W + o_tot), s->stream, nd2));
  }
  const bool had = s->n_deleted != 0;
  gate_rule_bits_kernel<<<(uint32_t)std::min<size_t>(2048, (words / 2 + 256) / 256), 256, 0, s->stream>>>(
      (const unsigned long long*)(W + o_sets), nd2 / 2, groups, had ? s->d_deleted : nullptr, had ? (uint32_t)s->deleted_words : 0u, s->d_excl_bits, (uint32_t)words);
  SS_HIP(hipGetLastError());
  SS_TRY(ssi_bm25_sparse_mark_unlisted(s, sp_lists, n_sp, bm_q_field_filter(Q.op), s->d_excl_bits, (uint32_t)words, s->stream));
  ss_bm25_query U = Q;  // the plain union: the filter is in the bitmap now
  U.op = SS_OP_UNION | SS_OP_NOT_TERMS(nn);
  *a_cnt = 0; *a_tot = 0;
  if (kk && rt != SS_RT_COUNT) {
    {
      ExclSwap sw(s, s->d_excl_bits, words);
      SS_TRY(ssi_bm25_search_host_queries(s, 1, &U, kk, SS_RT_TOPK, 0, nullptr));
    }
    SS_HIP(hipStreamSynchronize(s->stream));
    SS_HIP(hipMemcpy(a_doc, s->d_out_doc, (size_t)kw * 4, hipMemcpyDeviceToHost));
    SS_HIP(hipMemcpy(a_score, s->d_out_score, (size_t)kw * 4, hipMemcpyDeviceToHost));
    SS_HIP(hipMemcpy(a_cnt, s->d_out_count, 4, hipMemcpyDeviceToHost));
    *a_tot = *a_cnt;
  }
  if (rt != SS_RT_TOPK) {
    SS_TRY(ssi_bm25_search_host_queries(s, 1, &U, 0, SS_RT_COUNT, 0, nullptr));
    SS_HIP(hipStreamSynchronize(s->stream));
    SS_HIP(hipMemcpy(a_tot, s->d_out_total, 8, hipMemcpyDeviceToHost));
  }
  return SS_OK;
}

static int bm25_search_compose(ss_shard* s, uint32_t nq, const ss_bm25_query* q, uint32_t kk, uint32_t rt, const std::vector<uint32_t>& composed) {
  const uint32_t kw = std::max<uint32_t>(kk, 1), n_co = (uint32_t)composed.size();
  std::vector<uint32_t> a_doc((size_t)n_co * kw, SS_NO_DOC), a_cnt(n_co, 0);
  std::vector<float> a_score((size_t)n_co * kw, 0.f);
  std::vector<unsigned long long> a_tot(n_co, 0);
  std::vector<ss_bm25_query> rest(q, q + nq);
  const uint32_t rt_sub = rt == SS_RT_TOPK ? SS_RT_TOPK : (rt == SS_RT_COUNT ? SS_RT_COUNT : SS_RT_TOPKCOUNT);
  for (uint32_t j = 0; j < n_co; j++) {
    const ss_bm25_query& Q = q[composed[j]];
    const uint32_t n = Q.n_terms, nn = bm_q_nnot(Q.op);
    const uint32_t op_sub = SS_OP_INTERSECTION | SS_OP_NOT_TERMS(nn) | SS_OP_FIELD_FILTER(bm_q_field_filter(Q.op));
    if (n > 10) {  // the reference's other rule (union_scan + the per-doc filter): above
      SS_TRY(bm25_search_gated_scan_rule(s, Q, kk, rt, a_doc.data() + (size_t)j * kw, a_score.data() + (size_t)j * kw, &a_cnt[j], &a_tot[j]));
      rest[composed[j]] = Q;  // keeps the row's place in the batch below; its answer is overwritten
      rest[composed[j]].n_terms = 1;
      for (uint32_t t = 1; t < (uint32_t)SS_MAX_QUERY_TERMS; t++) { rest[composed[j]].term[t] = 0; rest[composed[j]].idf[t] = 0.f; }
      rest[composed[j]].op = SS_OP_INTERSECTION | SS_OP_FIELD_FILTER(bm_q_field_filter(Q.op));
      continue;
    }
    std::vector<ss_bm25_query> subs;
    for (uint32_t m = 1; m < (1u << n); m++) {
      ss_bm25_query S;
      memset(&S, 0, sizeof(S));
      for (uint32_t t = 0; t < n; t++)
        if ((m >> t) & 1u) { S.term[S.n_terms] = Q.term[t]; S.idf[S.n_terms] = Q.idf[t]; S.n_terms++; }
      if (S.n_terms + nn > (uint32_t)SS_MAX_QUERY_TERMS) return SS_EINVAL;
      for (uint32_t t = 0; t < nn; t++) S.term[S.n_terms + t] = Q.term[n + t];
      S.op = op_sub;
      subs.push_back(S);
    }
    rest[composed[j]] = subs[0];  // keeps the row's place in the batch below; its answer is overwritten
    rest[composed[j]].op = SS_OP_INTERSECTION | SS_OP_FIELD_FILTER(bm_q_field_filter(Q.op));
    const uint32_t ns = (uint32_t)subs.size();
    std::vector<unsigned long long> tot(ns, 0);
    std::vector<std::pair<float, uint32_t>> ranked;
    const bool need_subs = rt != SS_RT_COUNT || n == 2;
    if (need_subs) {
      SS_TRY(ssi_bm25_search_host_queries(s, ns, subs.data(), kk, rt_sub, 0, nullptr));
      std::vector<uint32_t> doc((size_t)ns * kw), cnt(ns);
      std::vector<float> score((size_t)ns * kw);
      SS_HIP(hipStreamSynchronize(s->stream));
      if (kk && rt != SS_RT_COUNT) {
        SS_HIP(hipMemcpy(doc.data(), s->d_out_doc, (size_t)ns * kw * 4, hipMemcpyDeviceToHost));
        SS_HIP(hipMemcpy(score.data(), s->d_out_score, (size_t)ns * kw * 4, hipMemcpyDeviceToHost));
        SS_HIP(hipMemcpy(cnt.data(), s->d_out_count, (size_t)ns * 4, hipMemcpyDeviceToHost));
        std::unordered_map<uint32_t, float> best;
        for (uint32_t i = 0; i < ns; i++)
          for (uint32_t r = 0; r < std::min(cnt[i], kk); r++) {
            auto it = best.find(doc[(size_t)i * kw + r]);
            if (it == best.end()) best.emplace(doc[(size_t)i * kw + r], score[(size_t)i * kw + r]);
            else if (score[(size_t)i * kw + r] > it->second) it->second = score[(size_t)i * kw + r];
          }
        ranked.reserve(best.size());
        for (const auto& e : best) ranked.emplace_back(e.second, e.first);
        std::sort(ranked.begin(), ranked.end(), [](const std::pair<float, uint32_t>& a, const std::pair<float, uint32_t>& b) {
          return a.first != b.first ? a.first > b.first : a.second < b.second;
        });
        if (ranked.size() > kk) ranked.resize(kk);
      }
      if (rt != SS_RT_TOPK) SS_HIP(hipMemcpy(tot.data(), s->d_out_total, (size_t)ns * 8, hipMemcpyDeviceToHost));
    }
    for (size_t r = 0; r < ranked.size(); r++) { a_doc[(size_t)j * kw + r] = ranked[r].second; a_score[(size_t)j * kw + r] = ranked[r].first; }
    a_cnt[j] = (uint32_t)ranked.size();
    if (rt == SS_RT_TOPK) a_tot[j] = ranked.size();
    else if (n == 2) a_tot[j] = tot[0] + tot[1] - tot[2];  // subsets in mask order: {X}, {Y}, {X, Y}
    else {
      ss_bm25_query U = Q;
      U.op = SS_OP_UNION | SS_OP_NOT_TERMS(nn);
      SS_TRY(ssi_bm25_search_host_queries(s, 1, &U, 0, SS_RT_COUNT, 0, nullptr));
      SS_HIP(hipStreamSynchronize(s->stream));
      SS_HIP(hipMemcpy(&a_tot[j], s->d_out_total, 8, hipMemcpyDeviceToHost));
    }
  }
  if (n_co < nq) SS_TRY(ssi_bm25_search_host_queries(s, nq, rest.data(), kk, rt, 0, nullptr));
  else SS_TRY(ensure_out(s, nq, kw));
  SS_HIP(hipStreamSynchronize(s->stream));
  for (uint32_t j = 0; j < n_co; j++) {
    const size_t i = composed[j];
    if (kk && rt != SS_RT_COUNT) {
      SS_HIP(hipMemcpy(s->d_out_doc + i * kw, a_doc.data() + (size_t)j * kw, (size_t)kw * 4, hipMemcpyHostToDevice));
      SS_HIP(hipMemcpy(s->d_out_score + i * kw, a_score.data() + (size_t)j * kw, (size_t)kw * 4, hipMemcpyHostToDevice));
    }
    SS_HIP(hipMemcpy(s->d_out_count + i, &a_cnt[j], 4, hipMemcpyHostToDevice));
    SS_HIP(hipMemcpy(s->d_out_total + i, &a_tot[j], 8, hipMemcpyHostToDevice));
  }
  return SS_OK;
}

// A batch in which some query names a term of the SPARSE tier (bm25_sparse.hip).  Those queries are answered in two parts -- their
// dense terms through the ordinary path (together with the batch's all-dense queries: one sub-batch), their sparse lists by the
// sparse kernel, which scores every doc of a sparse list in full -- and put together per query by bm25_tier_merge_kernel; the
// answers land in s->d_out_* in the callers' order, like any other batch's.  Caller holds s->mu.
static int bm25_search_tiered(ss_shard* s, uint32_t nq, const ss_bm25_query* q, uint32_t kk, uint32_t rt) {
  const uint32_t n_dense = s->bm_n_terms / s->bm_n_fields;  // public terms of the dense image
  if (s->bm_n_fields != 1 && !s->bm_merged) return SS_ENOTSUP;  // (several indexed fields: the sparse tier holds merged weights)
  std::vector<uint32_t> special;       // unions with a SPARSE NOT term: answered one by one under a per-query exclusion bitmap
  std::vector<uint32_t> composed;      // unions of several terms under a field filter: the reference's own sub-queries, one by one
  std::vector<ss_bm25_query> sub;      // the dense sub-batch: all-dense queries as they are, tiered unions reduced to their dense terms
  std::vector<ss_bm25_query> spq;      // the tiered queries, whole, for the sparse kernel
  std::vector<ss_bm25_query> spq_phrase;  // ... the phrases among them, for the sparse phrase kernel
  std::vector<uint32_t> dense_row(nq, 0xFFFFFFFFu), sparse_row(nq, 0xFFFFFFFFu);
  for (uint32_t i = 0; i < nq; i++) {
    const uint32_t op = bm_q_op(q[i].op), n_not = bm_q_nnot(q[i].op), all = q[i].n_terms + n_not;
    if (q[i].n_terms == 0 || all > SS_MAX_QUERY_TERMS) return SS_EINVAL;
    bool any_sparse = false, sparse_not = false, sparse_pos = false;
    for (uint32_t t = 0; t < all; t++) {
      if (q[i].term[t] >= n_dense + s->sp_n) return SS_EINVAL;
      if (q[i].term[t] >= n_dense) { any_sparse = true; sparse_not |= t >= q[i].n_terms; sparse_pos |= t < q[i].n_terms; }
      if (t < q[i].n_terms && !(q[i].idf[t] > 0.0f)) return SS_EINVAL;
      for (uint32_t u = 0; u < t; u++)
        if (q[i].term[u] == q[i].term[t]) return SS_EINVAL;
    }
    if (!any_sparse) {
      dense_row[i] = (uint32_t)sub.size();
      sub.push_back(q[i]);
      continue;
    }
    if (op != SS_OP_INTERSECTION && op != SS_OP_UNION && op != SS_OP_PHRASE) return SS_EINVAL;
    const bool is_phrase = op == SS_OP_PHRASE;
    // a field filter (several indexed fields): a phrase's is a test on its positions' tags; an intersection's / a single term's asks
    // every term for a listed field -- a sparse posting carries its fields; a UNION of several terms under a filter is the dense tier's
    // gated scan over (term, field) lists, which the tier does not keep: composed from filtered intersections (<= 5 terms)
    if (bm_q_field_filter(q[i].op) >> bm_real_fields(s)) return SS_EINVAL;
    const bool filtered = s->bm_n_fields > 1 && bm_q_field_filter(q[i].op) != 0u;
    if (bm_q_all_frequent(q[i].op)) return SS_ENOTSUP;
    if (filtered && op == SS_OP_UNION && q[i].n_terms > 1) {  // (bm25_route_shapes sends these to bm25_search_compose before they get here)
      if (q[i].n_terms > 10) return SS_ENOTSUP;
      composed.push_back(i);
      continue;
    }
    const bool is_and = (op == SS_OP_INTERSECTION && q[i].n_terms > 1) || is_phrase;
    // (a union's dense part cannot probe a sparse NOT list; an intersection is driven by a sparse list -- it needs one)
    const bool is_special = sparse_not && (!is_and || !sparse_pos);
    if (is_special) special.push_back(i);
    if (is_phrase && !is_special) {  // the sparse phrase kernel (bm25_sparse.hip): its shortest sparse list drives
      if (q[i].phrase_len < 2 || q[i].phrase_len > SS_MAX_PHRASE || q[i].phrase_seq[0] >= q[i].n_terms) return SS_EINVAL;
      for (uint32_t j = 1; j < q[i].phrase_len; j++)
        if (q[i].phrase_seq[j] >= q[i].n_terms && q[i].phrase_seq[j] != SS_PHRASE_SKIP) return SS_EINVAL;
      if (q[i].n_terms > 6) return SS_ENOTSUP;
      bool dense_pos = false;
      for (uint32_t t = 0; t < q[i].n_terms; t++) dense_pos |= q[i].term[t] < n_dense;
      // positions: the tier's own, and the image's for the phrase's dense words
      if (!s->d_sp_pos_end || (dense_pos && (s->bm_n_fields > 1 ? !s->d_pos32 : !s->d_pos))) return SS_ESTATE;
      sparse_row[i] = 0x80000000u | (uint32_t)spq_phrase.size();  // row behind the plain queries' (fixed up below)
      spq_phrase.push_back(q[i]);
      continue;
    }
    sparse_row[i] = (uint32_t)spq.size();
    spq.push_back(q[i]);
    if (!is_and) {  // the union's dense terms (with its NOT terms) as a query of their own
      ss_bm25_query d = q[i];
      uint32_t n = 0;
      for (uint32_t t = 0; t < q[i].n_terms; t++)
        if (q[i].term[t] < n_dense) { d.term[n] = q[i].term[t]; d.idf[n] = q[i].idf[t]; n++; }
      if (n) {
        for (uint32_t t = 0; t < n_not; t++) d.term[n + t] = q[i].term[q[i].n_terms + t];
        for (uint32_t t = n + n_not; t < (uint32_t)SS_MAX_QUERY_TERMS; t++) { d.term[t] = 0; if (t >= n) d.idf[t] = 0.f; }
        d.n_terms = n;
        dense_row[i] = (uint32_t)sub.size();
        sub.push_back(d);
      }
    }
  }
  SS_HIP(hipSetDevice(s->device));
  if (!composed.empty()) return bm25_search_compose(s, nq, q, kk, rt, composed);
  if (!special.empty()) return bm25_search_tiered_excl(s, nq, q, kk, rt, special);
  const uint32_t ns_plain = (uint32_t)spq.size();
  for (uint32_t i = 0; i < nq; i++)
    if (sparse_row[i] != 0xFFFFFFFFu && (sparse_row[i] & 0x80000000u)) sparse_row[i] = ns_plain + (sparse_row[i] & 0x7FFFFFFFu);
  spq.insert(spq.end(), spq_phrase.begin(), spq_phrase.end());
  const uint32_t kw = std::max<uint32_t>(kk, 1), ns = (uint32_t)spq.size(), nd = (uint32_t)sub.size();
  const int KPL = ssi_bm25_sparse_kpl(kw);
  SS_TRY(ensure_out(s, std::max<size_t>(nq, nd), kw));  // reserved before the sub-batch runs: its own ensure_out then keeps the buffers
  // workspace: [sparse queries][row maps 2 nq][sparse keys][sparse counts][merged doc | score | count | total][seeds of the dense sub-batch]
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t o_q = 0, o_dr = o_q + al((size_t)ns * sizeof(ss_bm25_query)), o_sr = o_dr + al((size_t)nq * 4), o_keys = o_sr + al((size_t)nq * 4),
               o_ext = o_keys + al((size_t)ns * 64 * KPL * 8), o_doc = o_ext + al((size_t)ns * 8), o_sc = o_doc + al((size_t)nq * kw * 4),
               o_cnt = o_sc + al((size_t)nq * kw * 4), o_tot = o_cnt + al((size_t)nq * 4), o_seed = o_tot + al((size_t)nq * 8), need = o_seed + al((size_t)nd * 4 + 4);
  SS_TRY(reserve(s, &s->d_tier_ws, &s->tier_ws_cap, need, need * 2));
  char* W = (char*)s->d_tier_ws;
  // the host vectors are read by synchronous copies (they may die with this frame) -- which do not wait for the stream: a tiered
  // search still queued (the device-pointer entry point returns early, bm25_search_tiered_excl runs several) reads this workspace.
  // Waited for HERE, while nothing of this call is queued yet (the stream is idle then, as a rule).
  SS_HIP(hipStreamSynchronize(s->stream));
  SS_HIP(hipMemcpy(W + o_q, spq.data(), (size_t)ns * sizeof(ss_bm25_query), hipMemcpyHostToDevice));
  SS_HIP(hipMemcpy(W + o_dr, dense_row.data(), (size_t)nq * 4, hipMemcpyHostToDevice));
  SS_HIP(hipMemcpy(W + o_sr, sparse_row.data(), (size_t)nq * 4, hipMemcpyHostToDevice));
  // The SPARSE kernel first (round 6; it used to run behind the dense sub-batch): its lists are short, its docs carry FULL scores -- a
  // union that finds k docs among its rare terms hands their k-th score to its dense terms as a threshold seed (sp_seed_kernel), and the
  // dense kernels stop reading frequent words' lists that cannot reach it.  (Small calls take the one-launch path, where the same idea
  // is role 3 publishing into the query's shared threshold; bm25_small.hip.)
  SS_TRY(ssi_bm25_launch_sparse(s, (const ss_bm25_query*)(W + o_q), ns_plain, kk, (unsigned long long*)(W + o_keys), (unsigned long long*)(W + o_ext), s->stream));
  SS_TRY(ssi_bm25_launch_sparse_phrase(s, (const ss_bm25_query*)(W + o_q) + ns_plain, ns - ns_plain, kk,
                                       (unsigned long long*)(W + o_keys) + (size_t)ns_plain * 64 * KPL, (unsigned long long*)(W + o_ext) + ns_plain, s->stream));
  if (nd) {
    if (kk) {
      SS_HIP(hipMemsetAsync(W + o_seed, 0, (size_t)nd * 4, s->stream));
      SS_TRY(ssi_bm25_launch_sparse_seeds(nq, kk, (const uint32_t*)(W + o_dr), (const uint32_t*)(W + o_sr), (const ss_bm25_query*)(W + o_q),
                                          (const unsigned long long*)(W + o_keys), (float*)(W + o_seed), s->stream));
      s->d_ext_seed = (const float*)(W + o_seed);
      s->ext_seed_n = nd;
    }
    const int rc_sub = ssi_bm25_search_host_queries(s, nd, sub.data(), kk, rt, 0, nullptr);  // -> s->d_out_* rows [0, nd)
    s->d_ext_seed = nullptr; s->ext_seed_n = 0;
    if (rc_sub != SS_OK) return rc_sub;
  }
  SS_TRY(ssi_bm25_launch_tier_merge(nq, kk, (const uint32_t*)(W + o_dr), (const uint32_t*)(W + o_sr), s->d_out_doc, s->d_out_score, s->d_out_count,
                                    (const unsigned long long*)s->d_out_total, (const unsigned long long*)(W + o_keys),
                                    (const unsigned long long*)(W + o_ext), (uint32_t*)(W + o_doc), (float*)(W + o_sc), (uint32_t*)(W + o_cnt),
                                    (unsigned long long*)(W + o_tot), s->stream));
  if (kk) {
    SS_HIP(hipMemcpyAsync(s->d_out_doc, W + o_doc, (size_t)nq * kw * 4, hipMemcpyDeviceToDevice, s->stream));
    SS_HIP(hipMemcpyAsync(s->d_out_score, W + o_sc, (size_t)nq * kw * 4, hipMemcpyDeviceToDevice, s->stream));
  }
  SS_HIP(hipMemcpyAsync(s->d_out_count, W + o_cnt, (size_t)nq * 4, hipMemcpyDeviceToDevice, s->stream));
  SS_HIP(hipMemcpyAsync(s->d_out_total, W + o_tot, (size_t)nq * 8, hipMemcpyDeviceToDevice, s->stream));
  return SS_OK;
}

// ---------------------------------------------------------------- query shapes (VERDICT r5 "next" 1)
// Every host-pointer batch passes here first.  The specialised kernel families each serve a range of shapes (check_queries,
// bm25_search_tiered); what lies outside used to come back SS_ENOTSUP -- to a drop-in caller an EMPTY result for a query the reference
// answers.  Now a query is classified and the batch run as sub-batches per kernel family, answers back in the callers' order:
//   NATIVE         what the specialised paths serve (unchanged)
//   GALLOP         intersections / filtered single terms beyond them: all_terms_frequent with > 7 terms, > 8 terms or > BM_MAX_VTERMS
//                  (term, field) lists over per-field lists (a field filter, or an image without merged lists)  -> bm25_gallop.hip
//   GALLOP_PHRASE  phrases of 7 .. SS_MAX_PHRASE unique terms, or k > 128, either tier                                 -> bm25_gallop.hip
//   COMPOSE        unions of 2 .. 10 terms under a field filter that the gated scan does not take (8 .. 10 terms, or a term of the
//                  sparse tier): the reference's own sub-queries (union.rs:1330-1425), bm25_search_compose
// SS_ENOTSUP remains for the shapes INTEGRATION.md section 4 lists as CPU fall-through (tests/test_gpu_shape_sweep.py pins the list).
enum : uint8_t { SH_NATIVE = 0, SH_GALLOP = 1, SH_GALLOP_PHRASE = 2, SH_COMPOSE = 3 };

// postings of the list(s) a query walks for `term` when it drives (dense: its only / merged list, or all its field lists)
static uint64_t shape_term_postings(const ss_shard* s, uint32_t term) {
  const uint32_t L = s->bm_n_fields, n_dense = s->bm_n_terms / L;
  if (term >= n_dense) { const uint32_t i = term - n_dense; return i + 1 < s->h_sp_base.size() ? s->h_sp_base[i + 1] - s->h_sp_base[i] : 0; }
  if (L == 1 || s->bm_merged) return s->h_df[(size_t)term * L + (L - 1u)];
  uint64_t n = 0;
  for (uint32_t f = 0; f < L; f++) n += s->h_df[(size_t)term * L + f];
  return n;
}
// the reference's own condition for all_terms_frequent (intersection.rs:198-209: posting_count / indexed_doc_count >= 0.5 in f32 for
// EVERY term), which is also the builders' rule for the lists whose codes carry the tf < 10 mark (synth.hip bm_list_flagged): a bit
// set on a query the rule does not hold for is dropped -- the reference would not have set it, and the mark is not there to read
static bool shape_freq_rule(const ss_shard* s, const ss_bm25_query& Q) {
  const uint32_t L = s->bm_n_fields, n_dense = s->bm_n_terms / L;
  for (uint32_t t = 0; t < Q.n_terms; t++) {
    if (Q.term[t] >= n_dense) return false;  // (a sparse list's codes carry no mark; ss_index_bin_tier keeps lists of half the docs dense)
    const uint64_t df = (L > 1 && !s->bm_merged) ? (Q.term[t] < s->h_df_real.size() ? s->h_df_real[Q.term[t]] : 0) : s->h_df[(size_t)Q.term[t] * L + (L - 1u)];
    if (!((float)df / (float)s->bm_n_docs >= 0.5f)) return false;
  }
  return true;
}

static int bm25_shape_of(const ss_shard* s, const ss_bm25_query& Q, uint32_t kk, uint8_t* shape, bool* drop_freq, uint64_t* driver_len) {
  const uint32_t L = s->bm_n_fields, RF = bm_real_fields(s), n_dense = s->bm_n_terms / L;
  const uint32_t op = bm_q_op(Q.op), n_not = bm_q_nnot(Q.op), np = Q.n_terms, all = np + n_not;
  *shape = SH_NATIVE; *drop_freq = false; *driver_len = 0;
  if (np == 0 || all > (uint32_t)SS_MAX_QUERY_TERMS) return SS_EINVAL;
  if (op != SS_OP_INTERSECTION && op != SS_OP_UNION && op != SS_OP_PHRASE) return SS_EINVAL;
  if (bm_q_field_filter(Q.op) >> RF) return SS_EINVAL;  // a field the image does not have
  const uint32_t filt = RF > 1 ? bm_q_field_filter(Q.op) : 0u;
  bool any_sparse = false;
  uint64_t best = ~0ull;
  for (uint32_t t = 0; t < all; t++) {
    if (Q.term[t] >= n_dense + s->sp_n) return SS_EINVAL;
    if (t < np && !(Q.idf[t] > 0.0f)) return SS_EINVAL;
    for (uint32_t u = 0; u < t; u++)
      if (Q.term[u] == Q.term[t]) return SS_EINVAL;  // unique terms only (search.rs:3023 unique_terms)
    any_sparse |= Q.term[t] >= n_dense;
    if (t < np) best = std::min(best, shape_term_postings(s, Q.term[t]));
  }
  *driver_len = best;
  const bool is_and = op == SS_OP_INTERSECTION && np > 1;
  if (bm_q_all_frequent(Q.op) && is_and && !filt) {  // (anywhere else the bit has no effect: single terms, unions, phrases, under a field filter)
    if (!shape_freq_rule(s, Q)) *drop_freq = true;
    else if (L > 1 && !s->bm_merged) return SS_ENOTSUP;  // the several-fields form of the rule is coded into the merged lists
    else if (np > 7) *shape = SH_GALLOP;
  }
  if (op == SS_OP_PHRASE) {
    if (Q.phrase_len < 2 || Q.phrase_len > SS_MAX_PHRASE || Q.phrase_seq[0] >= np) return SS_EINVAL;
    for (uint32_t j = 1; j < Q.phrase_len; j++)
      if (Q.phrase_seq[j] >= np && Q.phrase_seq[j] != SS_PHRASE_SKIP) return SS_EINVAL;
    // the phrase kernels keep positions for the unique terms 0 .. SS_MAX_PHRASE - 1 only (bm25_gallop.hip GP_NT; the staged kernel: 6): a
    // word naming a later one (an n-gram key's components before it) is the crate's to answer
    for (uint32_t j = 0; j < Q.phrase_len; j++)
      if (Q.phrase_seq[j] >= SS_MAX_PHRASE && Q.phrase_seq[j] != SS_PHRASE_SKIP) return SS_ENOTSUP;
    if (L > 1 && !s->bm_merged) return SS_ENOTSUP;  // phrases of several indexed fields run over the merged lists' field-tagged positions
    if (np > 6 || kk > 128) *shape = SH_GALLOP_PHRASE;
    // a rationed vocabulary: the phrase kernel of the probe index needs a row for EVERY list it reads and has no scan to fall back on -- a
    // phrase over a list without one takes the generic kernel, which needs none (round 5 built pool rows for it first and refused the
    // batch whose phrases alone exceeded the pool); the pool stays with the queries that gain from it.  No probe index at all (a budget
    // below two rows, or none that fitted): every list is row-less, and the phrase is answered the same way instead of being refused
    if (!any_sparse && s->bm_probe_rows == 0) *shape = SH_GALLOP_PHRASE;
    else if (!any_sparse && s->bm_probe_rows < s->bm_n_terms)
      for (uint32_t t = 0; t < all; t++) {
        const uint32_t v = Q.term[t] * L + (L - 1u);
        if (s->h_probe_row[v] == BM_NO_PROBE_ROW && s->h_df[v] != 0) *shape = SH_GALLOP_PHRASE;
      }
    return SS_OK;
  }
  if (filt && op == SS_OP_UNION && np > 1) {  // a union under a field filter: the gated scan (<= 7 dense terms), else composed
    if (np > 10 && !s->bm_merged) return SS_ENOTSUP;  // (the scan rule runs the plain union over the merged lists)
    if (any_sparse || np > 7) *shape = SH_COMPOSE;  // 8 .. 10: the reference's sub-queries; more: its other rule (bm25_search_gated_scan_rule)
    return SS_OK;
  }
  // per-field lists: under a field filter, or on an image without merged lists
  if (RF > 1 && (filt || !s->bm_merged) && !any_sparse && (all * RF > (uint32_t)BM_MAX_VTERMS || (is_and && np > 8))) {
    if (is_and || np == 1 || filt) *shape = SH_GALLOP;
    else return SS_ENOTSUP;  // a union of more than BM_MAX_VTERMS (term, field) lists on an image without merged lists
  }
  return SS_OK;
}

// *handled = false: every query is NATIVE (`*use` = the batch to run: q itself, or `norm` -- the copy with the dropped bits)
static int bm25_route_shapes(ss_shard* s, uint32_t nq, const ss_bm25_query* q, uint32_t kk, uint32_t rt, std::vector<ss_bm25_query>& norm,
                             const ss_bm25_query** use, bool* handled) {
  *handled = false;
  *use = q;
  std::vector<uint8_t> shape(nq);
  std::vector<uint64_t> dlen(nq);
  uint32_t n_class[4] = {0, 0, 0, 0};
  for (uint32_t i = 0; i < nq; i++) {
    bool drop = false;
    SS_TRY(bm25_shape_of(s, q[i], kk, &shape[i], &drop, &dlen[i]));
    if (drop) {
      if (norm.empty()) norm.assign(q, q + nq);
      norm[i].op &= ~SS_OP_ALL_TERMS_FREQUENT;
    }
    n_class[shape[i]]++;
  }
  if (!norm.empty()) *use = norm.data();
  if (n_class[SH_NATIVE] == nq) return SS_OK;
  *handled = true;
  const ss_bm25_query* Q = *use;
  if (n_class[SH_COMPOSE]) {  // (the rest of the batch comes back here through ssi_bm25_search_host_queries)
    std::vector<uint32_t> composed;
    for (uint32_t i = 0; i < nq; i++)
      if (shape[i] == SH_COMPOSE) composed.push_back(i);
    return bm25_search_compose(s, nq, Q, kk, rt, composed);
  }
  // sub-batches per kernel family; their answers are held until all have run (each writes s->d_out_* rows 0 ..)
  const uint32_t kw = std::max<uint32_t>(kk, 1);
  SS_HIP(hipSetDevice(s->device));
  SS_TRY(ensure_out(s, nq, kw));
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t o_q = 0, o_perm = o_q + al((size_t)nq * sizeof(ss_bm25_query)), o_doc = o_perm + al((size_t)nq * 4), o_sc = o_doc + al((size_t)nq * kw * 4),
               o_cnt = o_sc + al((size_t)nq * kw * 4), o_tot = o_cnt + al((size_t)nq * 4), need = o_tot + al((size_t)nq * 8);
  SS_HIP(hipStreamSynchronize(s->stream));  // the workspace may still be read by the batch before; the copies below are synchronous
  SS_TRY(reserve(s, &s->d_route_ws, &s->route_ws_cap, need, need * 2));
  char* W = (char*)s->d_route_ws;
  std::vector<ss_bm25_query> sub;
  std::vector<uint32_t> perm;
  uint32_t at = 0;
  for (uint8_t c : {SH_NATIVE, SH_GALLOP, SH_GALLOP_PHRASE}) {
    if (!n_class[c]) continue;
    sub.clear(); perm.clear();
    uint64_t longest = 0;
    for (uint32_t i = 0; i < nq; i++)
      if (shape[i] == c) { sub.push_back(Q[i]); perm.push_back(i); longest = std::max(longest, dlen[i]); }
    const uint32_t n = (uint32_t)sub.size();
    SS_HIP(hipMemcpy(W + o_perm + (size_t)at * 4, perm.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    if (c == SH_NATIVE) {
      SS_TRY(ssi_bm25_search_host_queries(s, n, sub.data(), kk, rt, 0, nullptr));
    } else {
      SS_HIP(hipMemcpy(W + o_q + (size_t)at * sizeof(ss_bm25_query), sub.data(), (size_t)n * sizeof(ss_bm25_query), hipMemcpyHostToDevice));
      SS_TRY(ssi_bm25_gallop_search(s, n, (const ss_bm25_query*)(W + o_q) + at, c == SH_GALLOP_PHRASE, longest, kk, rt, s->d_out_doc, s->d_out_score,
                                    s->d_out_count, s->d_out_total, s->stream));
      s->gallop_batches++;
    }
    bm25_unpermute_kernel<<<n, 64, 0, s->stream>>>((const uint32_t*)(W + o_perm) + at, n, kk, s->d_out_doc, s->d_out_score, s->d_out_count,
                                                  (const unsigned long long*)s->d_out_total, (uint32_t*)(W + o_doc), (float*)(W + o_sc),
                                                  (uint32_t*)(W + o_cnt), (unsigned long long*)(W + o_tot));
    SS_HIP(hipGetLastError());
    at += n;
  }
  SS_TRY(ensure_out(s, nq, kw));  // (a sub-batch never needs more rows than the batch: the buffers are the ones reserved above)
  if (kk) {
    SS_HIP(hipMemcpyAsync(s->d_out_doc, W + o_doc, (size_t)nq * kw * 4, hipMemcpyDeviceToDevice, s->stream));
    SS_HIP(hipMemcpyAsync(s->d_out_score, W + o_sc, (size_t)nq * kw * 4, hipMemcpyDeviceToDevice, s->stream));
  }
  SS_HIP(hipMemcpyAsync(s->d_out_count, W + o_cnt, (size_t)nq * 4, hipMemcpyDeviceToDevice, s->stream));
  SS_HIP(hipMemcpyAsync(s->d_out_total, W + o_tot, (size_t)nq * 8, hipMemcpyDeviceToDevice, s->stream));
  return SS_OK;
}

// the search of ss_bm25_search_filtered / _sharded up to the device lists (s->d_out_*, on s->stream); caller holds s->mu
extern "C++" int ssi_bm25_search_host_queries(ss_shard* s, uint32_t nq, const ss_bm25_query* q, uint32_t kk, uint32_t rt, uint32_t n_filters,
                                    const ss_facet_filter* filters, bool filter_prebuilt) {
  // (a facet filter: its exclusion bitmap stands in for the tombstones of everything below -- every kernel family reads the same one)
  if (n_filters) return with_facet_filter(s, n_filters, filters, s->stream, [&]() { return ssi_bm25_search_host_queries(s, nq, q, kk, rt, 0, nullptr); }, filter_prebuilt);
  std::vector<ss_bm25_query> norm;
  {
    bool handled = false;
    const ss_bm25_query* use = q;
    SS_TRY(bm25_route_shapes(s, nq, q, kk, rt, norm, &use, &handled));
    if (handled) return SS_OK;
    q = use;
  }
  if (s->sp_n) {  // an image with a sparse tier: does the batch name one of its terms?
    bool any_sparse = false;
    for (uint32_t i = 0; i < nq && !any_sparse; i++)
      for (uint32_t t = 0; t < std::min<uint32_t>(q[i].n_terms + bm_q_nnot(q[i].op), SS_MAX_QUERY_TERMS); t++)
        any_sparse |= q[i].term[t] >= s->bm_n_terms / s->bm_n_fields && q[i].term[t] < s->bm_n_terms / s->bm_n_fields + s->sp_n;
    // (a facet filter: the sparse kernel reads the same exclusion bitmap as the dense ones)
    if (any_sparse) return with_facet_filter(s, n_filters, filters, s->stream, [&]() { return bm25_search_tiered(s, nq, q, kk, rt); });
  }
  SS_TRY(ssi_bm25_ensure_probe_rows(s, nq, q, s->stream));
  if (nq > 1) {  // phrase queries have a kernel of their own: a batch that mixes them with others runs as two, answers back in place
    // (this count stays a pass of its own in front of check_queries: a mixed batch is split BEFORE that pass could refuse it, and each
    // half then reports its own errors -- folding it would change which code a batch with two faults returns)
    uint32_t n_phrase = 0;
    for (uint32_t i = 0; i < nq; i++) n_phrase += bm_q_op(q[i].op) == SS_OP_PHRASE ? 1u : 0u;
    if (n_phrase != 0 && n_phrase != nq) {
      std::vector<uint8_t> is_phrase(nq);
      for (uint32_t i = 0; i < nq; i++) is_phrase[i] = bm_q_op(q[i].op) == SS_OP_PHRASE ? 1 : 0;
      return bm25_search_split_batch(s, nq, q, kk, rt, n_filters, filters, is_phrase, n_phrase);
    }
  }
  if (nq > 1 && s->bm_probe_rows != 0 && s->bm_probe_rows < s->bm_n_terms) {  // rationed probe rows: a mixed batch runs as two
    std::vector<uint8_t> probed(nq);
    uint32_t n_probed = 0;
    for (uint32_t i = 0; i < nq; i++) n_probed += (probed[i] = query_lists_probed(s, q[i]) ? 1 : 0);
    if (n_probed != 0 && n_probed != nq) {
      bool has_and, has_or, all_probed, any_frequent, phrase;
      uint32_t nt_max, np_max;
      bool any_filter_ = false, uniform_ = false, gated_ = false;
      SS_TRY(check_queries(s, nq, q, &has_and, &has_or, &nt_max, &np_max, &all_probed, &any_frequent, &phrase, &any_filter_, &uniform_, &gated_));  // the batch's own errors first
      return bm25_search_split_batch(s, nq, q, kk, rt, n_filters, filters, probed, n_probed);
    }
  }
  // One pass validates the batch, packs it into the pinned staging and sums its postings: the staging is made ready first.  It is sized
  // for the full form, which no packed batch exceeds (bm25_pack.h).
  SS_HIP(hipSetDevice(s->device));
  const size_t qbytes = (size_t)nq * sizeof(ss_bm25_query);
  if (qbytes > s->h_bq_cap) {
    if (s->bq_ev_set) SS_HIP(hipEventSynchronize(s->bq_ev));
    if (s->h_bq) (void)hipHostFree(s->h_bq);
    s->h_bq = nullptr; s->h_bq_cap = 0;
    const size_t cap = std::max<size_t>(qbytes * 2, 64u << 10);
    SS_HIP(hipHostMalloc(&s->h_bq, cap, hipHostMallocDefault));
    s->h_bq_cap = cap;
  }
  if (!s->bq_ev) SS_HIP(hipEventCreateWithFlags(&s->bq_ev, hipEventDisableTiming));
  if (s->bq_ev_set) SS_HIP(hipEventSynchronize(s->bq_ev));  // (the copy of the batch before: long done unless the stream is backed up)
  bm_batch_sink sink;
  sink.pack.dst = (uint32_t*)s->h_bq;
  sink.pack.cap_dwords = s->h_bq_cap / sizeof(uint32_t);
  sink.df = s->bm_n_fields > 1 ? &s->h_df_real : &s->h_df;
  bool has_and = false, has_or = false;
  uint32_t nt_max = 0, np_max = 0, nn_max = 0;
  bool all_probed = false, any_frequent = false, phrase = false, any_filter = false, uniform = false, gated = false;
  SS_TRY(check_queries(s, nq, q, &has_and, &has_or, &nt_max, &np_max, &all_probed, &any_frequent, &phrase, &any_filter, &uniform, &gated, &nn_max, &sink));
  SS_TRY(ensure_out(s, nq, std::max<uint32_t>(kk, 1)));
  if (qbytes > s->bq_cap) {
    if (s->d_bq) (void)hipFree(s->d_bq);
    s->d_bq = nullptr; s->bq_cap = 0;
    SS_HIP(hipMalloc(&s->d_bq, qbytes));
    s->bq_cap = qbytes;
  }
  // the packed batch (a ninth of the full form's bytes for three-term queries), or -- a phrase batch -- the queries as they are
  const uint32_t packed_w = sink.pack.ok && sink.pack.n == nq ? sink.pack.W : 0u;
  const size_t up_bytes = packed_w ? bm_pack_bytes(nq, packed_w) : qbytes;
  if (!packed_w) memcpy(s->h_bq, q, qbytes);
  SS_HIP(hipMemcpyAsync(s->d_bq, s->h_bq, up_bytes, hipMemcpyHostToDevice, s->stream));
  SS_HIP(hipEventRecord(s->bq_ev, s->stream));
  s->bq_ev_set = true;
  s->bm_batch_postings = sink.postings / nq;  // the batch's weight, for the pruned kernel's partition rule
  const int rc_search = with_facet_filter(s, n_filters, filters, s->stream, [&]() {
    return ssi_bm25_search(s, nq, (const ss_bm25_query*)s->d_bq, kk, rt, s->d_out_doc, s->d_out_score, s->d_out_count,
                           s->d_out_total, has_and, has_or, nt_max, np_max, all_probed, s->stream, any_frequent, phrase, any_filter, uniform, gated, nn_max,
                           packed_w);
  });
  s->bm_batch_postings = 0;
  return rc_search;
}

// ---- the one-launch path of small batches (bm25_small.hip).  Pinned block of the shard: three 64-byte flag slots (0: direct calls,
// 1 / 2: the coalescer's lanes), then answer staging for direct calls (SM_H_QUERIES queries x k <= 128).
constexpr uint32_t SM_H_QUERIES = 256;  // queries of ONE host-pointer call the path takes (launches of <= 64)
constexpr size_t SM_H_DOC = 256, SM_H_SCORE = SM_H_DOC + SM_H_QUERIES * 128 * 4, SM_H_COUNT = SM_H_SCORE + SM_H_QUERIES * 128 * 4, SM_H_TOTAL = SM_H_COUNT + SM_H_QUERIES * 4,
                 SM_H_BYTES = SM_H_TOTAL + SM_H_QUERIES * 8;
// Does ONE query fit the one-launch path?  What it takes: unions and intersections of <= 4 scored and <= 4 NOT terms over one list per
// term, no field filter, no all_terms_frequent mark; terms of either tier (a sparse term: k <= 32, and a sparse NOT term only where the
// sparse role meets it -- an intersection that has a sparse scored term); phrases of <= 4 unique terms that name a sparse term (all-dense
// phrases keep their staged kernel, bm25_phrase.hip).  Cheap: host tables only, nothing of the probe pool is touched.
// sh / nn_max: the query's part in its batch's shape.  An invalid query does not fit: the staged path reports it.
static bool small_query_fits(const ss_shard* s, const ss_bm25_query& Q, uint32_t kk, ss_small_shape* sh, uint32_t* nn_max) {
  const uint32_t L = s->bm_n_fields, n_dense = s->bm_n_terms / L, RF = bm_real_fields(s);
  const uint32_t np = Q.n_terms, nn = bm_q_nnot(Q.op), op = bm_q_op(Q.op);
  if (np == 0 || np > 4 || nn > 4 || op > (uint32_t)SS_OP_PHRASE || bm_q_all_frequent(Q.op) || (RF > 1 && bm_q_field_filter(Q.op)) ||
      (bm_q_field_filter(Q.op) >> RF))  // (a field the image does not have: the staged path reports it)
    return false;
  uint32_t nd = 0;
  bool sp_scored = false, sp_not = false;
  for (uint32_t t = 0; t < np + nn; t++) {
    if (Q.term[t] >= n_dense + s->sp_n) return false;
    if (t < np && !(Q.idf[t] > 0.0f)) return false;
    for (uint32_t u = 0; u < t; u++)
      if (Q.term[u] == Q.term[t]) return false;
    if (Q.term[t] >= n_dense) { if (t < np) sp_scored = true; else sp_not = true; }
    else if (t < np) nd++;
  }
  const bool is_and = op == SS_OP_INTERSECTION && np > 1;
  bool phrase = false;
  if (op == SS_OP_PHRASE) {
    if (!sp_scored || Q.phrase_len < 2 || Q.phrase_len > (uint32_t)SS_MAX_PHRASE || Q.phrase_seq[0] >= np) return false;
    for (uint32_t j = 1; j < Q.phrase_len; j++)
      if (Q.phrase_seq[j] >= np && Q.phrase_seq[j] != SS_PHRASE_SKIP) return false;
    if (!s->d_sp_pos_end || s->sp_pos_elem != (L > 1 ? 4u : 2u) || (nd && (L > 1 ? !s->d_pos32 : !s->d_pos))) return false;
    phrase = true;
  } else if (sp_not && !(is_and && sp_scored)) {
    return false;  // a sparse NOT list the dense roles would have to probe: the staged path's per-query exclusion bitmap
  }
  if (sp_scored || sp_not) {
    if (kk > 32 || (L > 1 && !(s->bm_merged && s->h_boost.size() == L))) return false;
    sh->any_sparse = true;
  }
  sh->any_phrase |= phrase;
  const bool dense_roles = nd != 0 && !(sp_scored && (is_and || phrase));  // (an intersection with a sparse term: the sparse role alone)
  if (dense_roles) {
    if (is_and && nd > 1) sh->has_and = true;
    // (counting workgroups: unions of two or more dense lists; ONE dense list where reading it to its end would be the price of counting
    // it in passing -- under tombstones, or beside a sparse role whose threshold lets it stop early; bm25_small.hip count_by_bits)
    else if (nd > 1 || ((sp_scored || s->n_deleted) && !phrase)) sh->has_or = true;
    sh->np_max = std::max(sh->np_max, nd);
  }
  sh->any_not |= nn != 0;
  *nn_max = std::max(*nn_max, nn);
  return true;
}

// Tries the batch on the one-launch path: *handled = false (and SS_OK) when it is not of that shape -- the staged pipeline then runs it.
// p_* = pinned buffers the kernel answers into (null: the shard's own staging).  Called under s->mu.
static int bm25_small_try(ss_shard* s, uint32_t nq, const ss_bm25_query* q, uint32_t kk, uint32_t rt, uint32_t n_filters, uint32_t slot,
                          uint32_t* p_doc, float* p_score, uint32_t* p_count, uint64_t* p_total, bool* handled, uint32_t* seq_out) {
  *handled = false;
  // up to SM_H_QUERIES queries: launches of <= 64 back to back on the stream (each answers into its own rows; the flag shows the last
  // launch's number once ITS answers are in place, and the launches of one stream finish in order).  A 96-query call of the tiered image
  // was six launches and seven copies of the staged pipeline: 402 us; two launches: see profiles/r6_real_format_1m.log
  if (n_filters != 0 || kk == 0 || nq == 0 || nq > SM_H_QUERIES || !ssi_bm25_small_serves(s, std::min<uint32_t>(nq, 64u), kk, 1, 0)) return SS_OK;
  {
    ss_small_shape sh{};
    uint32_t nn_max = 0;
    for (uint32_t i = 0; i < nq; i++)
      if (!small_query_fits(s, q[i], kk, &sh, &nn_max)) return SS_OK;
    if (!ssi_bm25_small_serves(s, std::min<uint32_t>(nq, 64u), kk, sh.np_max, nn_max)) return SS_OK;
  }
  SS_TRY(ssi_bm25_ensure_probe_rows(s, nq, q, s->stream));
  for (uint32_t i = 0; i < nq; i++)  // every dense list the batch reads has a probe row now, or the scans take the batch
    if (!query_lists_probed_dense(s, q[i])) return SS_OK;
  SS_HIP(hipSetDevice(s->device));
  // slot 0 (direct calls, under ShardLock): the shard's stream and workspace.  Slots 1 / 2 (the coalescer's lanes): the lane's own
  // (ss_common.h lstream) -- created on first use; the launch waits for whatever s->stream holds at this moment.
  hipStream_t st = s->stream;
  void** wsp = &s->d_small_ws;
  if (slot != 0u) {
    const uint32_t li = slot - 1u;
    if (!s->ev_main) SS_HIP(hipEventCreateWithFlags(&s->ev_main, hipEventDisableTiming));
    // a BIG batch fills the chip by itself: two of them at once only get in each other's way (T = 256: batches of 90, 415 - 490 K q/s
    // overlapped against 490 - 510 K one behind the other) -- those queue on lane 0's stream whichever lane they come from (the workspace
    // and the flag stay the lane's own; a lane has one batch in flight at a time)
#ifndef SS_LANE_SHARE_FROM
#define SS_LANE_SHARE_FROM 48u  // (measured at 32 / 48 / 64 / never: profiles/r6_lane_streams3.log)
#endif
    constexpr uint32_t share_from = SS_LANE_SHARE_FROM;
    const uint32_t si = nq >= share_from ? 0u : li;
    if (!s->lstream[si]) {
      int pr_least = 0, pr_greatest = 0;
      (void)hipDeviceGetStreamPriorityRange(&pr_least, &pr_greatest);
      SS_HIP(hipStreamCreateWithPriority(&s->lstream[si], hipStreamNonBlocking, pr_greatest));
      s->main_dirty = true;  // (a new stream is ordered behind nothing)
    }
    st = s->lstream[si];
    s->lane_last[li] = st;
    wsp = &s->d_small_ws_l[li];
  }
  if (!*wsp) {
    SS_HIP(hipMalloc(wsp, ssi_bm25_small_ws_bytes()));
    SS_HIP(hipMemsetAsync(*wsp, 0, ssi_bm25_small_ws_bytes(), st));
  }
  SS_TRY(ssi_bm25_ensure_kth(s, s->stream));
  if (slot != 0u) {
    if (s->main_dirty) {  // both lanes behind the tail of s->stream as it stands (the flag is theirs together)
      SS_HIP(hipEventRecord(s->ev_main, s->stream));
      for (hipStream_t ls : s->lstream)
        if (ls) SS_HIP(hipStreamWaitEvent(ls, s->ev_main, 0));
      s->main_dirty = false;
    }
    s->lanes_inflight = true;
  }
  if (!s->h_small) {
    SS_HIP(hipHostMalloc((void**)&s->h_small, SM_H_BYTES, hipHostMallocDefault));
    memset(s->h_small, 0, SM_H_BYTES);
  }
  if (!p_doc) {
    p_doc = (uint32_t*)(s->h_small + SM_H_DOC); p_score = (float*)(s->h_small + SM_H_SCORE);
    p_count = (uint32_t*)(s->h_small + SM_H_COUNT); p_total = (uint64_t*)(s->h_small + SM_H_TOTAL);
  }
  uint32_t seq = 0;
  for (uint32_t c0 = 0; c0 < nq; c0 += 64u) {
    const uint32_t n = std::min<uint32_t>(64u, nq - c0);
    ss_small_shape sh{rt != SS_RT_TOPK, false, false, false, false, false, 0u};
    uint32_t nn_max = 0;
    for (uint32_t i = 0; i < n; i++) (void)small_query_fits(s, q[c0 + i], kk, &sh, &nn_max);  // this launch's own shape
    seq = ++s->small_seq ? s->small_seq : ++s->small_seq;  // never 0
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ssi_prof_begin(s, 0, st, &e0, &e1);
    const int rc = ssi_bm25_small_launch(s, *wsp, n, q + c0, kk, sh, p_doc + (size_t)c0 * kk, p_score + (size_t)c0 * kk, p_count + c0, p_total + c0,
                                        (uint32_t*)(s->h_small + 64 * slot), seq, st);
    ssi_prof_end(s, 0, st, e0, e1);
    if (rc != SS_OK) {  // (the per-query state may be half-way: start the next launch from zero; launches already queued finish first)
      (void)hipStreamSynchronize(st);
      (void)hipMemsetAsync(*wsp, 0, ssi_bm25_small_ws_bytes(), st);
      return rc;
    }
  }
  s->small_launches++;
  *seq_out = seq;
  *handled = true;
  return SS_OK;
}
// waits for the flag of `slot` to show `seq`: the kernel raises it behind the last answer.  Polled -- the answers are a few
// microseconds old when the loop sees it, where a stream synchronisation adds the completion signal's round trip
// mu_held: the caller holds s->mu (the direct path); the coalescer's lanes wait outside it
static int bm25_small_wait(ss_shard* s, uint32_t slot, uint32_t seq, bool mu_held) {
  volatile uint32_t* flag = (volatile uint32_t*)(s->h_small + 64 * slot);
  const auto t0 = std::chrono::steady_clock::now();
  int rc = SS_EDEVICE;
  for (uint32_t spins = 0;; spins++) {
    if (__atomic_load_n((const uint32_t*)flag, __ATOMIC_ACQUIRE) == seq) return SS_OK;
    __builtin_ia32_pause();
    if ((spins & 0xFFu) == 0xFFu) {
      const auto dt = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
      // a small batch is back within ~0.2 ms; past that the stream is backed up behind somebody's long work (a hybrid caller's vector
      // pass): give the core away between looks instead of burning it
      if (dt > 300) sched_yield();
      if (dt > 2000) {  // long past any small batch: ask the runtime (a kernel that died leaves the flag untouched)
        const hipError_t e = hipStreamQuery(slot ? s->lane_last[slot - 1u] : s->stream);
        if (e != hipSuccess && e != hipErrorNotReady) break;
        if (e == hipSuccess) { if (__atomic_load_n((const uint32_t*)flag, __ATOMIC_ACQUIRE) == seq) return SS_OK; break; }
        if (dt > 10000000) break;
        struct timespec ts = {0, 50000};
        nanosleep(&ts, nullptr);
      }
    }
  }
  // The launch did not come back: its per-query state (arrival counters, thresholds, totals) may be half-way, and the kernel may still
  // be writing the lane's pinned answers.  Drain the stream, start the next launch from zero, and tell the caller (VERDICT r5 weak 12,
  // ADVICE r5): without this every later one-launch batch would merge on a wrong "last arriver" or wait out the 10 s cap.
  std::unique_lock<std::mutex> g(s->mu, std::defer_lock);
  if (!mu_held) g.lock();  // (nobody enqueues another launch while the state is being zeroed)
  hipStream_t st = slot ? s->lane_last[slot - 1u] : s->stream;
  void* ws = slot ? s->d_small_ws_l[slot - 1u] : s->d_small_ws;
  (void)hipStreamSynchronize(st);
  if (ws) {
    (void)hipMemsetAsync(ws, 0, ssi_bm25_small_ws_bytes(), st);
    (void)hipStreamSynchronize(st);
  }
  return rc;
}

// The staged pipeline's answers home: rows [0, nq) of the shard's output arrays -> one pinned block [doc | score | count | total], the
// last block to finish raises the flag behind them (system-scope fence before its arrival, as bm25_small_kernel does).  The host polls
// the flag and copies into the caller's arrays: a 1000-query C2 call came home in 4 pageable copies + a stream synchronisation, ~95 us
// of its 770 (profiles/r6_bench_a.json: 0.769 ms end to end against 0.674 ms device-resident).
__global__ void __launch_bounds__(256) bm25_answers_home_kernel(const uint32_t* __restrict__ d_doc, const uint32_t* __restrict__ d_score,
                                                                const uint32_t* __restrict__ d_count, const uint32_t* __restrict__ d_total,
                                                                uint32_t n_cells, uint32_t nq, uint32_t* __restrict__ h, uint32_t* done,
                                                                uint32_t* flag, uint32_t seq) {
  const uint32_t n = 2u * n_cells + 3u * nq;  // dwords: docs, scores, counts, totals (two each)
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    uint32_t v;
    if (i < n_cells) v = d_doc[i];
    else if (i < 2u * n_cells) v = d_score[i - n_cells];
    else if (i < 2u * n_cells + nq) v = d_count[i - 2u * n_cells];
    else v = d_total[i - 2u * n_cells - nq];
    h[i] = v;
  }
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t prev = atomicAdd(done, 1u);
    if (prev + 1u == gridDim.x) {
      *done = 0u;
      __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}
// rows [0, nq) of s->d_out_* -> the caller's arrays.  Called under s->mu, behind the search on s->stream.
static int bm25_answers_home(ss_shard* s, uint32_t nq, uint32_t kk, uint32_t* out_doc, float* out_score, uint32_t* out_count, uint64_t* out_total) {
  const size_t cells = (size_t)nq * kk, dwords = 2 * cells + 3 * (size_t)nq;
  if (dwords > (64u << 20)) {  // (a huge call: the copies' bandwidth is what counts)
    if (kk) {
      SS_HIP(hipMemcpyAsync(out_doc, s->d_out_doc, cells * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
      SS_HIP(hipMemcpyAsync(out_score, s->d_out_score, cells * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    }
    SS_HIP(hipMemcpyAsync(out_count, s->d_out_count, (size_t)nq * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    SS_HIP(hipMemcpyAsync(out_total, s->d_out_total, (size_t)nq * sizeof(uint64_t), hipMemcpyDeviceToHost, s->stream));
    SS_HIP(hipStreamSynchronize(s->stream));
    return SS_OK;
  }
  if (!s->h_small) {
    SS_HIP(hipHostMalloc((void**)&s->h_small, SM_H_BYTES, hipHostMallocDefault));
    memset(s->h_small, 0, SM_H_BYTES);
  }
  if (dwords * 4 > s->h_ans_cap) {
    SS_HIP(hipStreamSynchronize(s->stream));
    if (s->h_ans) (void)hipHostFree(s->h_ans);
    s->h_ans = nullptr; s->h_ans_cap = 0;
    const size_t cap = std::max<size_t>(dwords * 4 * 2, 256u << 10);
    SS_HIP(hipHostMalloc((void**)&s->h_ans, cap, hipHostMallocDefault));
    s->h_ans_cap = cap;
  }
  if (!s->d_ans_done) {
    SS_HIP(hipMalloc(&s->d_ans_done, 64));
    SS_HIP(hipMemsetAsync(s->d_ans_done, 0, 64, s->stream));
  }
  const uint32_t seq = ++s->small_seq ? s->small_seq : ++s->small_seq;  // never 0
  const uint32_t grid = (uint32_t)std::min<size_t>(256, (dwords + 1023) / 1024);
  bm25_answers_home_kernel<<<std::max(grid, 1u), 256, 0, s->stream>>>(s->d_out_doc, (const uint32_t*)s->d_out_score, s->d_out_count, (const uint32_t*)s->d_out_total,
                                                                      (uint32_t)cells, nq, (uint32_t*)s->h_ans, s->d_ans_done, (uint32_t*)s->h_small, seq);
  SS_HIP(hipGetLastError());
  const int rc = bm25_small_wait(s, 0, seq, true);
  if (rc != SS_OK) { (void)hipMemsetAsync(s->d_ans_done, 0, 64, s->stream); return rc; }
  const uint32_t* h = (const uint32_t*)s->h_ans;
  if (kk) {
    memcpy(out_doc, h, cells * 4);
    memcpy(out_score, h + cells, cells * 4);
  }
  memcpy(out_count, h + 2 * cells, (size_t)nq * 4);
  memcpy(out_total, h + 2 * cells + nq, (size_t)nq * 8);
  return SS_OK;
}

// (the caller holds the shard lock -- taken before check_queries: it reads the image's host-side tables, which an upload replaces)
static int bm25_search_direct_locked(ss_shard* s, uint32_t nq, const ss_bm25_query* q, uint32_t k, uint32_t rt, uint32_t n_filters,
                                     const ss_facet_filter* filters, uint32_t* out_doc, float* out_score, uint32_t* out_count, uint64_t* out_total,
                                     bool filter_prebuilt = false) {
  if (!s->d_post) return SS_ESTATE;
  const uint32_t kk = rt == SS_RT_COUNT ? 0 : k, kw = std::max<uint32_t>(kk, 1u);
  // by shape, like a coalesced batch (ssi_bm25_search_direct_lane): the queries that fit the one-launch path take it, the staged pipeline
  // runs the rest -- one all-dense phrase among a caller's 96 queries used to send all of them down the staged tiered pipeline
  static thread_local std::vector<ss_bm25_query> qs;
  static thread_local std::vector<uint32_t> row_of;
  uint32_t n_fit = nq;
  bool split = false;
  // (a rationed vocabulary: one pass over the whole batch deals the pool's rows -- no split)
  // (a call of more than SM_H_QUERIES queries is the staged pipeline's whole: its fixed cost is spread thin there -- 1000 C2 queries 0.67 ms --
  // where launches of 64 cost 0.1 ms each)
  if (kk && nq > 1 && nq <= SM_H_QUERIES && n_filters == 0 && !(s->bm_probe_rows != 0 && s->bm_probe_rows < s->bm_n_terms)) {
    ss_small_shape sh{};
    uint32_t nn_max = 0;
    std::vector<uint8_t> fits(nq);
    n_fit = 0;
    for (uint32_t i = 0; i < nq; i++) n_fit += (fits[i] = (n_fit < SM_H_QUERIES && small_query_fits(s, q[i], kk, &sh, &nn_max)) ? 1 : 0);
    if (n_fit != 0 && n_fit != nq) {
      split = true;
      qs.resize(nq); row_of.resize(nq);
      uint32_t a = 0, b = n_fit;
      for (uint32_t i = 0; i < nq; i++) { const uint32_t at = fits[i] ? a++ : b++; row_of[i] = at; qs[at] = q[i]; }
    } else {
      n_fit = nq;
    }
  }
  const ss_bm25_query* qq = split ? qs.data() : q;
  bool handled = false;
  uint32_t seq = 0;
  SS_TRY(bm25_small_try(s, n_fit, qq, kk, rt, n_filters, 0, nullptr, nullptr, nullptr, nullptr, &handled, &seq));
  const uint32_t r0 = handled ? n_fit : 0u, nr = nq - r0;  // what the staged pipeline runs: the rest, or (no launch) everything
  if (!split) {  // the whole call one way or the other: straight into the caller's arrays
    if (handled) {
      SS_TRY(bm25_small_wait(s, 0, seq, true));
      memcpy(out_doc, s->h_small + SM_H_DOC, (size_t)nq * kk * sizeof(uint32_t));
      memcpy(out_score, s->h_small + SM_H_SCORE, (size_t)nq * kk * sizeof(float));
      memcpy(out_count, s->h_small + SM_H_COUNT, (size_t)nq * sizeof(uint32_t));
      memcpy(out_total, s->h_small + SM_H_TOTAL, (size_t)nq * sizeof(uint64_t));
      return SS_OK;
    }
    SS_TRY(ssi_bm25_search_host_queries(s, nq, q, kk, rt, n_filters, filters, filter_prebuilt));
    return bm25_answers_home(s, nq, kk, out_doc, out_score, out_count, out_total);
  }
  // split: the staged part behind the launch on the same stream, its answers into rows [r0, nq) of a host copy in run order
  static thread_local std::vector<uint32_t> t_doc, t_cnt;
  static thread_local std::vector<float> t_score;
  static thread_local std::vector<uint64_t> t_tot;
  t_doc.resize((size_t)nq * kw); t_score.resize((size_t)nq * kw); t_cnt.resize(nq); t_tot.resize(nq);
  int rc = SS_OK;
  if (nr) {
    rc = ssi_bm25_search_host_queries(s, nr, qq + r0, kk, rt, 0, nullptr);
    if (rc == SS_OK) {
      SS_HIP(hipStreamSynchronize(s->stream));  // (the launch ahead of it on the stream is done as well)
      SS_HIP(hipMemcpy(t_doc.data() + (size_t)r0 * kw, s->d_out_doc, (size_t)nr * kk * sizeof(uint32_t), hipMemcpyDeviceToHost));
      SS_HIP(hipMemcpy(t_score.data() + (size_t)r0 * kw, s->d_out_score, (size_t)nr * kk * sizeof(float), hipMemcpyDeviceToHost));
      SS_HIP(hipMemcpy(t_cnt.data() + r0, s->d_out_count, (size_t)nr * sizeof(uint32_t), hipMemcpyDeviceToHost));
      SS_HIP(hipMemcpy(t_tot.data() + r0, s->d_out_total, (size_t)nr * sizeof(uint64_t), hipMemcpyDeviceToHost));
    }
  }
  if (handled) {  // (waited for even when the staged part failed: the kernel writes the shard's pinned staging)
    const int rw = bm25_small_wait(s, 0, seq, true);
    if (rc == SS_OK) rc = rw;
    if (rc == SS_OK) {
      memcpy(t_doc.data(), s->h_small + SM_H_DOC, (size_t)n_fit * kk * sizeof(uint32_t));
      memcpy(t_score.data(), s->h_small + SM_H_SCORE, (size_t)n_fit * kk * sizeof(float));
      memcpy(t_cnt.data(), s->h_small + SM_H_COUNT, (size_t)n_fit * sizeof(uint32_t));
      memcpy(t_tot.data(), s->h_small + SM_H_TOTAL, (size_t)n_fit * sizeof(uint64_t));
    }
  }
  if (rc != SS_OK) return rc;
  for (uint32_t i = 0; i < nq; i++) {
    const size_t r = row_of[i];
    memcpy(out_doc + (size_t)i * kk, t_doc.data() + r * kw, (size_t)kk * sizeof(uint32_t));
    memcpy(out_score + (size_t)i * kk, t_score.data() + r * kw, (size_t)kk * sizeof(float));
    out_count[i] = t_cnt[r];
    out_total[i] = t_tot[r];
  }
  return SS_OK;
}
extern "C++" int ssi_bm25_search_direct(ss_shard* s, uint32_t nq, const ss_bm25_query* q, uint32_t k, uint32_t rt, uint32_t n_filters,
                              const ss_facet_filter* filters, uint32_t* out_doc, float* out_score, uint32_t* out_count, uint64_t* out_total) {
  ShardLock g(s);
  return bm25_search_direct_locked(s, nq, q, k, rt, n_filters, filters, out_doc, out_score, out_count, out_total);
}

// the same for a coalesced batch on a lane: the shard mutex is held while the batch is ENQUEUED (queries from the lane's pinned staging,
// kernels, results back into it, the lane's event behind them -- all on s->stream); the wait for the event happens outside, so the next
// lane's leader can enqueue behind this batch at once.
// A coalesced batch is whoever happened to call at the same time: ONE query outside the one-launch shape (a phrase of dense words only,
// five terms, ...) must not send sixty-three others down the staged pipeline.  The batch is therefore split by shape: the queries that
// fit take the one launch (answers in rows 0 .. of the lane's pinned buffers), the rest the staged pipeline (rows behind them); row_of[i]
// = where query i's answer stands.
extern "C++" int ssi_bm25_search_direct_lane(ss_shard* s, uint32_t nq, const ss_bm25_query* q, uint32_t k, uint32_t rt, uint32_t* out_doc, float* out_score,
                                   uint32_t* out_count, uint64_t* out_total, hipEvent_t ev, uint32_t lane_slot, std::vector<uint32_t>& row_of) {
  const bool trace = ssi_co_trace_on();
  const uint64_t t_in = trace ? co_now_us() : 0;
  bool small = false, staged = false;
  uint32_t small_seq = 0;
  row_of.resize(nq);
  for (uint32_t i = 0; i < nq; i++) row_of[i] = i;
  {
    std::lock_guard<std::mutex> g(s->mu);  // (NOT ShardLock: the other lane's kernel may be in flight, that is the point)
    if (!s->d_post) return SS_ESTATE;
    const uint32_t kk = rt == SS_RT_COUNT ? 0 : k, kw = std::max<uint32_t>(kk, 1u);
    std::vector<ss_bm25_query> qs;  // the batch in the order it runs in: the fitting queries first
    uint32_t n_fit = 0;
    if (kk && nq > 1 && nq <= SM_H_QUERIES && !(s->bm_probe_rows != 0 && s->bm_probe_rows < s->bm_n_terms)) {  // (a rationed vocabulary: one pass deals the pool's rows)
      ss_small_shape sh{};
      uint32_t nn_max = 0;
      std::vector<uint8_t> fits(nq);
      for (uint32_t i = 0; i < nq; i++) n_fit += (fits[i] = (n_fit < SM_H_QUERIES && small_query_fits(s, q[i], kk, &sh, &nn_max)) ? 1 : 0);  // (what one call takes)
      if (n_fit != 0 && n_fit != nq) {
        qs.resize(nq);
        uint32_t a = 0, b = n_fit;
        for (uint32_t i = 0; i < nq; i++) { const uint32_t at = fits[i] ? a++ : b++; row_of[i] = at; qs[at] = q[i]; }
        q = qs.data();
      } else {
        n_fit = nq;  // all of one kind: one attempt on the whole batch
      }
    } else {
      n_fit = nq;
    }
    // the lane's buffers are pinned: the one-launch path answers straight into them (flag slot 1 / 2 by the lane's event)
    SS_TRY(bm25_small_try(s, n_fit, q, kk, rt, 0, lane_slot, out_doc, out_score, out_count, out_total, &small, &small_seq));
    const uint32_t r0 = small ? n_fit : 0u, nr = nq - r0;  // what the staged pipeline runs: the rest, or (no launch) everything
    if (nr) {
      staged = true;
      SS_TRY(ssi_bm25_search_host_queries(s, nr, q + r0, kk, rt, 0, nullptr));
      if (kk) {
        SS_HIP(hipMemcpyAsync(out_doc + (size_t)r0 * kw, s->d_out_doc, (size_t)nr * kk * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
        SS_HIP(hipMemcpyAsync(out_score + (size_t)r0 * kw, s->d_out_score, (size_t)nr * kk * sizeof(float), hipMemcpyDeviceToHost, s->stream));
      }
      SS_HIP(hipMemcpyAsync(out_count + r0, s->d_out_count, (size_t)nr * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
      SS_HIP(hipMemcpyAsync(out_total + r0, s->d_out_total, (size_t)nr * sizeof(uint64_t), hipMemcpyDeviceToHost, s->stream));
      SS_HIP(hipEventRecord(ev, s->stream));
    }
  }
  const uint64_t te = trace ? co_now_us() : 0;
  int rc = SS_OK;
  if (small) rc = bm25_small_wait(s, lane_slot, small_seq, false);
  if (staged && hipEventSynchronize(ev) != hipSuccess && rc == SS_OK) rc = SS_EDEVICE;  // (both waited for whatever the first says: the buffers are the lane's)
  if (trace) ssi_co_trace_lane(te - t_in, co_now_us() - te);
  return rc;
}

static int bm25_search_deep(ss_shard* s, uint32_t nq, const ss_bm25_query* q, uint32_t k, uint32_t rt, uint32_t n_filters, const ss_facet_filter* filters,
                            uint32_t* out_doc, float* out_score, uint32_t* out_count, uint64_t* out_total) {
  ShardLock g(s);
  if (!s->d_post) return SS_ESTATE;
  SS_HIP(hipSetDevice(s->device));
  return with_facet_filter(s, n_filters, filters, s->stream, [&]() { return ssi_bm25_search_deep_locked(s, nq, q, k, rt, out_doc, out_score, out_count, out_total); });
}

int ss_bm25_search_filtered(ss_shard* s, uint32_t nq, const ss_bm25_query* q, uint32_t k, uint32_t rt, uint32_t n_filters,
                            const ss_facet_filter* filters, uint32_t* out_doc, float* out_score, uint32_t* out_count,
                            uint64_t* out_total) {
  if (!s || !q || !out_count || !out_total) return SS_EINVAL;
  if (rt > SS_RT_TOPKCOUNT) return SS_EINVAL;
  if (rt != SS_RT_COUNT && (k == 0 || !out_doc || !out_score)) return SS_EINVAL;
  if (!s->d_post) return SS_ESTATE;
  if (nq == 0) return SS_OK;
  // (the crate's offset + length is unbounded, search.rs:1658-1659: a page deeper than SS_MAX_K results is answered in passes)
  if (rt != SS_RT_COUNT && k > SS_MAX_K) return bm25_search_deep(s, nq, q, k, rt, n_filters, filters, out_doc, out_score, out_count, out_total);
  if (n_filters) {  // concurrent filtered callers share batches, each query under its own filters (api_coalesce.hip)
    bool submitted = false;
    const int rc = ssi_co_fac_try(s, SS_CO_FILTERED, nq, q, 0, nullptr, k, rt, n_filters, filters, 0, nullptr, nullptr, nullptr, nullptr, nullptr, out_doc, out_score,
                                  out_count, out_total, nullptr, &submitted);
    if (submitted) return rc;
  }
  if (n_filters == 0 && nq <= SS_COALESCE_MAX_REQUEST && s->co_lex.max_batch) {
    ss_co_req r;
    r.q = q; r.nq = nq; r.k = rt == SS_RT_COUNT ? 0u : k; r.rt = rt;
    r.out_doc = out_doc; r.out_score = out_score; r.out_count = out_count; r.out_total = out_total;
    return ssi_co_submit(s, s->co_lex, true, &r);
  }
  return ssi_bm25_search_direct(s, nq, q, k, rt, n_filters, filters, out_doc, out_score, out_count, out_total);
}

// One shard's part of <IndexArc as Search>::search over shards on different GPUs (search.rs:1637-1743 + 1875-2119): search
// this shard, ONE all-gather of the lists + an all-reduce of the totals over the communicator, merge on the device; every
// rank's caller receives the merged answer.  Collective: the rank of every shard of the communicator calls it with the
// same batch (in one process: one thread per shard).
int ss_bm25_search_sharded(ss_shard* s, ss_comm* c, uint32_t nq, const ss_bm25_query* q, uint32_t k, uint32_t rt,
                           uint64_t* out_doc, float* out_score, uint32_t* out_count, uint64_t* out_total) {
  if (!s || !c || !q || !out_total) return SS_EINVAL;
  if (rt > SS_RT_TOPKCOUNT) return SS_EINVAL;
  if (rt != SS_RT_COUNT && (k == 0 || !out_doc || !out_score || !out_count)) return SS_EINVAL;
  int dev = -1, n_ranks = 0;
  SS_TRY(ss_comm_info(c, nullptr, &n_ranks, &dev));
  const uint32_t kk = rt == SS_RT_COUNT ? 0 : k;
  if ((uint64_t)n_ranks * kk > 0xFFFFFFFFull) return SS_EINVAL;  // the same on every rank: nobody enters the collective
  if (nq == 0) return SS_OK;
  // From here on a failure is a matter of THIS shard (image missing, a query its lists cannot serve, an allocation): the rank
  // still enters the exchange, empty-handed, and every rank returns an error (ssi_comm_exchange) instead of blocking in it.
  ShardLock g(s);
  int rc = dev != s->device ? SS_EINVAL : !s->d_post ? SS_ESTATE : SS_OK;
  if (rc == SS_OK && kk > SS_MAX_K) {  // a deep page: this shard's (0, k) list in passes (api_deep.hip), then the exchange as ever
    std::vector<uint32_t> h_doc((size_t)nq * kk), h_cnt(nq);
    std::vector<float> h_score((size_t)nq * kk);
    std::vector<uint64_t> h_tot(nq);
    rc = ssi_bm25_search_deep_locked(s, nq, q, kk, rt, h_doc.data(), h_score.data(), h_cnt.data(), h_tot.data());
    if (rc == SS_OK) rc = ensure_out(s, nq, kk);
    if (rc == SS_OK && (hipMemcpy(s->d_out_doc, h_doc.data(), h_doc.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
                        hipMemcpy(s->d_out_score, h_score.data(), h_score.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
                        hipMemcpy(s->d_out_count, h_cnt.data(), (size_t)nq * 4, hipMemcpyHostToDevice) != hipSuccess ||
                        hipMemcpy(s->d_out_total, h_tot.data(), (size_t)nq * 8, hipMemcpyHostToDevice) != hipSuccess))
      rc = SS_EDEVICE;
  } else if (rc == SS_OK) rc = ssi_bm25_search_host_queries(s, nq, q, kk, rt, 0, nullptr);
  const ss_dev_list L{s->d_out_doc, s->d_out_score, s->d_out_count, kk};
  return ssi_comm_exchange(c, nq, kk ? 1 : 0, &L, s->d_out_total, nullptr, rc, false, 0, 0, out_doc, out_score, nullptr, out_count, out_total,
                           s->stream);
}

// The vector and hybrid shard tasks of the same search (search.rs:1680-1689, 1723-1732; RRF after the gather, 1962-2035):
// this shard's f32 scan (AnnMode::All; host queries), the same single all-gather, the merged top-k on every rank.
int ss_vec_search_sharded(ss_shard* s, ss_comm* c, uint32_t nq, const float* queries, uint32_t k, float thr, uint64_t* out_doc,
                          float* out_score, uint32_t* out_count, uint64_t* out_total) {
  if (!s || !c || !queries || !out_doc || !out_score || !out_count || !out_total) return SS_EINVAL;
  if (k == 0) return SS_EINVAL;  // (any number of queries: the scan takes them SS_VEC_BATCH per pass, one all-gather for all of them)
  int dev = -1, n_ranks = 0;
  SS_TRY(ss_comm_info(c, nullptr, &n_ranks, &dev));
  if ((uint64_t)n_ranks * k > 0xFFFFFFFFull) return SS_EINVAL;
  if (nq == 0) return SS_OK;
  ShardLock g(s);
  int rc = dev != s->device ? SS_EINVAL : !s->d_X ? SS_ESTATE : SS_OK;
  std::vector<uint32_t> h_count(nq);
  if (rc == SS_OK && k > SS_MAX_K) {  // a deep page: this shard's list in passes, then the exchange as ever
    std::vector<uint32_t> h_doc((size_t)nq * k);
    std::vector<float> h_score((size_t)nq * k);
    std::vector<uint64_t> h_tot(nq);
    rc = ssi_vec_search_deep_locked(s, nq, queries, sizeof(float), nullptr, k, thr, nullptr, h_doc.data(), h_score.data(), h_count.data(), h_tot.data(), nullptr, nullptr);
    if (rc == SS_OK) rc = ensure_out(s, nq, k);
    if (rc == SS_OK && (hipMemcpy(s->d_out_doc, h_doc.data(), h_doc.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
                        hipMemcpy(s->d_out_score, h_score.data(), h_score.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
                        hipMemcpy(s->d_out_count, h_count.data(), (size_t)nq * 4, hipMemcpyHostToDevice) != hipSuccess ||
                        hipMemcpy(s->d_out_total, h_tot.data(), (size_t)nq * 8, hipMemcpyHostToDevice) != hipSuccess))
      rc = SS_EDEVICE;
  } else if (rc == SS_OK) rc = ssi_vec_search_host_lists(s, nq, queries, sizeof(float), nullptr, k, thr, nullptr, h_count.data(), nullptr);
  const ss_dev_list L{s->d_out_doc, s->d_out_score, s->d_out_count, k};
  return ssi_comm_exchange(c, nq, 1, &L, s->d_out_total, nullptr, rc, false, 0, 0, out_doc, out_score, nullptr, out_count, out_total, s->stream);
}

// SearchMode::Hybrid over shards on different GPUs: both shard tasks with (offset 0, length k = offset + length), ONE all-gather
// of both lists, the two cross-shard concatenations sorted, RRF over them and sort / offset / length (search.rs:1962-2035,
// 2098-2119) on the device; result_count_total = sum over the shards of max(lexical, vector) (1919-1921).
int ss_hybrid_search_sharded(ss_shard* s, ss_comm* c, uint32_t nq, const ss_bm25_query* q, uint32_t rt, const float* queries, float thr,
                             uint32_t k, uint32_t offset, uint32_t length, uint64_t* out_doc, float* out_score, uint8_t* out_source,
                             uint32_t* out_count, uint64_t* out_total) {
  if (!s || !c || !q || !queries || !out_doc || !out_score || !out_count || !out_total) return SS_EINVAL;
  if (rt != SS_RT_TOPK && rt != SS_RT_TOPKCOUNT) return SS_EINVAL;
  if (k == 0 || length == 0) return SS_EINVAL;
  int dev = -1, n_ranks = 0;
  SS_TRY(ss_comm_info(c, nullptr, &n_ranks, &dev));
  if ((uint64_t)n_ranks * k > 0xFFFFFFFFull) return SS_EINVAL;
  // both concatenations live in the fusion kernel's LDS (8192 entries): beyond that, and for a page deeper than SS_MAX_K, they come home
  // after the exchange and the host fuses them (ss_merge_results: the same f32 operations in the same order) -- the same on every rank
  const bool host_fuse = k > SS_MAX_K || (uint64_t)n_ranks * k * 2 > 8192;
  if (nq == 0) return SS_OK;
  ShardLock g(s);
  int rc = dev != s->device ? SS_EINVAL : (!s->d_post || !s->d_X) ? SS_ESTATE : SS_OK;
  // outputs of the two searches side by side: the vector lists behind the lexical ones (reserved before either runs)
  if (rc == SS_OK && hipSetDevice(s->device) != hipSuccess) rc = SS_EDEVICE;
  std::vector<uint32_t> h_count(nq);
  if (rc == SS_OK && k > SS_MAX_K) {  // both shard tasks as deep pages (api_deep.hip), then placed as the exchange expects them
    std::vector<uint32_t> h_doc(2 * (size_t)nq * k), h_cnt(2 * (size_t)nq);
    std::vector<float> h_score(2 * (size_t)nq * k);
    std::vector<uint64_t> h_tot(2 * (size_t)nq);
    rc = ssi_bm25_search_deep_locked(s, nq, q, k, rt, h_doc.data(), h_score.data(), h_cnt.data(), h_tot.data());
    if (rc == SS_OK)
      rc = ssi_vec_search_deep_locked(s, nq, queries, sizeof(float), nullptr, k, thr, nullptr, h_doc.data() + (size_t)nq * k, h_score.data() + (size_t)nq * k,
                                  h_cnt.data() + nq, h_tot.data() + nq, nullptr, nullptr);
    if (rc == SS_OK) rc = ensure_out(s, 2 * (size_t)nq, k);
    if (rc == SS_OK && (hipMemcpy(s->d_out_doc, h_doc.data(), h_doc.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
                        hipMemcpy(s->d_out_score, h_score.data(), h_score.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
                        hipMemcpy(s->d_out_count, h_cnt.data(), h_cnt.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
                        hipMemcpy(s->d_out_total, h_tot.data(), h_tot.size() * 8, hipMemcpyHostToDevice) != hipSuccess))
      rc = SS_EDEVICE;
  } else {
    if (rc == SS_OK) rc = ensure_out(s, 2 * (size_t)nq, k);
    if (rc == SS_OK) rc = ssi_bm25_search_host_queries(s, nq, q, k, rt, 0, nullptr);
    if (rc == SS_OK) rc = ssi_vec_search_host_lists(s, nq, queries, sizeof(float), nullptr, k, thr, nullptr, h_count.data(), nullptr, nullptr, false, nq);
  }
  const ss_dev_list L[2] = {{s->d_out_doc, s->d_out_score, s->d_out_count, k},
                            {s->d_out_doc + (size_t)nq * k, s->d_out_score + (size_t)nq * k, s->d_out_count + nq, k}};
  return ssi_comm_exchange_hf(c, nq, 2, L, s->d_out_total, s->d_out_total + nq, rc, true, offset, length, out_doc, out_score, out_source,
                              out_count, out_total, s->stream, host_fuse);
}

// A batch for the entries that walk MATCH SETS (facet counts, the sort pivot, result sorts) on an image with a sparse tier: validated
// with tier awareness and planned (bm25_match.h).  plan->any_tiered false: nothing names a sparse term, the caller's own path applies
// untouched.  Else the dense lists of the whole batch have their probe rows and the dense parts have passed check_queries;
// SS_ENOTSUP for what the tiered match set leaves to the caller's own path.
static int tier_prepare(ss_shard* s, uint32_t nq, const ss_bm25_query* q, BmTierPlan* plan, hipStream_t st) {
  plan->any_tiered = false;
  if (!s->sp_n || nq > 64) return SS_OK;
  SS_TRY(ssi_bm25_tier_plan(s, nq, q, plan));
  if (!plan->any_tiered) return SS_OK;
  SS_TRY(ssi_bm25_ensure_probe_rows(s, nq, q, st));  // (terms of the sparse tier are passed over)
  std::vector<ss_bm25_query> dense;
  for (uint32_t i = 0; i < nq; i++)
    if (plan->has_sub[i]) dense.push_back(plan->sub[i]);
  if (!dense.empty()) {
    bool has_and, has_or, all_probed, any_frequent, phrase = false, any_filter = false, uniform = false, gated = false;
    uint32_t nt_max, np_max;
    SS_TRY(check_queries(s, (uint32_t)dense.size(), dense.data(), &has_and, &has_or, &nt_max, &np_max, &all_probed, &any_frequent, &phrase, &any_filter,
                         &uniform, &gated));
    if (!all_probed || phrase) return SS_ENOTSUP;
  }
  if (!s->d_probe) return SS_ENOTSUP;  // the match set comes from the probe index's bit records
  return SS_OK;
}

// PHRASES in such a batch (bm25_phrase_bits.hip): a phrase's match set is the match set of its intersection form, refined by its
// positions.  match_stage_phrases checks every phrase of the chunk against the image -- under the shard lock, before anything is staged;
// SS_ENOTSUP for what stays with the caller's own path -- and writes the chunk with its phrases in intersection
// form into mc->staged.  A chunk without a phrase leaves it empty: form() is then the caller's own array and every call below is the
// one such a chunk has always taken.  The staged forms are read by asynchronous copies: a MatchChunk lives until the call's synchronisation.
// (struct MatchChunk: api_internal.h -- api_delete.hip plans chunks too)
static int match_stage_phrases(const ss_shard* s, uint32_t nb, const ss_bm25_query* qc, MatchChunk* mc) {
  mc->staged.clear();
  bool any = false;
  for (uint32_t i = 0; i < nb; i++)
    if (bm_q_op(qc[i].op) == SS_OP_PHRASE) {
      SS_TRY(ssi_bm25_phrase_check(s, qc[i]));
      any = true;
    }
  if (!any) return SS_OK;
  mc->staged.assign(qc, qc + nb);
  for (uint32_t i = 0; i < nb; i++)
    if (bm_q_op(qc[i].op) == SS_OP_PHRASE) ssi_bm25_phrase_stage(qc[i], &mc->staged[i]);
  return SS_OK;
}
// what check_queries says of a chunk nothing of which is tiered: the arguments of the sorted entry's batched ssi_bm25_search
struct MatchBatchInfo {
  bool has_and = false, has_or = false, all_probed = false, any_frequent = false, any_filter = false, uniform = false, gated = false;
  uint32_t nt_max = 0, np_max = 0, nn_max = 0;
};
// THE MATCH-SET STEP of a chunk of nb <= 64 queries, in two halves, because an entry's own refusals (its facet record, its workspace)
// come between them and the order of the refusals is part of the ABI.  match_prepare, on the host: the phrases staged, the tiers
// planned, and -- where nothing is tiered -- the probe rows ensured and the chunk passed through check_queries; SS_ENOTSUP for a list
// without bit records (the match set comes from the probe index).  `info`: the sorted entry runs the chunk's batched search itself and
// takes check_queries' findings, a union under a field filter among them; without `info` check_queries refuses such a union
// (SS_ENOTSUP), as it always has for the other entries.  match_enqueue, on s->stream: the chunk's form to d_q (and the chunk as given
// to d_ph when it holds a phrase), then under the facet filter's bitmap the match sets of both tiers and the phrases' refine.  d_total
// and d_bits are the caller's to clear: the layouts differ.
static int match_prepare(ss_shard* s, uint32_t nb, const ss_bm25_query* qc, MatchChunk* mc, MatchBatchInfo* info = nullptr) {
  SS_TRY(match_stage_phrases(s, nb, qc, mc));
  const ss_bm25_query* qf = mc->form(qc);
  SS_TRY(tier_prepare(s, nb, qf, &mc->tier, s->stream));
  if (mc->tier.any_tiered) return SS_OK;
  MatchBatchInfo local, &b = info ? *info : local;
  bool phrase = false;
  SS_TRY(ssi_bm25_ensure_probe_rows(s, nb, qf, s->stream));
  SS_TRY(check_queries(s, nb, qf, &b.has_and, &b.has_or, &b.nt_max, &b.np_max, &b.all_probed, &b.any_frequent, &phrase, &b.any_filter, &b.uniform,
                       info ? &b.gated : nullptr, &b.nn_max));
  return b.all_probed && s->d_probe && !phrase ? SS_OK : SS_ENOTSUP;
}
static int match_enqueue(ss_shard* s, uint32_t nb, const ss_bm25_query* qc, const MatchChunk& mc, uint32_t n_filters, const ss_facet_filter* filters,
                         bool prebuilt, ss_bm25_query* d_q, ss_bm25_query* d_sub, ss_bm25_query* d_ph, unsigned long long* d_bits,
                         unsigned long long* d_total) {
  const ss_bm25_query* qf = mc.form(qc);
  SS_HIP(hipMemcpyAsync(d_q, qf, (size_t)nb * sizeof(ss_bm25_query), hipMemcpyHostToDevice, s->stream));
  if (mc.any_phrase()) SS_HIP(hipMemcpyAsync(d_ph, qc, (size_t)nb * sizeof(ss_bm25_query), hipMemcpyHostToDevice, s->stream));
  return with_facet_filter(s, n_filters, filters, s->stream, [&]() {
    SS_TRY(mc.tier.any_tiered ? ssi_bm25_match_bits_tiered(s, mc.tier, qf, d_q, d_sub, d_bits, d_total, s->stream, nb)
                              : ssi_bm25_match_bits(s, d_q, d_bits, d_total, s->stream, nb));
    return mc.any_phrase() ? ssi_bm25_phrase_refine(s, d_ph, d_bits, d_total, s->stream, nb) : SS_OK;
  }, prebuilt);
}

// the two halves for the ABI layer's other files (api_delete.hip): match_prepare in its form without `info`
extern "C++" int ssi_match_prepare(ss_shard* s, uint32_t nb, const ss_bm25_query* qc, MatchChunk* mc) { return match_prepare(s, nb, qc, mc); }
extern "C++" int ssi_match_enqueue(ss_shard* s, uint32_t nb, const ss_bm25_query* qc, const MatchChunk& mc, uint32_t n_filters, const ss_facet_filter* filters,
                                   ss_bm25_query* d_q, ss_bm25_query* d_sub, ss_bm25_query* d_ph, unsigned long long* d_bits, unsigned long long* d_total) {
  return match_enqueue(s, nb, qc, mc, n_filters, filters, false, d_q, d_sub, d_ph, d_bits, d_total);
}
// ss_bm25_search_filtered's deep page for a caller that holds the shard lock: the filter's bitmap built, then the passes
extern "C++" int ssi_bm25_search_deep_filtered_locked(ss_shard* s, uint32_t nq, const ss_bm25_query* q, uint32_t k, uint32_t rt, uint32_t n_filters,
                                                      const ss_facet_filter* filters, uint32_t* out_doc, float* out_score, uint32_t* out_count,
                                                      uint64_t* out_total) {
  return with_facet_filter(s, n_filters, filters, s->stream, [&]() { return ssi_bm25_search_deep_locked(s, nq, q, k, rt, out_doc, out_score, out_count, out_total); });
}

// ONE query's match set, as ss_bm25_facet_count and ss_bm25_facet_kth build it: the query prepared, then the facet's place in the record
// checked, then the workspace [query][total][match words][`extra` bytes of the caller's][dense part of a tiered query][phrase as given].
// The caller holds the shard lock, clears d_total / d_bits and calls match_enqueue; `mc` lives until its synchronisation.
struct OneMatch {
  MatchChunk mc;
  ss_bm25_query *d_q, *d_sub, *d_ph;
  unsigned long long *d_total, *d_bits;  // d_bits [groups]; the caller's bytes follow
  uint64_t groups;
};
static int one_match_prepare(ss_shard* s, const ss_bm25_query* query, uint32_t facet_offset, uint32_t facet_type, size_t extra, OneMatch* m) {
  SS_TRY(match_prepare(s, 1, query, &m->mc));
  SS_HIP(hipSetDevice(s->device));
  if (!s->d_facets || s->facet_docs < s->bm_n_docs || facet_offset + ssi_facet_width(facet_type) > s->facet_record_size) return SS_ESTATE;
  m->groups = (uint64_t)s->bm_n_sub * (BM_SUB / 64);
  SS_TRY(reserve(s, &s->d_facet_ws, &s->facet_ws_cap, sizeof(ss_bm25_query) + 8 + m->groups * 8 + extra + 2 * sizeof(ss_bm25_query)));
  char* ws = (char*)s->d_facet_ws;
  m->d_q = (ss_bm25_query*)ws;
  m->d_total = (unsigned long long*)(ws + sizeof(ss_bm25_query));
  m->d_bits = m->d_total + 1;
  m->d_sub = (ss_bm25_query*)((char*)(m->d_bits + m->groups) + extra);
  m->d_ph = m->d_sub + 1;
  return SS_OK;
}

// Facet counts of ONE query (query_facets / facet_count, add_result.rs:484-640): histogram of a facet over the query's match
// set (after NOT terms, tombstones and the facet filter).  out_counts [n_buckets + 1]: a string facet's ids 0 .. n_buckets-1,
// or the numeric ranges given by their ascending lower bounds; the last slot collects what falls outside.
static int facet_count_impl(ss_shard* s, const ss_bm25_query* query, uint32_t n_filters, const ss_facet_filter* filters,
                            uint32_t facet_offset, uint32_t facet_type, const ss_facet_point* point, uint32_t n_buckets,
                            const uint64_t* range_lower_bounds, uint64_t* out_counts, uint64_t* out_total) {
  if (!s || !query || !out_counts || n_buckets == 0 || n_buckets > (1u << 24)) return SS_EINVAL;
  const bool string_facet = facet_type == SS_FACET_STRING16 || facet_type == SS_FACET_STRING32;
  if (facet_type > SS_FACET_POINT || (!string_facet && !range_lower_bounds)) return SS_EINVAL;
  if (facet_type == SS_FACET_POINT && (!point || point->unit > SS_POINT_MILES)) return SS_EINVAL;
  if (!s->d_post) return SS_ESTATE;
  ShardLock g(s);
  OneMatch m;
  SS_TRY(one_match_prepare(s, query, facet_offset, facet_type, ((size_t)n_buckets + 1) * 8 + (size_t)n_buckets * 8, &m));
  unsigned long long* d_counts = m.d_bits + m.groups;
  uint64_t* d_bounds = (uint64_t*)(d_counts + n_buckets + 1);
  int rc = SS_OK;
  if (hipMemsetAsync(m.d_total, 0, 8 + m.groups * 8 + ((size_t)n_buckets + 1) * 8, s->stream) != hipSuccess ||
      (!string_facet &&
       hipMemcpyAsync(d_bounds, range_lower_bounds, (size_t)n_buckets * 8, hipMemcpyHostToDevice, s->stream) != hipSuccess))
    rc = SS_EDEVICE;
  if (rc == SS_OK) rc = match_enqueue(s, 1, query, m.mc, n_filters, filters, false, m.d_q, m.d_sub, m.d_ph, m.d_bits, m.d_total);
  if (rc == SS_OK) rc = ssi_facet_count(s, m.d_bits, s->bm_n_docs, facet_offset, facet_type, n_buckets, d_bounds, d_counts, point, s->stream);
  if (rc == SS_OK && (hipMemcpyAsync(out_counts, d_counts, ((size_t)n_buckets + 1) * 8, hipMemcpyDeviceToHost, s->stream) != hipSuccess ||
                      (out_total && hipMemcpyAsync(out_total, m.d_total, 8, hipMemcpyDeviceToHost, s->stream) != hipSuccess)))
    rc = SS_EDEVICE;
  if (hipStreamSynchronize(s->stream) != hipSuccess && rc == SS_OK) rc = SS_EDEVICE;
  return rc;
}

int ss_bm25_facet_count(ss_shard* s, const ss_bm25_query* query, uint32_t n_filters, const ss_facet_filter* filters,
                        uint32_t facet_offset, uint32_t facet_type, uint32_t n_buckets, const uint64_t* range_lower_bounds,
                        uint64_t* out_counts, uint64_t* out_total) {
  if (facet_type > SS_FACET_STRING32) return SS_EINVAL;  // a Point facet is counted by its distances: ss_bm25_facet_count_point
  return facet_count_impl(s, query, n_filters, filters, facet_offset, facet_type, nullptr, n_buckets, range_lower_bounds, out_counts, out_total);
}
int ss_bm25_facet_count_point(ss_shard* s, const ss_bm25_query* query, uint32_t n_filters, const ss_facet_filter* filters,
                              uint32_t facet_offset, const ss_facet_point* base, uint32_t n_buckets,
                              const uint64_t* range_lower_bounds, uint64_t* out_counts, uint64_t* out_total) {
  return facet_count_impl(s, query, n_filters, filters, facet_offset, SS_FACET_POINT, base, n_buckets, range_lower_bounds, out_counts, out_total);
}

// The pivot of a result sort (facet.hip): match set from the bit records as for facet counts, then the radix select.
static int facet_kth_impl(ss_shard* s, const ss_bm25_query* query, uint32_t n_filters, const ss_facet_filter* filters,
                          uint32_t facet_offset, uint32_t facet_type, const ss_facet_point* point, uint32_t descending, uint64_t k,
                          uint64_t* out_value, uint64_t* out_n_better, uint64_t* out_n_equal, uint64_t* out_total) {
  if (!s || !query || !out_value || !out_n_better || !out_n_equal || k == 0) return SS_EINVAL;
  if (facet_type > SS_FACET_POINT) return SS_EINVAL;
  if (facet_type == SS_FACET_STRING16 || facet_type == SS_FACET_STRING32) return SS_ENOTSUP;
  if (facet_type == SS_FACET_POINT && (!point || point->unit > SS_POINT_MILES)) return SS_EINVAL;
  if (!s->d_post) return SS_ESTATE;
  ShardLock g(s);
  OneMatch m;
  SS_TRY(one_match_prepare(s, query, facet_offset, facet_type, 256 * 8, &m));
  unsigned long long* d_hist = m.d_bits + m.groups;
  SS_HIP(hipMemsetAsync(m.d_total, 0, 8 + m.groups * 8, s->stream));
  SS_TRY(match_enqueue(s, 1, query, m.mc, n_filters, filters, false, m.d_q, m.d_sub, m.d_ph, m.d_bits, m.d_total));
  uint64_t total = 0;
  SS_HIP(hipMemcpyAsync(&total, m.d_total, 8, hipMemcpyDeviceToHost, s->stream));
  SS_HIP(hipStreamSynchronize(s->stream));
  if (out_total) *out_total = total;
  return ssi_facet_kth(s, m.d_bits, s->bm_n_docs, total, facet_offset, facet_type, descending != 0, k, d_hist, out_value, out_n_better,
                       out_n_equal, point, s->stream);
}
int ss_bm25_facet_kth(ss_shard* s, const ss_bm25_query* query, uint32_t n_filters, const ss_facet_filter* filters,
                      uint32_t facet_offset, uint32_t facet_type, uint32_t descending, uint64_t k, uint64_t* out_value,
                      uint64_t* out_n_better, uint64_t* out_n_equal, uint64_t* out_total) {
  if (facet_type > SS_FACET_STRING32) return SS_EINVAL;
  return facet_kth_impl(s, query, n_filters, filters, facet_offset, facet_type, nullptr, descending, k, out_value, out_n_better, out_n_equal, out_total);
}
int ss_bm25_facet_kth_point(ss_shard* s, const ss_bm25_query* query, uint32_t n_filters, const ss_facet_filter* filters,
                            uint32_t facet_offset, const ss_facet_point* base, uint32_t descending, uint64_t k, uint64_t* out_value,
                            uint64_t* out_n_better, uint64_t* out_n_equal, uint64_t* out_total) {
  return facet_kth_impl(s, query, n_filters, filters, facet_offset, SS_FACET_POINT, base, descending, k, out_value, out_n_better, out_n_equal, out_total);
}

// The query_facets of a call (ss_bm25_search_facets, ss_bm25_search_sorted_facets, ss_docs_search): the caller's arrays as
// query_facets_check passed them; n_bounds = the lower bounds of the range facets, back to back; stride = the counters of one query.
struct QueryFacets {
  uint32_t n_facets = 0;
  const uint32_t *facet_offset = nullptr, *facet_type = nullptr, *n_buckets = nullptr;
  const uint64_t* range_lower_bounds = nullptr;
  const ss_facet_point* bases = nullptr;
  size_t n_bounds = 0, stride = 0;
  uint64_t* out_counts = nullptr;  // [queries][stride]
};
// every argument check of the query-facet arrays (SS_EINVAL): nulls, the number of facets, every type, bucket count and Point base
static int query_facets_check(uint32_t n_facets, const uint32_t* facet_offset, const uint32_t* facet_type, const uint32_t* n_buckets,
                              const uint64_t* range_lower_bounds, const ss_facet_point* bases, uint64_t* out_counts, QueryFacets* qf) {
  if (n_facets > SS_MAX_QUERY_FACETS || (n_facets && (!facet_offset || !facet_type || !n_buckets || !out_counts))) return SS_EINVAL;
  *qf = QueryFacets{n_facets, facet_offset, facet_type, n_buckets, range_lower_bounds, bases, 0, 0, out_counts};
  for (uint32_t f = 0; f < n_facets; f++) {
    if (facet_type[f] > SS_FACET_POINT || n_buckets[f] == 0 || n_buckets[f] > (1u << 24)) return SS_EINVAL;
    if (facet_type[f] == SS_FACET_POINT && (!bases || bases[f].unit > SS_POINT_MILES)) return SS_EINVAL;
    if (facet_type[f] != SS_FACET_STRING16 && facet_type[f] != SS_FACET_STRING32) qf->n_bounds += n_buckets[f];
    qf->stride += (size_t)n_buckets[f] + 1;
  }
  return qf->n_bounds && !range_lower_bounds ? SS_EINVAL : SS_OK;
}
// what an entry asks of the facet records, under the shard lock; the return code is the entry's (ss_docs_search answers SS_EINVAL for
// a field outside the record, the other entries SS_ESTATE)
static bool facet_records_cover(const ss_shard* s) { return s->d_facets && s->facet_docs >= s->bm_n_docs; }  // a record for every doc
static bool facets_fit_records(const ss_shard* s, const QueryFacets& qf) {
  for (uint32_t f = 0; f < qf.n_facets; f++)
    if ((uint64_t)qf.facet_offset[f] + ssi_facet_width(qf.facet_type[f]) > s->facet_record_size) return false;
  return true;
}
static bool sorts_fit_records(const ss_shard* s, uint32_t n_sorts, const ss_result_sort* sorts) {
  for (uint32_t f = 0; f < n_sorts; f++)
    if ((uint64_t)sorts[f].facet_offset + ssi_facet_width(sorts[f].facet_type) > s->facet_record_size) return false;
  return true;
}

// The exclusion rows of ONE chunk (<= 64 queries) of a batch with a filter set per query: the sets grouped (filter_rows.h), staged and
// evaluated in one pass over the records (facet.hip facet_filter_rows_kernel), the row of every query uploaded.  The EachChunk is read by
// asynchronous copies: it lives until the call's synchronisation.
struct EachChunk {
  ss_filter_rows rows;
  std::vector<uint8_t> stage;
};
static size_t each_sets_bytes(uint32_t ch) { return (((size_t)ch + 1) * 4 + 15) / 16 * 16 + (size_t)ch * SS_MAX_FACET_FILTERS * sizeof(ss_facet_filter); }
static int each_chunk_rows(ss_shard* s, uint32_t nb, const uint32_t* filter_begin, const ss_facet_filter* filters, EachChunk* ec, void* d_sets,
                           uint32_t* d_rows, uint32_t* d_row_of, uint64_t groups) {
  SS_TRY(ssi_filter_rows(nb, filter_begin, filters, s->facet_record_size, &ec->rows));
  if (ec->rows.n_slow) return SS_EINVAL;  // (the entry runs those queries alone)
  SS_TRY(ssi_facet_build_rows(s, ec->rows, d_sets, &ec->stage, d_rows, (uint32_t)(groups * 2), s->stream));
  SS_HIP(hipMemcpyAsync(d_row_of, ec->rows.row_of.data(), (size_t)nb * 4, hipMemcpyHostToDevice, s->stream));
  return SS_OK;
}

// Result sort for a batch (facet.hip: "Result sort for a BATCH, pivots on the device").  The batch runs in chunks of <= 64 queries,
// every step a grid over the chunk: match sets (one expansion + one bit-record pass) -> per sort field the radix select and the
// classification -> the exclusion bitmaps -> TWO batched searches, each query inside its own doc set (the pruned kernel's filtered
// instances take one bitmap per query) -> compose into the queries' output rows.  One synchronisation per call.  A chunk the pruned
// kernel does not serve (k > 128, more than 4 lists per query, the exhaustive strategy) runs its searches query by query instead.
// With `qf` (ss_bm25_search_sorted_facets) the chunk's match sets serve the batch's query_facets too: ONE launch counts every facet of
// every query and, on the same visit of each matched doc, byte 0 of the first sort field's radix select (facet.hip
// facet_sort_first_kernel), so the select starts at its second pass.  SS_SORT_FUSED=0 (read once): the two steps apart --
// ssi_facet_count_multi, then the whole select -- for measurements; the answers are the same.
static bool sort_fused() {
  static const int on = [] { const char* e = getenv("SS_SORT_FUSED"); return e ? atoi(e) : 1; }();
  return on != 0;
}
extern "C++" int ssi_bm25_search_sorted_locked(ss_shard* s, uint32_t nq, const ss_bm25_query* queries, uint32_t n_sorts, const ss_result_sort* sorts,
                                     const ss_sort_sources& src, uint32_t k,
                                     uint32_t n_filters, const ss_facet_filter* filters, uint32_t* out_doc, float* out_score, uint32_t* out_count,
                                     uint64_t* out_total, const QueryFacets* qf, const EachSets* each) {
  if (!s->d_post) return SS_ESTATE;
  SS_HIP(hipSetDevice(s->device));
  if (!facet_records_cover(s) || !sorts_fit_records(s, n_sorts, sorts) || (qf && !facets_fit_records(s, *qf))) return SS_ESTATE;
  const uint64_t groups = (uint64_t)s->bm_n_sub * (BM_SUB / 64);
  const uint32_t CH = std::min<uint32_t>(nq, 64u);
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t o_q = 0, o_tot = o_q + al((size_t)CH * sizeof(ss_bm25_query)), o_state = o_tot + al((size_t)CH * 8), o_hist = o_state + al((size_t)CH * 64),
               o_E = o_hist + al((size_t)CH * 256 * 8), o_B = o_E + al((size_t)CH * groups * 8), o_xb = o_B + al((size_t)CH * groups * 8),
               o_xe = o_xb + al((size_t)CH * groups * 8), o_ad = o_xe + al((size_t)CH * groups * 8), o_as = o_ad + al((size_t)CH * k * 4),
               o_ac = o_as + al((size_t)CH * k * 4), o_cd = o_ac + al((size_t)CH * 4), o_cs = o_cd + al((size_t)CH * k * 4),
               o_cc = o_cs + al((size_t)CH * k * 4), o_at = o_cc + al((size_t)CH * 4), o_od = o_at + al((size_t)CH * 8),
               o_os = o_od + al((size_t)nq * k * 4), o_oc = o_os + al((size_t)nq * k * 4), o_ot = o_oc + al((size_t)nq * 4),
               o_sub = o_ot + al((size_t)nq * 8), o_ph = o_sub + al((size_t)CH * sizeof(ss_bm25_query)),
               o_bounds = o_ph + al((size_t)CH * sizeof(ss_bm25_query)), o_cnt = o_bounds + al(qf ? qf->n_bounds * 8 : 0),
               o_X = o_cnt + al(qf ? (size_t)nq * qf->stride * 8 : 0),  // (the facets' bounds and counters [nq][stride] behind the sort's own)
               o_sets = o_X + al(each ? (size_t)CH * groups * 8 : 0), o_rowof = o_sets + al(each ? each_sets_bytes(CH) : 0),
               need = o_rowof + al(each ? (size_t)CH * 4 : 0);  // (`each`: the chunk's exclusion rows, its filter sets and the row of every query)
  SS_TRY(reserve(s, &s->d_sort_ws, &s->sort_ws_cap, need));
  char* W = (char*)s->d_sort_ws;
  uint64_t* d_bounds = (uint64_t*)(W + o_bounds);
  unsigned long long* d_counts = (unsigned long long*)(W + o_cnt);
  if (qf) {
    SS_HIP(hipMemsetAsync(d_counts, 0, (size_t)nq * qf->stride * 8, s->stream));
    if (qf->n_bounds) SS_HIP(hipMemcpyAsync(d_bounds, qf->range_lower_bounds, qf->n_bounds * 8, hipMemcpyHostToDevice, s->stream));
  }
  ss_bm25_query* d_q = (ss_bm25_query*)(W + o_q);
  unsigned long long* d_total = (unsigned long long*)(W + o_tot);
  unsigned long long *d_E = (unsigned long long*)(W + o_E), *d_B = (unsigned long long*)(W + o_B), *d_xb = (unsigned long long*)(W + o_xb),
                     *d_xe = (unsigned long long*)(W + o_xe);
  SS_TRY(ensure_out(s, 1, k));
  constexpr int batched_off = 0;
  std::vector<MatchChunk> plans((nq + CH - 1) / CH);  // (staged by asynchronous copies: they live until the call's synchronisation)
  std::vector<EachChunk> each_plans(each ? plans.size() : 0);  // (likewise)
  // (`each`: a later chunk's refusal returns while the copies of the chunks before it may still read these vectors -- the stream is
  // waited for on every way out, before they go)
  struct SyncOnExit { ss_shard* s; bool on; ~SyncOnExit() { if (on) (void)hipStreamSynchronize(s->stream); } } sync_on_exit{s, each != nullptr};
  for (uint32_t c0 = 0; c0 < nq; c0 += CH) {
    const uint32_t nb = std::min<uint32_t>(CH, nq - c0);
    const ss_bm25_query* qc = queries + c0;
    // a chunk that names a sparse-tier term: its match sets from both tiers (bm25_match.h), its two searches query by query below
    // (ssi_bm25_search_host_queries routes each to bm25_search_tiered under the swapped exclusion bitmap); select and compose stay batched
    // a chunk that holds a phrase: match sets of the intersection forms, refined (bm25_phrase_bits.hip); its two searches query by
    // query as well -- the ordinary search answers a phrase under the swapped bitmap and routes it to its own kernel family
    MatchChunk& mc = plans[c0 / CH];
    MatchBatchInfo b;
    SS_TRY(match_prepare(s, nb, qc, &mc, &b));
    if (each) {  // every query under its own filters: the match sets under the tombstones alone, then each query's exclusion row applied
      EachChunk& ec = each_plans[c0 / CH];
      SS_TRY(each_chunk_rows(s, nb, each->filter_begin + c0, each->filters, &ec, W + o_sets, (uint32_t*)(W + o_X), (uint32_t*)(W + o_rowof), groups));
      SS_TRY(match_enqueue(s, nb, qc, mc, 0, nullptr, false, d_q, (ss_bm25_query*)(W + o_sub), (ss_bm25_query*)(W + o_ph), d_E, d_total));
      SS_TRY(ssi_match_exclude_rows(s, nb, d_E, (const unsigned long long*)(W + o_X), (const uint32_t*)(W + o_rowof), groups, d_total, nullptr, s->stream));
    } else
    SS_TRY(match_enqueue(s, nb, qc, mc, n_filters, filters, false, d_q, (ss_bm25_query*)(W + o_sub), (ss_bm25_query*)(W + o_ph), d_E, d_total));
    const bool fused = qf && sort_fused();
    if (fused)
      SS_TRY(ssi_facet_sort_first(s, nb, d_E, qf->n_facets, qf->facet_offset, qf->facet_type, qf->n_buckets, qf->bases, d_bounds,
                                  d_counts + (size_t)c0 * qf->stride, sorts, src, (unsigned long long*)(W + o_hist), s->stream));
    else if (qf)
      SS_TRY(ssi_facet_count_multi(s, nb, d_E, qf->n_facets, qf->facet_offset, qf->facet_type, qf->n_buckets, qf->bases, d_bounds,
                                   d_counts + (size_t)c0 * qf->stride, s->stream));
    SS_TRY(ssi_sort_select(s, nb, d_E, d_B, d_xb, d_xe, d_total, (unsigned long long*)(W + o_hist), W + o_state, n_sorts, sorts, src, k, s->stream,
                           fused));
    bool batched = !batched_off && !mc.tier.any_tiered && !mc.any_phrase();
    for (int part = 0; part < 2 && batched; part++) {  // both searches as ONE batch each: every query under its own exclusion bitmap
      ExclSwap sw(s, (uint32_t*)(part == 0 ? d_xb : d_xe), groups * 2);
      sw.per_query();
      const int rc = ssi_bm25_search(s, nb, d_q, k, SS_RT_TOPK, (uint32_t*)(W + (part == 0 ? o_ad : o_cd)), (float*)(W + (part == 0 ? o_as : o_cs)),
                                     (uint32_t*)(W + (part == 0 ? o_ac : o_cc)), (uint64_t*)(W + o_at), b.has_and, b.has_or, b.nt_max, b.np_max,
                                     b.all_probed, s->stream, b.any_frequent, false, b.any_filter, b.uniform, b.gated, b.nn_max);
      if (rc == SS_ENOTSUP && part == 0) batched = false;  // not the pruned kernel's batch: query by query below
      else if (rc != SS_OK) return rc;
    }
    if (!batched) {
      for (uint32_t i = 0; i < nb; i++)
        for (int part = 0; part < 2; part++) {
          {
            ExclSwap sw(s, (uint32_t*)((part == 0 ? d_xb : d_xe) + (size_t)i * groups), groups * 2);
            SS_TRY(ssi_bm25_search_host_queries(s, 1, qc + i, k, SS_RT_TOPK, 0, nullptr));
          }
          SS_HIP(hipMemcpyAsync(W + (part == 0 ? o_ad : o_cd) + (size_t)i * k * 4, s->d_out_doc, (size_t)k * 4, hipMemcpyDeviceToDevice, s->stream));
          SS_HIP(hipMemcpyAsync(W + (part == 0 ? o_as : o_cs) + (size_t)i * k * 4, s->d_out_score, (size_t)k * 4, hipMemcpyDeviceToDevice, s->stream));
          SS_HIP(hipMemcpyAsync(W + (part == 0 ? o_ac : o_cc) + (size_t)i * 4, s->d_out_count, 4, hipMemcpyDeviceToDevice, s->stream));
        }
    }
    SS_TRY(ssi_sort_compose(s, nb, (const uint32_t*)(W + o_ad), (const float*)(W + o_as), (const uint32_t*)(W + o_ac), (const uint32_t*)(W + o_cd),
                            (const float*)(W + o_cs), (const uint32_t*)(W + o_cc), d_total, n_sorts, sorts, src, k, (uint32_t*)(W + o_od) + (size_t)c0 * k,
                            (float*)(W + o_os) + (size_t)c0 * k, (uint32_t*)(W + o_oc) + c0, (unsigned long long*)(W + o_ot) + c0, s->stream));
  }
  SS_HIP(hipMemcpyAsync(out_doc, W + o_od, (size_t)nq * k * 4, hipMemcpyDeviceToHost, s->stream));
  SS_HIP(hipMemcpyAsync(out_score, W + o_os, (size_t)nq * k * 4, hipMemcpyDeviceToHost, s->stream));
  SS_HIP(hipMemcpyAsync(out_count, W + o_oc, (size_t)nq * 4, hipMemcpyDeviceToHost, s->stream));
  SS_HIP(hipMemcpyAsync(out_total, W + o_ot, (size_t)nq * 8, hipMemcpyDeviceToHost, s->stream));
  if (qf) SS_HIP(hipMemcpyAsync(qf->out_counts, d_counts, (size_t)nq * qf->stride * 8, hipMemcpyDeviceToHost, s->stream));
  SS_HIP(hipStreamSynchronize(s->stream));
  sync_on_exit.on = false;
  return SS_OK;
}

int ss_bm25_search_sorted(ss_shard* s, uint32_t nq, const ss_bm25_query* queries, uint32_t n_sorts, const ss_result_sort* sorts, uint32_t k,
                          uint32_t n_filters, const ss_facet_filter* filters, uint32_t* out_doc, float* out_score, uint32_t* out_count,
                          uint64_t* out_total) {
  if (!s || !queries || nq == 0 || !out_doc || !out_score || !out_count || !out_total || k == 0) return SS_EINVAL;
  if (n_sorts == 0) return ss_bm25_search_filtered(s, nq, queries, k, SS_RT_TOPKCOUNT, n_filters, filters, out_doc, out_score, out_count, out_total);
  if (!sorts) return SS_EINVAL;
  {
    bool submitted = false;
    const int rc = ssi_co_fac_try(s, SS_CO_SORTED, nq, queries, n_sorts, sorts, k, SS_RT_TOPKCOUNT, n_filters, filters, 0, nullptr, nullptr, nullptr, nullptr, nullptr,
                                  out_doc, out_score, out_count, out_total, nullptr, &submitted);
    if (submitted) return rc;
  }
  if (n_sorts > SS_MAX_SORT_FIELDS) return SS_ENOTSUP;
  for (uint32_t f = 0; f < n_sorts; f++) {
    if (sorts[f].facet_type > SS_FACET_POINT) return SS_EINVAL;
  }
  ShardLock g(s);  // (before the image is looked at: a commit swaps its arrays under this lock)
  // where every field's key is read, resolved once for the call.  A string field sorts by the rank column of
  // ss_facet_set_string_ranks; without a table SS_ENOTSUP: the host's own rank column
  ss_sort_sources src;
  SS_TRY(ssi_sort_resolve(s, n_sorts, sorts, &src));
  if (k <= SS_MAX_K) return ssi_bm25_search_sorted_locked(s, nq, queries, n_sorts, sorts, src, k, n_filters, filters, out_doc, out_score, out_count, out_total);
  return ssi_bm25_search_sorted_deep_locked(s, nq, queries, n_sorts, sorts, src, k, n_filters, filters, out_doc, out_score, out_count, out_total);
}
// A search WITH its query_facets (search.rs:3598-3760 finishes what add_result.rs:487-643 counted beside the hits): the facet counts
// of the whole batch are enqueued first -- per chunk of <= 64 queries one match-set build (both tiers) and ONE launch that counts every
// facet of every query (facet.hip: "Facet counts of a BATCH") -- and the search itself runs behind them on the same stream, through
// ss_bm25_search_filtered's direct path (bm25_search_direct_locked / ssi_bm25_search_deep_locked: that entry's answers, bit for bit; where
// the lexical coalescer is on, that entry hands an unfiltered request to it -- the search in here never goes that way, the answers are
// the same; the CALL as a whole, like every faceted, filtered or sorted call of <= 16 queries, may share a batch with concurrent callers
// through the faceted coalescer, ss_shard_set_coalescing_faceted).  The
// facet filter's bitmap is built once for all of it (`prebuilt`).  Waits: the search waits for its own answers (a deep page once per
// pass), and by then the counters are done; their copy home into the caller's pageable array and the wait that ends it are the call's
// second, short one -- the search paths own their waits, and the counters are not theirs to carry.  A workspace that has to grow waits
// for the stream before it is freed, the first time only.
static int bm25_facets_enqueue(ss_shard* s, uint32_t nq, const ss_bm25_query* q, uint32_t n_filters, const ss_facet_filter* filters,
                               const QueryFacets& qf, std::vector<MatchChunk>& plans, unsigned long long** d_counts_out) {
  const uint64_t groups = (uint64_t)s->bm_n_sub * (BM_SUB / 64);
  const bool prebuilt = n_filters != 0;  // (the entry built the bitmap)
  const uint32_t CH = std::min<uint32_t>(nq, 64u);  // (tier_prepare plans batches of <= 64, ssi_bm25_match_bits takes as many)
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t o_q = 0, o_sub = o_q + al((size_t)CH * sizeof(ss_bm25_query)), o_ph = o_sub + al((size_t)CH * sizeof(ss_bm25_query)),
               o_tot = o_ph + al((size_t)CH * sizeof(ss_bm25_query)),
               o_bits = o_tot + al((size_t)CH * 8), o_bounds = o_bits + al((size_t)CH * groups * 8), o_cnt = o_bounds + al(qf.n_bounds * 8),
               need = o_cnt + al((size_t)nq * qf.stride * 8);
  SS_TRY(reserve(s, &s->d_facet_ws, &s->facet_ws_cap, need));
  char* W = (char*)s->d_facet_ws;
  ss_bm25_query *d_q = (ss_bm25_query*)(W + o_q), *d_sub = (ss_bm25_query*)(W + o_sub), *d_ph = (ss_bm25_query*)(W + o_ph);
  unsigned long long *d_total = (unsigned long long*)(W + o_tot), *d_bits = (unsigned long long*)(W + o_bits), *d_counts = (unsigned long long*)(W + o_cnt);
  uint64_t* d_bounds = (uint64_t*)(W + o_bounds);
  *d_counts_out = d_counts;
  SS_HIP(hipMemsetAsync(d_counts, 0, (size_t)nq * qf.stride * 8, s->stream));
  if (qf.n_bounds) SS_HIP(hipMemcpyAsync(d_bounds, qf.range_lower_bounds, qf.n_bounds * 8, hipMemcpyHostToDevice, s->stream));
  plans.resize((nq + CH - 1) / CH);  // (staged by asynchronous copies: they live until the call's synchronisation)
  for (uint32_t c0 = 0; c0 < nq; c0 += CH) {
    const uint32_t nb = std::min<uint32_t>(CH, nq - c0);
    const ss_bm25_query* qc = q + c0;
    MatchChunk& mc = plans[c0 / CH];  // (a chunk holding a phrase: bm25_phrase_bits.hip; naming a sparse-tier term: bm25_match.h)
    SS_TRY(match_prepare(s, nb, qc, &mc));
    SS_HIP(hipMemsetAsync(d_total, 0, (size_t)((char*)(d_bits + (size_t)nb * groups) - (char*)d_total), s->stream));
    SS_TRY(match_enqueue(s, nb, qc, mc, n_filters, filters, prebuilt, d_q, d_sub, d_ph, d_bits, d_total));
    SS_TRY(ssi_facet_count_multi(s, nb, d_bits, qf.n_facets, qf.facet_offset, qf.facet_type, qf.n_buckets, qf.bases, d_bounds,
                                 d_counts + (size_t)c0 * qf.stride, s->stream));
  }
  return SS_OK;
}

int ss_bm25_search_facets(ss_shard* s, uint32_t nq, const ss_bm25_query* q, uint32_t k, uint32_t rt, uint32_t n_filters,
                          const ss_facet_filter* filters, uint32_t n_facets, const uint32_t* facet_offset, const uint32_t* facet_type,
                          const uint32_t* n_buckets, const uint64_t* range_lower_bounds, const ss_facet_point* bases, uint32_t* out_doc,
                          float* out_score, uint32_t* out_count, uint64_t* out_total, uint64_t* out_facet_counts) {
  if (n_facets == 0) return ss_bm25_search_filtered(s, nq, q, k, rt, n_filters, filters, out_doc, out_score, out_count, out_total);
  if (!s || !q || !out_count || !out_total) return SS_EINVAL;
  {
    bool submitted = false;
    const int rc = ssi_co_fac_try(s, SS_CO_FACETS, nq, q, 0, nullptr, k, rt, n_filters, filters, n_facets, facet_offset, facet_type, n_buckets, range_lower_bounds, bases,
                                  out_doc, out_score, out_count, out_total, out_facet_counts, &submitted);
    if (submitted) return rc;
  }
  QueryFacets qf;
  SS_TRY(query_facets_check(n_facets, facet_offset, facet_type, n_buckets, range_lower_bounds, bases, out_facet_counts, &qf));
  if (rt > SS_RT_TOPKCOUNT) return SS_EINVAL;
  if (rt != SS_RT_COUNT && (k == 0 || !out_doc || !out_score)) return SS_EINVAL;
  if (!s->d_post) return SS_ESTATE;
  if (nq == 0) return SS_OK;
  ShardLock g(s);  // (before the image is looked at: a commit swaps its arrays under this lock)
  if (!s->d_post) return SS_ESTATE;
  SS_HIP(hipSetDevice(s->device));
  if (!facet_records_cover(s) || !facets_fit_records(s, qf)) return SS_ESTATE;
  std::vector<MatchChunk> plans;
  unsigned long long* d_counts = nullptr;
  int rc = SS_OK;
  if (n_filters) {  // one exclusion bitmap for the match sets and the search
    rc = ssi_facet_build(s, n_filters, filters, s->stream);
  }
  if (rc == SS_OK) rc = bm25_facets_enqueue(s, nq, q, n_filters, filters, qf, plans, &d_counts);
  if (rc == SS_OK) {
    // (the crate's offset + length is unbounded: a page deeper than SS_MAX_K results is answered in passes, as ss_bm25_search_filtered does)
    if (rt != SS_RT_COUNT && k > SS_MAX_K)
      rc = with_facet_filter(s, n_filters, filters, s->stream, [&]() { return ssi_bm25_search_deep_locked(s, nq, q, k, rt, out_doc, out_score, out_count, out_total); }, true);
    else
      rc = bm25_search_direct_locked(s, nq, q, k, rt, n_filters, filters, out_doc, out_score, out_count, out_total, true);
  }
  if (rc == SS_OK && hipMemcpyAsync(out_facet_counts, d_counts, (size_t)nq * qf.stride * 8, hipMemcpyDeviceToHost, s->stream) != hipSuccess) rc = SS_EDEVICE;
  if (hipStreamSynchronize(s->stream) != hipSuccess && rc == SS_OK) rc = SS_EDEVICE;  // (also on an error: the plans and the caller's arrays are being read)
  return rc;
}

// A SORTED search with its query_facets: ss_bm25_search_sorted's hits and ss_bm25_search_facets' counters from ONE match-set build per
// chunk (bm25_search_sorted_locked with `qf`).  Without sort fields, without facets, or for SS_RT_COUNT one of the two entries answers
// alone; a deep page counts the facets once (bm25_facets_enqueue) and then peels the page as ss_bm25_search_sorted does.
int ss_bm25_search_sorted_facets(ss_shard* s, uint32_t nq, const ss_bm25_query* queries, uint32_t n_sorts, const ss_result_sort* sorts, uint32_t k,
                                 uint32_t rt, uint32_t n_filters, const ss_facet_filter* filters, uint32_t n_facets, const uint32_t* facet_offset,
                                 const uint32_t* facet_type, const uint32_t* n_buckets, const uint64_t* range_lower_bounds,
                                 const ss_facet_point* bases, uint32_t* out_doc, float* out_score, uint32_t* out_count, uint64_t* out_total,
                                 uint64_t* out_facet_counts) {
  if (rt > SS_RT_TOPKCOUNT) return SS_EINVAL;
  if (n_sorts == 0)
    return ss_bm25_search_facets(s, nq, queries, k, rt, n_filters, filters, n_facets, facet_offset, facet_type, n_buckets, range_lower_bounds, bases,
                                 out_doc, out_score, out_count, out_total, out_facet_counts);
  // the sorted entry's argument checks ...
  if (!s || !queries || nq == 0 || !out_count || !out_total || !sorts) return SS_EINVAL;
  {
    bool submitted = false;
    const int rc = ssi_co_fac_try(s, SS_CO_SORTED_FACETS, nq, queries, n_sorts, sorts, k, rt, n_filters, filters, n_facets, facet_offset, facet_type, n_buckets,
                                  range_lower_bounds, bases, out_doc, out_score, out_count, out_total, out_facet_counts, &submitted);
    if (submitted) return rc;
  }
  if (rt != SS_RT_COUNT && (k == 0 || !out_doc || !out_score)) return SS_EINVAL;
  if (n_sorts > SS_MAX_SORT_FIELDS) return SS_ENOTSUP;
  for (uint32_t f = 0; f < n_sorts; f++)
    if (sorts[f].facet_type > SS_FACET_POINT) return SS_EINVAL;
  if (rt != SS_RT_COUNT && n_facets == 0)
    return ss_bm25_search_sorted(s, nq, queries, n_sorts, sorts, k, n_filters, filters, out_doc, out_score, out_count, out_total);
  // ... and the facet entry's
  QueryFacets qf;
  SS_TRY(query_facets_check(n_facets, facet_offset, facet_type, n_buckets, range_lower_bounds, bases, out_facet_counts, &qf));
  ss_sort_sources src;
  {
    ShardLock g(s);  // (before the image is looked at: a commit swaps its arrays under this lock)
    SS_TRY(ssi_sort_resolve(s, n_sorts, sorts, &src));  // SS_ENOTSUP: a string field without a rank table
    if (rt != SS_RT_COUNT) {
      if (k <= SS_MAX_K)
        return ssi_bm25_search_sorted_locked(s, nq, queries, n_sorts, sorts, src, k, n_filters, filters, out_doc, out_score, out_count, out_total, &qf);
      // a deep page: the counters once, through ss_bm25_search_facets' batched count, then ss_bm25_search_sorted's passes
      if (!s->d_post) return SS_ESTATE;
      SS_HIP(hipSetDevice(s->device));
      if (!facet_records_cover(s) || !sorts_fit_records(s, n_sorts, sorts) || !facets_fit_records(s, qf)) return SS_ESTATE;
      std::vector<MatchChunk> plans;
      unsigned long long* d_counts = nullptr;
      int rc = n_filters ? ssi_facet_build(s, n_filters, filters, s->stream) : SS_OK;
      if (rc == SS_OK) rc = bm25_facets_enqueue(s, nq, queries, n_filters, filters, qf, plans, &d_counts);
      if (rc == SS_OK && hipMemcpyAsync(out_facet_counts, d_counts, (size_t)nq * qf.stride * 8, hipMemcpyDeviceToHost, s->stream) != hipSuccess)
        rc = SS_EDEVICE;
      if (hipStreamSynchronize(s->stream) != hipSuccess && rc == SS_OK) rc = SS_EDEVICE;  // (the plans and the caller's array are being read)
      if (rc != SS_OK) return rc;
      return ssi_bm25_search_sorted_deep_locked(s, nq, queries, n_sorts, sorts, src, k, n_filters, filters, out_doc, out_score, out_count, out_total);
    }
  }
  // SS_RT_COUNT: no docs, so no select -- the sort fields were checked above and play no further part
  return ss_bm25_search_facets(s, nq, queries, k, rt, n_filters, filters, n_facets, facet_offset, facet_type, n_buckets, range_lower_bounds, bases,
                               out_doc, out_score, out_count, out_total, out_facet_counts);
}

// ---- A batch whose queries each carry their OWN facet filters (ss_bm25_search_each): concurrent users of one page template share its
// sorts and its query_facets and differ in their filters.  Per chunk of <= 64 queries ONE pass over the facet records writes an exclusion
// row per distinct filter set (facet.hip facet_filter_rows_kernel), the match sets are built under the tombstones alone and every query's
// row is taken off its set (match_exclude_rows_kernel); from there on the chunk is what a call with one filter for all would have made of
// it.  The sorted half is ssi_bm25_search_sorted_locked with `each`; this is the other half: no sort fields, or SS_RT_COUNT.
//   SS_RT_TOPKCOUNT  the facets counted on the match sets, ONE batched SS_RT_TOPK search with an exclusion bitmap per query, the totals
//                    from the match sets -- where the chunk is the pruned kernel's (no phrase, no sparse-tier term, no field filter, no
//                    all_terms_frequent mark, k <= 128, ...); any other chunk runs its searches query by query through
//                    ss_bm25_search_filtered's direct path, which builds that query's own bitmap
//   SS_RT_COUNT      no search at all: the totals are the match sets' sizes
//   SS_RT_TOPK       every search through the direct path: what that entry leaves in *out_total for SS_RT_TOPK depends on the kernel
//                    family that answered, and the contract is that entry's answer
// A chunk whose match sets are refused (SS_ENOTSUP) fails the call when facets are wanted -- ss_bm25_search_facets refuses it as well --
// and runs query by query when they are not: ss_bm25_search_filtered needs no match set.  One synchronisation per call on the batched route.
// (Untuned: the batched search reads ONE bitmap per query, so every query's row is copied out beside the rows and the match sets -- three
// [chunk][groups] arrays in the workspace, 1.25 MB each per query at 10 M docs; a row index in the search kernels' exclusion read would
// spare the copy.)
static int bm25_each_unsorted_locked(ss_shard* s, uint32_t nq, const ss_bm25_query* q, uint32_t k, uint32_t rt, const EachSets& each, const QueryFacets* qf,
                                     uint32_t* out_doc, float* out_score, uint32_t* out_count, uint64_t* out_total) {
  if (!s->d_post) return SS_ESTATE;
  SS_HIP(hipSetDevice(s->device));
  const bool any_set = each.filter_begin[nq] != each.filter_begin[0], use_rows = facet_records_cover(s);
  if ((qf || any_set) && !use_rows) return SS_ESTATE;
  if (qf && !facets_fit_records(s, *qf)) return SS_ESTATE;
  const uint32_t kk = rt == SS_RT_COUNT ? 0u : k;
  auto direct_one = [&](uint32_t i) {  // query i alone, as ss_bm25_search_filtered's direct path answers it
    const uint32_t f0 = each.filter_begin[i], nf = each.filter_begin[i + 1] - f0;
    return bm25_search_direct_locked(s, 1, q + i, k, rt, nf, nf ? each.filters + f0 : nullptr, out_doc ? out_doc + (size_t)i * kk : nullptr,
                                     out_score ? out_score + (size_t)i * kk : nullptr, out_count + i, out_total + i);
  };
  if (!use_rows) {  // no facet records, and nothing that asks for them: plain searches
    for (uint32_t i = 0; i < nq; i++) SS_TRY(direct_one(i));
    return SS_OK;
  }
  const uint64_t groups = (uint64_t)s->bm_n_sub * (BM_SUB / 64);
  const uint32_t CH = std::min<uint32_t>(nq, 64u);
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t o_q = 0, o_sub = o_q + al((size_t)CH * sizeof(ss_bm25_query)), o_ph = o_sub + al((size_t)CH * sizeof(ss_bm25_query)),
               o_tot = o_ph + al((size_t)CH * sizeof(ss_bm25_query)), o_bits = o_tot + al((size_t)CH * 8), o_X = o_bits + al((size_t)CH * groups * 8),
               o_Xq = o_X + al((size_t)CH * groups * 8), o_sets = o_Xq + al((size_t)CH * groups * 8), o_rowof = o_sets + al(each_sets_bytes(CH)),
               o_stot = o_rowof + al((size_t)CH * 4), o_bounds = o_stot + al((size_t)CH * 8), o_cnt = o_bounds + al(qf ? qf->n_bounds * 8 : 0),
               o_od = o_cnt + al(qf ? (size_t)nq * qf->stride * 8 : 0), o_os = o_od + al((size_t)nq * kk * 4), o_oc = o_os + al((size_t)nq * kk * 4),
               o_ot = o_oc + al((size_t)nq * 4), need = o_ot + al((size_t)nq * 8);
  SS_TRY(reserve(s, &s->d_facet_ws, &s->facet_ws_cap, need));
  char* W = (char*)s->d_facet_ws;
  ss_bm25_query* d_q = (ss_bm25_query*)(W + o_q);
  unsigned long long *d_total = (unsigned long long*)(W + o_tot), *d_bits = (unsigned long long*)(W + o_bits), *d_counts = (unsigned long long*)(W + o_cnt);
  uint64_t* d_bounds = (uint64_t*)(W + o_bounds);
  std::vector<MatchChunk> plans((nq + CH - 1) / CH);  // (staged by asynchronous copies: they live until the call's synchronisation)
  std::vector<EachChunk> each_plans(plans.size());
  std::vector<uint8_t> batched(plans.size(), 0);
  auto run = [&]() -> int {
    if (qf) {
      SS_HIP(hipMemsetAsync(d_counts, 0, (size_t)nq * qf->stride * 8, s->stream));
      if (qf->n_bounds) SS_HIP(hipMemcpyAsync(d_bounds, qf->range_lower_bounds, qf->n_bounds * 8, hipMemcpyHostToDevice, s->stream));
    }
    for (uint32_t c0 = 0; c0 < nq; c0 += CH) {
      const uint32_t nb = std::min<uint32_t>(CH, nq - c0), ci = c0 / CH;
      const ss_bm25_query* qc = q + c0;
      MatchChunk& mc = plans[ci];
      MatchBatchInfo b;
      // (SS_RT_TOPK without facets: nothing reads a match set)
      int rp = qf || rt != SS_RT_TOPK ? match_prepare(s, nb, qc, &mc, &b) : SS_ENOTSUP;
      if (rp == SS_OK && b.gated) rp = SS_ENOTSUP;  // (a union under a field filter: the facet entries refuse it, the search runs it alone)
      if (rp != SS_OK && (rp != SS_ENOTSUP || qf)) return rp;
      const bool sets = rp == SS_OK;
      const bool fast_search = sets && rt == SS_RT_TOPKCOUNT && !mc.tier.any_tiered && !mc.any_phrase() && !b.any_filter && !b.any_frequent;
      const bool fast_count = sets && rt == SS_RT_COUNT;
      if (sets && (qf || fast_search || fast_count)) {
        SS_HIP(hipMemsetAsync(d_total, 0, (size_t)nb * 8, s->stream));
        SS_HIP(hipMemsetAsync(d_bits, 0, (size_t)nb * groups * 8, s->stream));
        SS_TRY(each_chunk_rows(s, nb, each.filter_begin + c0, each.filters, &each_plans[ci], W + o_sets, (uint32_t*)(W + o_X), (uint32_t*)(W + o_rowof), groups));
        SS_TRY(match_enqueue(s, nb, qc, mc, 0, nullptr, false, d_q, (ss_bm25_query*)(W + o_sub), (ss_bm25_query*)(W + o_ph), d_bits, d_total));
        SS_TRY(ssi_match_exclude_rows(s, nb, d_bits, (const unsigned long long*)(W + o_X), (const uint32_t*)(W + o_rowof), groups, d_total,
                                      fast_search ? (unsigned long long*)(W + o_Xq) : nullptr, s->stream));
        if (qf)
          SS_TRY(ssi_facet_count_multi(s, nb, d_bits, qf->n_facets, qf->facet_offset, qf->facet_type, qf->n_buckets, qf->bases, d_bounds,
                                       d_counts + (size_t)c0 * qf->stride, s->stream));
      }
      bool done = false;
      if (fast_search) {  // ONE batched search, every query under its own exclusion bitmap
        ExclSwap sw(s, (uint32_t*)(W + o_Xq), groups * 2);
        sw.per_query();
        const int rc = ssi_bm25_search(s, nb, d_q, k, SS_RT_TOPK, (uint32_t*)(W + o_od) + (size_t)c0 * k, (float*)(W + o_os) + (size_t)c0 * k,
                                       (uint32_t*)(W + o_oc) + c0, (uint64_t*)(W + o_stot), b.has_and, b.has_or, b.nt_max, b.np_max, b.all_probed, s->stream,
                                       b.any_frequent, false, b.any_filter, b.uniform, b.gated, b.nn_max);
        if (rc != SS_OK && rc != SS_ENOTSUP) return rc;
        done = rc == SS_OK;  // (SS_ENOTSUP: not the pruned kernel's batch -- query by query below)
      } else if (fast_count) {
        SS_HIP(hipMemsetAsync(W + o_oc + (size_t)c0 * 4, 0, (size_t)nb * 4, s->stream));
        done = true;
      }
      if (done) SS_HIP(hipMemcpyAsync(W + o_ot + (size_t)c0 * 8, d_total, (size_t)nb * 8, hipMemcpyDeviceToDevice, s->stream));
      else
        for (uint32_t i = 0; i < nb; i++) SS_TRY(direct_one(c0 + i));
      batched[ci] = done ? 1 : 0;
    }
    for (uint32_t c0 = 0; c0 < nq; c0 += CH) {
      if (!batched[c0 / CH]) continue;
      const uint32_t nb = std::min<uint32_t>(CH, nq - c0);
      if (kk) {
        SS_HIP(hipMemcpyAsync(out_doc + (size_t)c0 * kk, W + o_od + (size_t)c0 * kk * 4, (size_t)nb * kk * 4, hipMemcpyDeviceToHost, s->stream));
        SS_HIP(hipMemcpyAsync(out_score + (size_t)c0 * kk, W + o_os + (size_t)c0 * kk * 4, (size_t)nb * kk * 4, hipMemcpyDeviceToHost, s->stream));
      }
      SS_HIP(hipMemcpyAsync(out_count + c0, W + o_oc + (size_t)c0 * 4, (size_t)nb * 4, hipMemcpyDeviceToHost, s->stream));
      SS_HIP(hipMemcpyAsync(out_total + c0, W + o_ot + (size_t)c0 * 8, (size_t)nb * 8, hipMemcpyDeviceToHost, s->stream));
    }
    if (qf) SS_HIP(hipMemcpyAsync(qf->out_counts, d_counts, (size_t)nq * qf->stride * 8, hipMemcpyDeviceToHost, s->stream));
    return SS_OK;
  };
  int rc = run();
  if (hipStreamSynchronize(s->stream) != hipSuccess && rc == SS_OK) rc = SS_EDEVICE;  // (also on an error: the plans and the caller's arrays are being read)
  return rc;
}

int ss_bm25_search_each(ss_shard* s, uint32_t nq, const ss_bm25_query* queries, uint32_t n_sorts, const ss_result_sort* sorts, uint32_t k, uint32_t rt,
                        const uint32_t* filter_begin, const ss_facet_filter* filters, uint32_t n_facets, const uint32_t* facet_offset,
                        const uint32_t* facet_type, const uint32_t* n_buckets, const uint64_t* range_lower_bounds, const ss_facet_point* bases,
                        uint32_t* out_doc, float* out_score, uint32_t* out_count, uint64_t* out_total, uint64_t* out_facet_counts) {
  // the checks of ss_bm25_search_sorted_facets, in its order
  if (rt > SS_RT_TOPKCOUNT) return SS_EINVAL;
  if (!s || !queries || !out_count || !out_total || !filter_begin) return SS_EINVAL;
  if (n_sorts && (nq == 0 || !sorts)) return SS_EINVAL;
  if (rt != SS_RT_COUNT && (k == 0 || !out_doc || !out_score)) return SS_EINVAL;
  if (n_sorts > SS_MAX_SORT_FIELDS) return SS_ENOTSUP;
  for (uint32_t f = 0; f < n_sorts; f++)
    if (sorts[f].facet_type > SS_FACET_POINT) return SS_EINVAL;
  QueryFacets qf;
  SS_TRY(query_facets_check(n_facets, facet_offset, facet_type, n_buckets, range_lower_bounds, bases, out_facet_counts, &qf));
  for (uint32_t i = 0; i < nq; i++) {
    if (filter_begin[i + 1] < filter_begin[i] || filter_begin[i + 1] - filter_begin[i] > SS_MAX_FACET_FILTERS) return SS_EINVAL;
    if (filter_begin[i + 1] > filter_begin[i] && !filters) return SS_EINVAL;
  }
  if (!s->d_post) return SS_ESTATE;
  if (nq == 0) return SS_OK;
  const uint32_t kk = rt == SS_RT_COUNT ? 0u : k;
  // who runs alone through the single-filter entry: everybody on a deep page, else the queries with an SS_FACET_IDS_EXTERN filter
  const bool deep = rt != SS_RT_COUNT && k > SS_MAX_K;
  std::vector<uint8_t> slow(nq, deep ? 1 : 0);
  uint32_t n_slow = deep ? nq : 0;
  if (!deep)
    for (uint32_t i = 0; i < nq; i++) {
      for (uint32_t j = filter_begin[i]; j < filter_begin[i + 1] && !slow[i]; j++) slow[i] = ssi_filter_is_extern(filters[j]) ? 1 : 0;
      n_slow += slow[i];
    }
  if (n_slow < nq) {
    const uint32_t n = nq - n_slow;
    // the batched queries back to back (all of them, as a rule: then the caller's arrays serve as they are)
    std::vector<ss_bm25_query> cq;
    std::vector<uint32_t> cb, at, c_doc, c_cnt;
    std::vector<ss_facet_filter> cf;
    std::vector<float> c_score;
    std::vector<uint64_t> c_tot, c_fc;
    if (n_slow) {
      cb.push_back(0);
      for (uint32_t i = 0; i < nq; i++) {
        if (slow[i]) continue;
        at.push_back(i);
        cq.push_back(queries[i]);
        cf.insert(cf.end(), filters + filter_begin[i], filters + filter_begin[i + 1]);
        cb.push_back((uint32_t)cf.size());
      }
      c_doc.resize((size_t)n * kk); c_score.resize((size_t)n * kk); c_cnt.resize(n); c_tot.resize(n); c_fc.resize((size_t)n * qf.stride);
    }
    const ss_bm25_query* q_ = n_slow ? cq.data() : queries;
    const EachSets es{n_slow ? cb.data() : filter_begin, n_slow ? cf.data() : filters};
    uint32_t* o_doc = n_slow ? c_doc.data() : out_doc;
    float* o_score = n_slow ? c_score.data() : out_score;
    uint32_t* o_cnt = n_slow ? c_cnt.data() : out_count;
    uint64_t* o_tot = n_slow ? c_tot.data() : out_total;
    QueryFacets qf_ = qf;
    if (n_slow) qf_.out_counts = c_fc.data();
    {
      ShardLock g(s);  // (before the image is looked at: a commit swaps its arrays under this lock)
      if (!s->d_post) return SS_ESTATE;
      ss_sort_sources src;
      if (n_sorts) SS_TRY(ssi_sort_resolve(s, n_sorts, sorts, &src));  // SS_ENOTSUP: a string field without a rank table
      if (n_sorts && rt != SS_RT_COUNT)
        SS_TRY(ssi_bm25_search_sorted_locked(s, n, q_, n_sorts, sorts, src, k, 0, nullptr, o_doc, o_score, o_cnt, o_tot, n_facets ? &qf_ : nullptr, &es));
      else
        SS_TRY(bm25_each_unsorted_locked(s, n, q_, k, rt, es, n_facets ? &qf_ : nullptr, o_doc, o_score, o_cnt, o_tot));
    }
    for (uint32_t j = 0; j < (n_slow ? n : 0u); j++) {
      const uint32_t i = at[j];
      if (kk) {
        memcpy(out_doc + (size_t)i * kk, c_doc.data() + (size_t)j * kk, (size_t)kk * 4);
        memcpy(out_score + (size_t)i * kk, c_score.data() + (size_t)j * kk, (size_t)kk * 4);
      }
      out_count[i] = c_cnt[j];
      out_total[i] = c_tot[j];
      if (n_facets) memcpy(out_facet_counts + (size_t)i * qf.stride, c_fc.data() + (size_t)j * qf.stride, qf.stride * 8);
    }
  }
  for (uint32_t i = 0; i < nq; i++) {
    if (!slow[i]) continue;
    const uint32_t nf = filter_begin[i + 1] - filter_begin[i];
    SS_TRY(ss_bm25_search_sorted_facets(s, 1, queries + i, n_sorts, sorts, k, rt, nf, nf ? filters + filter_begin[i] : nullptr, n_facets, facet_offset, facet_type,
                                        n_buckets, range_lower_bounds, bases, out_doc ? out_doc + (size_t)i * kk : nullptr,
                                        out_score ? out_score + (size_t)i * kk : nullptr, out_count + i, out_total + i,
                                        n_facets ? out_facet_counts + (size_t)i * qf.stride : nullptr));
  }
  return SS_OK;
}

// The empty query of a shard (browse.hip; search_iterator_shard, iterator.rs:316-358).  Everything runs on s->stream: the match set of
// "every live doc under the filter" (and its slice counts), the facet counts over it, and then either the page by doc id -- one scan
// of the slice counts and one emit pass -- or, under a sort, ssi_sort_select over a copy of the match set, the two doc sets it leaves
// listed by doc id and composed (facet.hip, the browse instances of the compose kernel); ranks beyond SS_MAX_K in passes, the docs of
// the earlier passes cleared from the match set.  Waits: one, when skip + k <= SS_MAX_K (by doc id: k <= SS_MAX_K); else one for the
// match count -- it bounds the passes and the copy home -- and one for the docs.
int ss_docs_search(ss_shard* s, uint64_t skip, uint32_t k, uint32_t rt, uint32_t doc_ascending, uint32_t n_sorts, const ss_result_sort* sorts,
                   uint32_t n_filters, const ss_facet_filter* filters, uint32_t n_facets, const uint32_t* facet_offset, const uint32_t* facet_type,
                   const uint32_t* n_buckets, const uint64_t* range_lower_bounds, const ss_facet_point* bases, uint32_t* out_doc,
                   uint32_t* out_count, uint64_t* out_total, uint64_t* out_facet_counts) {
  if (!s || !out_count || !out_total || rt > SS_RT_TOPKCOUNT) return SS_EINVAL;
  const bool want_docs = rt != SS_RT_COUNT;
  if (want_docs && (k == 0 || !out_doc)) return SS_EINVAL;
  if (n_sorts > SS_MAX_SORT_FIELDS || (n_sorts && !sorts) || n_filters > SS_MAX_FACET_FILTERS || (n_filters && !filters)) return SS_EINVAL;
  for (uint32_t f = 0; f < n_sorts; f++)
    if (sorts[f].facet_type > SS_FACET_POINT) return SS_EINVAL;
  QueryFacets qf;
  SS_TRY(query_facets_check(n_facets, facet_offset, facet_type, n_buckets, range_lower_bounds, bases, out_facet_counts, &qf));
  const size_t n_bounds = qf.n_bounds, stride = qf.stride;
  ShardLock g(s);  // (before the image is looked at: a commit swaps its arrays under this lock)
  ss_sort_sources src;  // where every sort field's key is read, resolved once for the call
  if (ssi_sort_resolve(s, n_sorts, sorts, &src) != SS_OK) return SS_EINVAL;  // a string sort field without a rank table (ss_facet_set_string_ranks)
  if (!s->d_post) return SS_ESTATE;
  SS_HIP(hipSetDevice(s->device));
  if ((n_sorts || n_filters || n_facets) && !facet_records_cover(s)) return SS_ESTATE;
  if (!sorts_fit_records(s, n_sorts, sorts) || !facets_fit_records(s, qf)) return SS_EINVAL;
  for (uint32_t f = 0; f < n_filters; f++)
    if (filters[f].type > SS_FACET_POINT || (uint64_t)filters[f].offset + ssi_facet_width(filters[f].type) > s->facet_record_size) return SS_EINVAL;

  const uint64_t groups = (uint64_t)s->bm_n_sub * (BM_SUB / 64), n_slices = browse_slices(groups), n_docs = s->bm_n_docs;
  const bool sorted = want_docs && n_sorts != 0, descending = doc_ascending == 0;
  if (groups == 0 || n_docs == 0) {  // an image without docs
    *out_count = 0;
    *out_total = 0;
    if (n_facets) memset(out_facet_counts, 0, stride * 8);
    return SS_OK;
  }
  // ranks wanted: [skip, skip + k) of at most n_docs matches; a sorted page finds the ranks before it too
  const uint64_t reach = skip > UINT64_MAX - k ? UINT64_MAX : skip + k;
  const uint64_t out_cap = !want_docs ? 0 : sorted ? std::min<uint64_t>(reach, n_docs) : std::min<uint64_t>(k, n_docs);
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  // head: [0] matches, [1] matches left to a sorted pass, [2] the compose kernel's copy; [3] as uint32: page / list A / list C / composed counts
  const size_t o_head = 0, o_M = o_head + al(64), o_scnt = o_M + al(groups * 8), o_sbeg = o_scnt + al(n_slices * 4),
               o_E = o_sbeg + al(n_slices * 8), o_B = o_E + (sorted ? al(groups * 8) : 0), o_hist = o_B + (sorted ? al(groups * 8) : 0),
               o_state = o_hist + (sorted ? al(256 * 8) : 0), o_a = o_state + (sorted ? al(64) : 0), o_c = o_a + (sorted ? al(SS_MAX_K * 4) : 0),
               o_out = o_c + (sorted ? al(SS_MAX_K * 4) : 0), o_bounds = o_out + al(out_cap * 4), o_cnt = o_bounds + al(n_bounds * 8),
               need = o_cnt + al(stride * 8);
  SS_TRY(reserve(s, &s->d_facet_ws, &s->facet_ws_cap, need));
  char* W = (char*)s->d_facet_ws;
  unsigned long long *d_head = (unsigned long long*)(W + o_head), *d_M = (unsigned long long*)(W + o_M), *d_sbeg = (unsigned long long*)(W + o_sbeg),
                     *d_E = (unsigned long long*)(W + o_E), *d_B = (unsigned long long*)(W + o_B), *d_counts = (unsigned long long*)(W + o_cnt);
  uint32_t *d_scnt = (uint32_t*)(W + o_scnt), *d_n = (uint32_t*)(d_head + 3), *d_a = (uint32_t*)(W + o_a), *d_c = (uint32_t*)(W + o_c),
           *d_out = (uint32_t*)(W + o_out);
  uint64_t* d_bounds = (uint64_t*)(W + o_bounds);
  SS_HIP(hipMemsetAsync(d_head, 0, 64, s->stream));
  if (n_facets) SS_HIP(hipMemsetAsync(d_counts, 0, stride * 8, s->stream));
  if (n_bounds) SS_HIP(hipMemcpyAsync(d_bounds, range_lower_bounds, n_bounds * 8, hipMemcpyHostToDevice, s->stream));
  int rc = with_facet_filter(s, n_filters, filters, s->stream, [&]() { return ssi_browse_bits(s, d_M, d_scnt, d_head, s->stream); });
  if (rc == SS_OK && n_facets)
    rc = ssi_facet_count_multi(s, 1, d_M, n_facets, facet_offset, facet_type, n_buckets, bases, d_bounds, d_counts, s->stream);
  uint64_t total = 0;
  uint32_t count = 0, h_doc[SS_MAX_K];  // (h_doc: a shallow page's docs on their way home)
  auto hip_ok = [&](hipError_t e) { if (e != hipSuccess && rc == SS_OK) rc = e == hipErrorOutOfMemory ? SS_ENOMEM : SS_EDEVICE; return rc == SS_OK; };
  if (rc == SS_OK && want_docs && !sorted) {
    rc = ssi_browse_select(s, d_M, descending, skip, k, d_scnt, d_sbeg, true, d_out, d_n, s->stream);
    if (rc == SS_OK && k <= SS_MAX_K) {  // a shallow page: the docs come home with the counts, one wait
      if (hip_ok(hipMemcpyAsync(&total, d_head, 8, hipMemcpyDeviceToHost, s->stream)) &&
          hip_ok(hipMemcpyAsync(&count, d_n, 4, hipMemcpyDeviceToHost, s->stream)) &&
          hip_ok(hipMemcpyAsync(h_doc, d_out, (size_t)out_cap * 4, hipMemcpyDeviceToHost, s->stream)) &&
          hip_ok(hipStreamSynchronize(s->stream))) {
        count = (uint32_t)std::min<uint64_t>(count, out_cap);
        memcpy(out_doc, h_doc, (size_t)count * 4);
      }
    } else if (rc == SS_OK) {
      if (hip_ok(hipMemcpyAsync(&total, d_head, 8, hipMemcpyDeviceToHost, s->stream)) &&
          hip_ok(hipMemcpyAsync(&count, d_n, 4, hipMemcpyDeviceToHost, s->stream)) && hip_ok(hipStreamSynchronize(s->stream))) {
        count = (uint32_t)std::min<uint64_t>(count, out_cap);
        if (count) hip_ok(hipMemcpyAsync(out_doc, d_out, (size_t)count * 4, hipMemcpyDeviceToHost, s->stream));
      }
    }
  } else if (rc == SS_OK && sorted) {
    uint64_t n_rank = out_cap;  // ranks [0, n_rank) are found; known to exist once the match count is home
    const bool deep = reach > SS_MAX_K;
    if (deep) {
      if (hip_ok(hipMemcpyAsync(&total, d_head, 8, hipMemcpyDeviceToHost, s->stream))) hip_ok(hipStreamSynchronize(s->stream));
      n_rank = total > skip ? std::min<uint64_t>(n_rank, total) : 0;  // (nobody at rank skip: no pass at all)
    }
    if (rc == SS_OK) hip_ok(hipMemcpyAsync(d_head + 1, d_head, 8, hipMemcpyDeviceToDevice, s->stream));
    for (uint64_t got = 0; rc == SS_OK && got < n_rank;) {
      const uint32_t kk = (uint32_t)std::min<uint64_t>(SS_MAX_K, n_rank - got);
      if (!hip_ok(hipMemcpyAsync(d_E, d_M, groups * 8, hipMemcpyDeviceToDevice, s->stream))) break;
      rc = ssi_sort_select(s, 1, d_E, d_B, nullptr, nullptr, d_head + 1, (unsigned long long*)(W + o_hist), W + o_state, n_sorts, sorts, src, kk, s->stream);
      // list A: all of B (fewer than kk docs); list C: the best kk of the last pivot's tie group by doc id, of which the compose takes kk - |A|
      if (rc == SS_OK) rc = ssi_browse_select(s, d_B, descending, 0, kk, d_scnt, d_sbeg, false, d_a, d_n + 1, s->stream);
      if (rc == SS_OK) rc = ssi_browse_select(s, d_E, descending, 0, kk, d_scnt, d_sbeg, false, d_c, d_n + 2, s->stream);
      if (rc == SS_OK)
        rc = ssi_sort_compose_browse(s, d_a, d_n + 1, d_c, d_n + 2, d_head, n_sorts, sorts, src, kk, !descending, d_out + got, d_n + 3, d_head + 2, s->stream);
      if (rc == SS_OK && got + kk < n_rank) rc = ssi_browse_clear(s, d_M, d_out + got, kk, d_head + 1, s->stream);  // (deep: every pass is full)
      got += kk;
    }
    if (rc == SS_OK && deep) {
      count = n_rank > skip ? (uint32_t)(n_rank - skip) : 0u;
      if (count) hip_ok(hipMemcpyAsync(out_doc, d_out + skip, (size_t)count * 4, hipMemcpyDeviceToHost, s->stream));
    } else if (rc == SS_OK) {  // one pass of skip + k <= SS_MAX_K ranks: the composed count says how many exist
      uint32_t n = 0;
      if (hip_ok(hipMemcpyAsync(&total, d_head, 8, hipMemcpyDeviceToHost, s->stream)) &&
          (n_rank == 0 || (hip_ok(hipMemcpyAsync(&n, d_n + 3, 4, hipMemcpyDeviceToHost, s->stream)) &&
                           hip_ok(hipMemcpyAsync(h_doc, d_out, (size_t)n_rank * 4, hipMemcpyDeviceToHost, s->stream)))) &&
          hip_ok(hipStreamSynchronize(s->stream))) {
        n = (uint32_t)std::min<uint64_t>(n, n_rank);
        count = n > skip ? n - (uint32_t)skip : 0u;
        memcpy(out_doc, h_doc + (count ? skip : 0), (size_t)count * 4);
      }
    }
  } else if (rc == SS_OK) {
    hip_ok(hipMemcpyAsync(&total, d_head, 8, hipMemcpyDeviceToHost, s->stream));
  }
  if (rc == SS_OK && n_facets) hip_ok(hipMemcpyAsync(out_facet_counts, d_counts, stride * 8, hipMemcpyDeviceToHost, s->stream));
  if (hipStreamSynchronize(s->stream) != hipSuccess && rc == SS_OK) rc = SS_EDEVICE;  // (also on an error: the caller's arrays are being read)
  if (rc != SS_OK) return rc;
  *out_count = count;
  *out_total = total;
  return SS_OK;
}

static int facet_values_impl(ss_shard* s, uint32_t n, const uint32_t* doc_ids, uint32_t facet_offset, uint32_t facet_type,
                             const ss_facet_point* point, uint64_t* out_values) {
  if (!s || (n && (!doc_ids || !out_values)) || facet_type > SS_FACET_POINT) return SS_EINVAL;
  if (point && point->unit > SS_POINT_MILES) return SS_EINVAL;
  ShardLock g(s);
  if (!s->d_facets || facet_offset + ssi_facet_width(facet_type) > s->facet_record_size) return SS_ESTATE;
  if (n == 0) return SS_OK;
  SS_HIP(hipSetDevice(s->device));
  SS_TRY(ensure_qstage(s, (size_t)n * 12));
  uint32_t* d_docs = (uint32_t*)((char*)s->d_qstage + (size_t)n * 8);
  unsigned long long* d_out = (unsigned long long*)s->d_qstage;
  SS_HIP(hipMemcpyAsync(d_docs, doc_ids, (size_t)n * 4, hipMemcpyHostToDevice, s->stream));
  SS_TRY(ssi_facet_values(s, d_docs, n, facet_offset, facet_type, d_out, point, s->stream));
  SS_HIP(hipMemcpyAsync(out_values, d_out, (size_t)n * 8, hipMemcpyDeviceToHost, s->stream));
  SS_HIP(hipStreamSynchronize(s->stream));
  return SS_OK;
}
int ss_facet_values(ss_shard* s, uint32_t n, const uint32_t* doc_ids, uint32_t facet_offset, uint32_t facet_type, uint64_t* out_values) {
  return facet_values_impl(s, n, doc_ids, facet_offset, facet_type, nullptr, out_values);  // a Point facet: its Morton codes
}
int ss_facet_point_distances(ss_shard* s, uint32_t n, const uint32_t* doc_ids, uint32_t facet_offset, const ss_facet_point* base,
                             uint64_t* out_values) {
  if (!base) return SS_EINVAL;
  return facet_values_impl(s, n, doc_ids, facet_offset, SS_FACET_POINT, base, out_values);
}

int ss_bm25_search_dev(ss_shard* s, uint32_t nq, const ss_bm25_query* d_q, uint32_t k, uint32_t rt, uint32_t ops_mask,
                       uint32_t* d_out_doc, float* d_out_score, uint32_t* d_out_count, uint64_t* d_out_total,
                       void* stream) {
  return ss_bm25_search_filtered_dev(s, nq, d_q, k, rt, ops_mask, 0, nullptr, d_out_doc, d_out_score, d_out_count, d_out_total, stream);
}

int ss_bm25_search_filtered_dev(ss_shard* s, uint32_t nq, const ss_bm25_query* d_q, uint32_t k, uint32_t rt, uint32_t ops_mask,
                                uint32_t n_filters, const ss_facet_filter* filters, uint32_t* d_out_doc, float* d_out_score,
                                uint32_t* d_out_count, uint64_t* d_out_total, void* stream) {
  if (!s || !d_q || !d_out_count || !d_out_total) return SS_EINVAL;
  if (rt > SS_RT_TOPKCOUNT) return SS_EINVAL;
  if (rt != SS_RT_COUNT && (k == 0 || !d_out_doc || !d_out_score)) return SS_EINVAL;
  if (!s->d_post) return SS_ESTATE;
  ShardLock g(s);
  SS_HIP(hipSetDevice(s->device));
  hipStream_t st = stream ? (hipStream_t)stream : s->stream;
  if (rt != SS_RT_COUNT && k > SS_MAX_K) {
    // a DEEP page (api_deep.hip): the passes are steered from the host, so the queries make one trip there (like the tiered batches
    // below) and the call is synchronous; the page is left in the caller's device arrays, ordered on `st`
    std::vector<ss_bm25_query> hq(nq);
    SS_HIP(hipMemcpyAsync(hq.data(), d_q, (size_t)nq * sizeof(ss_bm25_query), hipMemcpyDeviceToHost, st));
    SS_HIP(hipStreamSynchronize(st));
    std::vector<uint32_t> h_doc((size_t)nq * k), h_cnt(nq);
    std::vector<float> h_score((size_t)nq * k);
    std::vector<uint64_t> h_tot(nq);
    SS_TRY(with_facet_filter(s, n_filters, filters, s->stream, [&]() {
      return ssi_bm25_search_deep_locked(s, nq, hq.data(), k, rt, h_doc.data(), h_score.data(), h_cnt.data(), h_tot.data());
    }));
    SS_HIP(hipMemcpyAsync(d_out_doc, h_doc.data(), h_doc.size() * 4, hipMemcpyHostToDevice, st));
    SS_HIP(hipMemcpyAsync(d_out_score, h_score.data(), h_score.size() * 4, hipMemcpyHostToDevice, st));
    SS_HIP(hipMemcpyAsync(d_out_count, h_cnt.data(), (size_t)nq * 4, hipMemcpyHostToDevice, st));
    SS_HIP(hipMemcpyAsync(d_out_total, h_tot.data(), (size_t)nq * 8, hipMemcpyHostToDevice, st));
    SS_HIP(hipStreamSynchronize(st));  // (the host copies are this frame's)
    return SS_OK;
  }
  if ((ops_mask & (1u << 28)) && s->sp_n) {
    // the batch may name terms of the SPARSE tier: splitting it into its dense and sparse parts is host work, so the queries make
    // one trip to the host (the cost the header states); the answers are left in the caller's device arrays, ordered on `st`
    const uint32_t kk = rt == SS_RT_COUNT ? 0 : k, kw = std::max<uint32_t>(kk, 1);
    std::vector<ss_bm25_query> hq(nq);
    SS_HIP(hipMemcpyAsync(hq.data(), d_q, (size_t)nq * sizeof(ss_bm25_query), hipMemcpyDeviceToHost, st));
    SS_HIP(hipStreamSynchronize(st));
    SS_TRY(ssi_bm25_search_host_queries(s, nq, hq.data(), kk, rt, n_filters, filters));
    if (kk) {
      SS_HIP(hipMemcpyAsync(d_out_doc, s->d_out_doc, (size_t)nq * kw * 4, hipMemcpyDeviceToDevice, s->stream));
      SS_HIP(hipMemcpyAsync(d_out_score, s->d_out_score, (size_t)nq * kw * 4, hipMemcpyDeviceToDevice, s->stream));
    }
    SS_HIP(hipMemcpyAsync(d_out_count, s->d_out_count, (size_t)nq * 4, hipMemcpyDeviceToDevice, s->stream));
    SS_HIP(hipMemcpyAsync(d_out_total, s->d_out_total, (size_t)nq * 8, hipMemcpyDeviceToDevice, s->stream));
    SS_HIP(hipStreamSynchronize(s->stream));  // (this path has made a trip to the host already; nothing of this frame is left in flight)
    return SS_OK;
  }
  return with_facet_filter(s, n_filters, filters, st, [&]() {
    return ssi_bm25_search(s, nq, d_q, rt == SS_RT_COUNT ? 0 : k, rt, d_out_doc, d_out_score, d_out_count, d_out_total,
                           (ops_mask & 1u) != 0, (ops_mask & 2u) != 0 || (ops_mask & 3u) == 0,
                           (ops_mask >> 8) & 0xFFu ? (ops_mask >> 8) & 0xFFu : SS_MAX_QUERY_TERMS,
                           (ops_mask >> 16) & 0xFFu ? (ops_mask >> 16) & 0xFFu
                                                    : ((ops_mask >> 8) & 0xFFu ? (ops_mask >> 8) & 0xFFu : SS_MAX_QUERY_TERMS),
                           // the caller vouches for the probe rows of its terms (ss_bm25_term_probed) unless none were rationed
                           s->bm_probe_rows != 0 && (s->bm_probe_rows >= s->bm_n_terms || (ops_mask & 4u) != 0), st,
                           (ops_mask & 8u) != 0, (ops_mask & 16u) != 0, (ops_mask & 32u) != 0, (ops_mask & 64u) != 0, (ops_mask & 128u) != 0,
                           (ops_mask >> 24) & 0xFu ? (ops_mask >> 24) & 0xFu : 0xFFFFFFFFu);
  });
}

// ------------------------------------------------------------------ cross-shard merge + RRF (search.rs:1875-2119)
int ss_merge_results(int mode, const uint64_t* lex_doc, const float* lex_score, uint32_t n_lex, const uint64_t* vec_doc,
                     const float* vec_score, uint32_t n_vec, uint32_t offset, uint32_t length, uint64_t* out_doc,
                     float* out_score, uint8_t* out_source) {
  if (mode < SS_MODE_LEXICAL || mode > SS_MODE_HYBRID) return SS_EINVAL;
  if ((n_lex && (!lex_doc || !lex_score)) || (n_vec && (!vec_doc || !vec_score))) return SS_EINVAL;
  if (length && (!out_doc || !out_score)) return SS_EINVAL;
  struct R { uint64_t doc; float score; uint8_t src; };
  std::vector<R> res;
  auto by_score_desc = [](const R& a, const R& b) { return a.score > b.score; };
  if (mode == SS_MODE_LEXICAL) {
    for (uint32_t i = 0; i < n_lex; i++) res.push_back({lex_doc[i], lex_score[i], SS_SRC_LEXICAL});
  } else if (mode == SS_MODE_VECTOR) {
    for (uint32_t i = 0; i < n_vec; i++) res.push_back({vec_doc[i], vec_score[i], SS_SRC_VECTOR});
  } else {
    // reciprocal rank fusion, k = 0.6, 0-based ranks over the score-sorted concatenation (search.rs:1962-2035)
    std::vector<R> L, V;
    for (uint32_t i = 0; i < n_lex; i++) L.push_back({lex_doc[i], lex_score[i], SS_SRC_LEXICAL});
    for (uint32_t i = 0; i < n_vec; i++) V.push_back({vec_doc[i], vec_score[i], SS_SRC_VECTOR});
    std::stable_sort(L.begin(), L.end(), by_score_desc);
    std::stable_sort(V.begin(), V.end(), by_score_desc);
    std::unordered_map<uint64_t, size_t> at;
    for (size_t i = 0; i < L.size(); i++) {
      float r = 1.0f / (0.6f + (float)i);
      auto it = at.find(L[i].doc);
      if (it == at.end()) { at.emplace(L[i].doc, res.size()); res.push_back({L[i].doc, r, SS_SRC_LEXICAL}); }
      else res[it->second].score = r;  // AHashMap::insert overwrites
    }
    for (size_t i = 0; i < V.size(); i++) {
      float r = 1.0f / (0.6f + (float)i);
      auto it = at.find(V[i].doc);
      if (it == at.end()) { at.emplace(V[i].doc, res.size()); res.push_back({V[i].doc, r, SS_SRC_VECTOR}); }
      else { res[it->second].score += r; res[it->second].src = SS_SRC_HYBRID; }
    }
    // the reference leaves equal RRF scores in hash order (search.rs:2034); we fix doc id ascending
    std::sort(res.begin(), res.end(), [](const R& a, const R& b) { return a.doc < b.doc; });
  }
  std::stable_sort(res.begin(), res.end(), by_score_desc);  // search.rs:2103-2105
  uint32_t w = 0;
  for (size_t i = offset; i < res.size() && w < length; i++, w++) {
    out_doc[w] = res[i].doc;
    out_score[w] = res[i].score;
    if (out_source) out_source[w] = res[i].src;
  }
  return (int)w;
}

// ------------------------------------------------------------------ measurement hooks
int ss_profile_enable(ss_shard* s, int on) {
  if (!s) return SS_EINVAL;
  ShardLock g(s);
  s->prof.on = on != 0;
  return SS_OK;
}

int ss_profile_read(ss_shard* s, int kernel, uint64_t* launches, double* total_ms, int reset) {
  if (!s || kernel < 0 || kernel > 1) return SS_EINVAL;
  ShardLock g(s);
  SS_HIP(hipSetDevice(s->device));
  for (auto& pr : s->prof.pending[kernel]) {
    SS_HIP(hipEventSynchronize(pr.second));
    float ms = 0.f;
    SS_HIP(hipEventElapsedTime(&ms, pr.first, pr.second));
    s->prof.ms[kernel] += ms;
    s->prof.launches[kernel] += 1;
    (void)hipEventDestroy(pr.first);
    (void)hipEventDestroy(pr.second);
  }
  s->prof.pending[kernel].clear();
  if (launches) *launches = s->prof.launches[kernel];
  if (total_ms) *total_ms = s->prof.ms[kernel];
  if (reset) { s->prof.launches[kernel] = 0; s->prof.ms[kernel] = 0.0; }
  return SS_OK;
}

}  // extern "C"

void ssi_prof_begin(ss_shard* s, int kernel, hipStream_t st, hipEvent_t* e0, hipEvent_t* e1) {
  (void)kernel;
  *e0 = nullptr; *e1 = nullptr;
  if (!s->prof.on) return;
  if (hipEventCreate(e0) != hipSuccess || hipEventCreate(e1) != hipSuccess) { *e0 = *e1 = nullptr; return; }
  (void)hipEventRecord(*e0, st);
}
void ssi_prof_end(ss_shard* s, int kernel, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
  if (!e0 || !e1) return;
  (void)hipEventRecord(e1, st);
  s->prof.pending[kernel].emplace_back(e0, e1);
}
