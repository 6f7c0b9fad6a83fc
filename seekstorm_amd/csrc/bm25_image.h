// The dense BM25 image of an ss_shard and the raw levels an incremental image is rebuilt from: what they own, enumerated ONCE.  Whoever
// frees, releases, takes or empties an image or a level goes through these; a new array of the image is added to bm_image_members only.
#pragma once
#include "ss_common.h"

// f(member pointer) for every device array of the dense image; bm_image_arrays: f(the array of s), by reference
template <class F>
inline void bm_image_members(F f) {
  f(&ss_shard::d_post); f(&ss_shard::d_term_base); f(&ss_shard::d_sub_off); f(&ss_shard::d_comp); f(&ss_shard::d_probe);
  f(&ss_shard::d_probe_z); f(&ss_shard::d_probe_row); f(&ss_shard::d_umax); f(&ss_shard::d_submax); f(&ss_shard::d_boost);
  f(&ss_shard::d_pos); f(&ss_shard::d_pos32); f(&ss_shard::d_pos_off); f(&ss_shard::d_pos_base); f(&ss_shard::d_doclen);
}
template <class F>
inline void bm_image_arrays(ss_shard* s, F f) { bm_image_members([&](auto m) { f(s->*m); }); }

// an image nobody owns the arrays of any more: pointers null, counts and host copies empty
inline void bm_image_clear_fields(ss_shard* s) {
  bm_image_arrays(s, [](auto*& p) { p = nullptr; });
  s->probe_pool_begin = 0; s->probe_pool_rows = 0; s->pool_list.clear(); s->pool_tick.clear();
  s->h_probe_row.clear(); s->bm_probe_rows = 0;
  s->bm_n_docs = 0; s->bm_n_terms = 0; s->bm_n_sub = 0; s->bm_n_post = 0; s->bm_n_fields = 1; s->bm_merged = false;
  s->h_df.clear(); s->h_df_real.clear(); s->h_boost.clear(); s->bm_n_post_pad = 0; s->bm_partmax = false;
}
// the one-field image a rebuild left in `src` becomes dst's (whose own arrays are gone already); src is left empty
inline void bm_image_take(ss_shard* dst, ss_shard* src) {
  bm_image_members([&](auto m) { dst->*m = src->*m; });
  dst->bm_n_docs = src->bm_n_docs; dst->bm_n_terms = src->bm_n_terms; dst->bm_n_sub = src->bm_n_sub; dst->bm_n_post = src->bm_n_post;
  dst->bm_n_post_pad = src->bm_n_post_pad; dst->bm_avgdl = src->bm_avgdl; dst->bm_partmax = src->bm_partmax; dst->bm_probe_rows = src->bm_probe_rows;
  dst->probe_pool_begin = src->probe_pool_begin; dst->probe_pool_rows = src->probe_pool_rows;
  dst->h_df.swap(src->h_df); dst->h_probe_row.swap(src->h_probe_row); dst->pool_list.swap(src->pool_list); dst->pool_tick.swap(src->pool_tick);
  dst->bm_n_fields = 1; dst->bm_merged = false; dst->pool_clock = 0;
  bm_image_clear_fields(src);
}

// f(p) on every device array of a raw level, by reference
template <class F>
inline void raw_level_arrays(ss_raw_level& L, F f) { f(L.d_off); f(L.d_doc); f(L.d_tf); f(L.d_npos); f(L.d_prel); f(L.d_tpos); f(L.d_pos); }
inline void raw_level_free(ss_raw_level& L) { raw_level_arrays(L, [](auto*& p) { if (p) (void)hipFree(p); p = nullptr; }); }

// the positions of a level's postings as the host prepared them: per posting its count and the positions of the term's earlier postings
// of the level, per term (+ 1) its first position, and the caller's positions themselves
struct raw_level_positions { const uint16_t* npos; const uint32_t* prel; const uint64_t* tpos; const uint16_t* positions; uint64_t n_positions; };

// A level's postings (CSR; offs need not start at 0) -> the device arrays of L, on `st`, which is idle again on return: the caller's
// arrays are free.  pos: null = a level without positions.  On failure nothing stays allocated: SS_ENOMEM / SS_EDEVICE.
inline int raw_level_upload(ss_raw_level& L, const uint64_t* offs, const uint32_t* docs, const uint16_t* tfs, uint32_t n_terms,
                            const raw_level_positions* pos, hipStream_t st) {
  const uint64_t np = offs[n_terms] - offs[0], np1 = std::max<uint64_t>(np, 1), nt1 = (uint64_t)n_terms + 1;
  std::vector<uint64_t> rel(nt1);
  for (uint32_t t = 0; t <= n_terms; t++) rel[t] = offs[t] - offs[0];
  hipError_t e = hipSuccess;
  auto alloc = [&](auto*& d, uint64_t n) { return (e = hipMalloc(&d, n * sizeof(*d))) == hipSuccess; };
  auto copy = [&](auto* d, const auto* h, uint64_t n) { return !n || (e = hipMemcpyAsync(d, h, n * sizeof(*d), hipMemcpyHostToDevice, st)) == hipSuccess; };
  bool ok = alloc(L.d_off, nt1) && alloc(L.d_doc, np1) && alloc(L.d_tf, np1) && copy(L.d_off, rel.data(), nt1) &&
            copy(L.d_doc, np ? docs + offs[0] : docs, np) && copy(L.d_tf, np ? tfs + offs[0] : tfs, np);
  if (ok && pos)
    ok = alloc(L.d_npos, np1) && alloc(L.d_prel, np1) && alloc(L.d_tpos, nt1) && alloc(L.d_pos, std::max<uint64_t>(pos->n_positions, 1)) &&
         copy(L.d_npos, pos->npos, np) && copy(L.d_prel, pos->prel, np) && copy(L.d_tpos, pos->tpos, nt1) &&
         copy(L.d_pos, pos->positions, pos->n_positions);
  if (ok && (e = hipStreamSynchronize(st)) == hipSuccess) return SS_OK;  // (rel dies with this frame)
  raw_level_free(L);
  return e == hipErrorOutOfMemory ? SS_ENOMEM : SS_EDEVICE;
}
