// The dense BM25 image of an ss_shard and the raw levels an incremental image is rebuilt from: what they own, enumerated ONCE.  Whoever
// frees, releases, takes or empties an image or a level goes through these; a new array of the image is added to bm_image_members only.
#pragma once
#include "ss_common.h"
#include "mf_level.h"

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

// A committed level of an image with several indexed fields whose levels stay in HBM (ss_bm25_commit_level_fields; beside ss_raw_level
// and the host-kept ss_raw_level_f of ss_common.h): the image -- per-field lists, merged lists, positions -- is rebuilt from them ON THE
// DEVICE (synth.hip ssi_bm25_rebuild_from_raw_fields).  The layout (mf_level.h, where the host prepares it) does not depend on whether
// a rebuild gets merged lists: that follows from the weights of all levels together.
struct ss_raw_level_mf {
  uint32_t n_docs = 0, n_terms = 0, n_fields = 0;
  uint64_t n_ent = 0, n_ment = 0, psum = 0;  // entries (term, doc, field); merged entries (term, doc); decoded length bytes, all fields
  uint64_t* d_foff = nullptr;        // [n_terms * n_fields + 1] CSR over (term, field)
  uint32_t* d_fdoc = nullptr;        // [n_ent] shard-local doc ids, ascending inside a list
  uint16_t* d_ftf = nullptr;
  uint64_t* d_moff = nullptr;        // [n_terms + 1] CSR over terms: the term's distinct docs
  uint32_t* d_mdoc = nullptr;        // [n_ment]
  uint16_t* d_mtf = nullptr;         // [n_ment][n_fields] the tf of every field, 0 = the doc does not hold the term there
  uint8_t* d_doclen = nullptr;       // [n_fields][n_docs] the level's length bytes
  // positions (every level of an image carries them, or none)
  uint32_t* d_pos = nullptr;         // [n_pos] field << BM_POS_FIELD_SHIFT | position, the caller's order
  uint32_t* d_mnpos = nullptr;       // [n_ment] positions of the merged entry, all its fields
  uint32_t* d_mprel = nullptr;       // [n_ment] positions of the term's earlier merged entries IN THIS LEVEL
  uint64_t* d_tpos = nullptr;        // [n_terms + 1] first position of every term in d_pos
  uint64_t n_pos = 0;
  std::vector<uint32_t> h_mdf;       // [n_terms] merged entries per term (the df of idf, summed over the levels on the host)
};
// Those levels of a shard live beside it, keyed by it (as the sparse tier's level state does, sparse_levels.h): raw / boost are guarded
// by the shard mutex; commit_mu is held across a commit, so that commits of one shard run one after the other.  The entry lives from
// the shard's first commit until ssi_mf_levels_drop (ss_shard_destroy); an upload empties it (api_image.hip free_raw_levels).
struct ss_mf_levels {
  std::vector<ss_raw_level_mf> raw;
  std::vector<float> boost;          // the fields' boosts of those levels
  std::mutex commit_mu;
};
ss_mf_levels* ssi_mf_levels(const ss_shard* s, bool create);  // null: the shard has none (and create is false)
void ssi_mf_levels_drop(const ss_shard* s);
// the image of several indexed fields from such levels: per-field lists + merged lists (none where the boosts keep the merged weights
// out of the code's range: positions are then refused, SS_ENOTSUP) + the merged lists' positions; `img` = a scratch ss_shard that
// receives it, with d_boost / h_boost / h_df_real
int ssi_bm25_rebuild_from_raw_fields(const ss_shard* s, const std::vector<ss_raw_level_mf>& levels, uint32_t n_fields, const float* boost, ss_shard* img,
                                     hipStream_t st);

// the image a rebuild of SEVERAL indexed fields left in `src` (ssi_bm25_rebuild_from_raw_fields)
inline void bm_image_take_fields(ss_shard* dst, ss_shard* src) {
  const uint32_t lists = src->bm_n_fields;
  const bool merged = src->bm_merged;
  std::vector<uint64_t> df_real;
  std::vector<float> boost;
  df_real.swap(src->h_df_real); boost.swap(src->h_boost);
  bm_image_take(dst, src);
  dst->bm_n_fields = lists; dst->bm_merged = merged;
  dst->h_df_real.swap(df_real); dst->h_boost.swap(boost);
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

// ... of a level of several indexed fields
template <class F>
inline void raw_level_mf_arrays(ss_raw_level_mf& L, F f) {
  f(L.d_foff); f(L.d_fdoc); f(L.d_ftf); f(L.d_moff); f(L.d_mdoc); f(L.d_mtf); f(L.d_doclen); f(L.d_pos); f(L.d_mnpos); f(L.d_mprel); f(L.d_tpos);
}
inline void raw_level_mf_free(ss_raw_level_mf& L) { raw_level_mf_arrays(L, [](auto*& p) { if (p) (void)hipFree(p); p = nullptr; }); }
inline uint64_t raw_level_mf_bytes(const ss_raw_level_mf& L) {
  const uint64_t F = L.n_fields;
  return ((uint64_t)L.n_terms * F + 1) * 8u + L.n_ent * 6u + ((uint64_t)L.n_terms + 1) * 8u + L.n_ment * (4u + 2u * F) + F * L.n_docs +
         (L.d_tpos ? L.n_pos * 4u + L.n_ment * 8u + ((uint64_t)L.n_terms + 1) * 8u : 0u);
}
// what mf_level_prepare made of a level -> the device arrays of L, on `st`, which is idle again on return.  On failure nothing stays allocated.
inline int raw_level_mf_upload(ss_raw_level_mf& L, const mf_level_host& H, const uint8_t* level_doclen, hipStream_t st) {
  hipError_t e = hipSuccess;
  auto put = [&](auto*& d, const auto* h, uint64_t n) {
    if ((e = hipMalloc(&d, std::max<uint64_t>(n, 1) * sizeof(*d))) != hipSuccess) return false;
    return !n || (e = hipMemcpyAsync(d, h, n * sizeof(*d), hipMemcpyHostToDevice, st)) == hipSuccess;
  };
  L.n_docs = H.n_docs; L.n_terms = H.n_terms; L.n_fields = H.n_fields;
  L.n_ent = H.fdoc.size(); L.n_ment = H.mdoc.size(); L.n_pos = H.with_pos ? H.pos.size() : 0;
  L.h_mdf.resize(H.n_terms);
  for (uint32_t t = 0; t < H.n_terms; t++) L.h_mdf[t] = (uint32_t)(H.moff[t + 1] - H.moff[t]);
  bool ok = put(L.d_foff, H.foff.data(), H.foff.size()) && put(L.d_fdoc, H.fdoc.data(), H.fdoc.size()) && put(L.d_ftf, H.ftf.data(), H.ftf.size()) &&
            put(L.d_moff, H.moff.data(), H.moff.size()) && put(L.d_mdoc, H.mdoc.data(), H.mdoc.size()) && put(L.d_mtf, H.mtf.data(), H.mtf.size()) &&
            put(L.d_doclen, level_doclen, (uint64_t)H.n_fields * H.n_docs);
  if (ok && H.with_pos)
    ok = put(L.d_pos, H.pos.data(), H.pos.size()) && put(L.d_mnpos, H.mnpos.data(), H.mnpos.size()) && put(L.d_mprel, H.mprel.data(), H.mprel.size()) &&
         put(L.d_tpos, H.tpos.data(), H.tpos.size());
  if (ok && (e = hipStreamSynchronize(st)) == hipSuccess) return SS_OK;
  raw_level_mf_free(L);
  return e == hipErrorOutOfMemory ? SS_ENOMEM : SS_EDEVICE;
}

// What a commit allocated before its swap -- the new level's device arrays, the image built aside -- goes back on EVERY way out, an
// exception included (ss_guard turns it into a code), until the swap has taken it over (taken = true); the commit's stream always goes.
template <class F>
struct CommitUndo {
  F undo;
  hipStream_t& st;
  bool taken = false;
  ~CommitUndo() { if (!taken) undo(); if (st) (void)hipStreamDestroy(st); }
};
