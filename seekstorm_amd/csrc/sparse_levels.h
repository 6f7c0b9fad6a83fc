// The sparse tier of an image that grows level by level (ss_bm25_append_level + ss_bm25_append_sparse_level; commit.rs:142-148).
// A commit changes the shard's average document length, and with it every BM25 weight (commit.rs recomputes bm25_component_cache): the
// tier therefore keeps the tf of every sparse posting beside its (code | doc) word and re-codes the postings on the device after a
// commit.  That state -- the tf array and the per-list starts of the positions pool -- lives beside the shard, keyed by it.
// One indexed field: one tf per posting, u16 positions.  Several (ss_bm25_commit_level_fields + ss_bm25_commit_sparse_level_fields): one
// merged posting per (term, doc) with a ROW of tfs, one per field (0 = absent), field-tagged u32 positions; the re-coding then follows the
// merged lists' scale as well as the average length.
#pragma once
#include "ss_common.h"

bool ssi_bm25_sparse_levels_has(const ss_shard* s);
// the tf row of its postings: 0 = no such tier, 1 = one indexed field, else the indexed fields of ssi_bm25_commit_sparse_level_fields
uint32_t ssi_bm25_sparse_levels_fields(const ss_shard* s);
// the tf of every posting of a tier of ONE indexed field that takes levels (device, [postings]); nullptr: no such tier
const uint16_t* ssi_bm25_sparse_levels_tf(const ss_shard* s);
void ssi_bm25_sparse_levels_drop(const ss_shard* s);
// every sparse posting's code again from its tf, the image's d_doclen and d_comp (after a commit moved the average length)
// (SS_ENOTSUP: a weight the code cannot hold, bm_w_codable)
int ssi_bm25_sparse_levels_recode(ss_shard* s, hipStream_t st);
// the same weights under the component cache and length bytes of `img` (a commit's new dense image), counted and not written: SS_ENOTSUP
// when one has no code -- the commit is refused before the image is swapped in
int ssi_bm25_sparse_levels_check(ss_shard* s, const ss_shard* img, hipStream_t st);
// the postings of the rare terms in `level` (the level the dense image committed last): list i continues sparse list i (ascending
// docs, all behind the list's last), lists past the tier's current count are new terms; a level the tier has seen already is
// replaced.  Caller holds s->mu, the device is idle.
int ssi_bm25_append_sparse_level(ss_shard* s, uint32_t level, uint32_t n_lists, const uint64_t* offs, const uint32_t* docs, const uint16_t* tfs,
                                 const uint16_t* npos, const uint16_t* positions, uint64_t n_positions);
// ... of an image with SEVERAL indexed fields whose levels came through ss_bm25_commit_level_fields: entries (doc, field, tf) sorted by
// (doc, field) inside a list; the tier keeps one merged posting per (list, doc) with the tf of every field beside it (mf_sparse_level.h),
// positions field-tagged in 32 bits.  SS_ESTATE: no such image, or a tier of whole lists; SS_ENOTSUP: an image without merged lists, a
// weight the code cannot hold.  Caller holds s->mu, the device is idle.
int ssi_bm25_commit_sparse_level_fields(ss_shard* s, uint32_t level, uint32_t n_lists, const uint64_t* offs, const uint32_t* docs, const uint8_t* fields,
                                        const uint16_t* tfs, const uint16_t* npos, const uint16_t* positions, uint64_t n_positions);

// A tier that takes levels, built ASIDE from whole lists (ss_bm25_open_index_bin_levels: the rare keys of an index.bin, their docs from
// the first level on) and swapped in with the image it was coded against.  d_post holds the docs (its codes: ssi_bm25_sparse_tier_code);
// h_last_n / h_last_pos = per list what `last_level` brought, which a re-commit of that level replaces (ss_bm25_append_sparse_level).
struct ss_sparse_tier_built {
  uint32_t n_lists = 0;
  std::vector<uint64_t> h_base;      // [n_lists + 1]
  uint64_t* d_base = nullptr;        // [n_lists + 1]
  uint64_t* d_post = nullptr;        // [postings]
  uint16_t* d_tf = nullptr;          // [postings]
  bool with_pos = false;             // positions (u16): per posting the END of its positions in the pool, the pool, the lists' starts
  uint64_t* d_pos_end = nullptr;
  uint16_t* d_pos = nullptr;
  uint64_t pos_n = 0;
  std::vector<uint64_t> h_pbase;     // [n_lists + 1]
  uint32_t last_level = 0;
  std::vector<uint32_t> h_last_n, h_last_pos;
};
// every posting's code under the length bytes and component cache of `img` (SS_ENOTSUP: a weight the code cannot hold)
int ssi_bm25_sparse_tier_code(ss_sparse_tier_built* T, const ss_shard* img, hipStream_t st);
// the tier becomes the shard's (whose own is gone: ssi_bm25_free); T is left empty.  Caller holds s->mu, the device is idle.
void ssi_bm25_sparse_tier_take(ss_shard* s, ss_sparse_tier_built* T);
void ssi_bm25_sparse_tier_drop(ss_sparse_tier_built* T);  // frees what T still owns
