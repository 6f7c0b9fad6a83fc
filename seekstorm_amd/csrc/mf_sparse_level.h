// One committed level of the SPARSE TIER of an image with several indexed fields (ss_bm25_commit_sparse_level_fields), as the host
// prepares it for the device: ONE pass over the level's own entries (list, doc, field, tf) of the rare terms, sorted by (doc, field)
// inside a list.  HOST-ONLY and free of any device header, like mf_level.h, so that a stand-alone program can run it under sanitizers
// (tests/mf_sparse_level_check.cpp).  The tier keeps ONE merged posting per (list, doc):
//   merged postings       moff [n_lists + 1], mdoc: the list's distinct docs; mtf [posting][n_fields]: the tf of every field, 0 = absent
//                         (the layout of ss_raw_level_mf::d_mtf; the field mask of a posting is tf_f != 0)
//   positions (optional)  pos: the caller's positions in the caller's order, each tagged field << MF_POS_FIELD_SHIFT | position;
//                         mnpos per posting: its positions (all fields); mpend: their END counted from the list's first position of
//                         the level; lpos [n_lists + 1]: the list's first position in pos
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "mf_level.h"  // MF_OK / MF_EINVAL / MF_ENOTSUP, MF_POS_FIELD_SHIFT

struct mf_sparse_level_host {
  uint32_t n_lists = 0, n_fields = 0;
  std::vector<uint64_t> moff;
  std::vector<uint32_t> mdoc;
  std::vector<uint16_t> mtf;
  bool with_pos = false;
  std::vector<uint32_t> pos, mnpos, mpend;
  std::vector<uint64_t> lpos;
};

// offs need not start at 0; docs / fields / tfs / npos are indexed by offs, positions from 0 at entry offs[0].  npos (may be null: tf)
// = positions per entry where that is not its tf.  positions null = a level without positions (npos and n_positions are then ignored).
// A list may be empty, and so may the whole level.
// MF_EINVAL: no offsets / no lists, offsets descending, a doc outside [level * 65536, + n_level_docs), tf 0, field >= n_fields, entries
// of a list not ascending by (doc, field), the counts' sum != n_positions, positions of an entry not ascending.  MF_ENOTSUP: a list with
// 2^32 positions or more in one level.  `out` is meaningless unless MF_OK comes back.
inline int mf_sparse_level_prepare(uint32_t level, uint32_t n_level_docs, uint32_t n_fields, uint32_t n_lists, const uint64_t* offs,
                                   const uint32_t* docs, const uint8_t* fields, const uint16_t* tfs, const uint16_t* npos, const uint16_t* positions,
                                   uint64_t n_positions, mf_sparse_level_host* out) {
  if (!offs || !out || n_lists == 0 || n_level_docs == 0 || n_level_docs > 65536u || n_fields < 2 || n_fields > 8) return MF_EINVAL;
  for (uint32_t i = 0; i < n_lists; i++)
    if (offs[i + 1] < offs[i]) return MF_EINVAL;
  const uint64_t n_ent = offs[n_lists] - offs[0];
  if (n_ent && (!docs || !fields || !tfs)) return MF_EINVAL;
  const bool with_pos = positions != nullptr;
  const uint64_t d_lo = (uint64_t)level * 65536u, d_hi = d_lo + n_level_docs;
  const size_t F = n_fields;
  mf_sparse_level_host& L = *out;
  L = mf_sparse_level_host();
  L.n_lists = n_lists; L.n_fields = n_fields; L.with_pos = with_pos;
  L.moff.assign((size_t)n_lists + 1, 0);
  if (with_pos) L.lpos.assign((size_t)n_lists + 1, 0);
  // pass 1: validate the entries, count the lists' docs and positions
  for (uint32_t i = 0; i < n_lists; i++) {
    uint64_t pc = 0;
    for (uint64_t j = offs[i]; j < offs[i + 1]; j++) {
      if (docs[j] < d_lo || docs[j] >= d_hi || tfs[j] == 0 || fields[j] >= n_fields) return MF_EINVAL;
      const bool first = j == offs[i];
      if (!first && (docs[j] < docs[j - 1] || (docs[j] == docs[j - 1] && fields[j] <= fields[j - 1]))) return MF_EINVAL;
      if (first || docs[j] != docs[j - 1]) L.moff[(size_t)i + 1]++;
      pc += npos ? npos[j] : tfs[j];
    }
    if (with_pos) {
      if (pc >= (1ull << 32)) return MF_ENOTSUP;
      L.lpos[(size_t)i + 1] = pc;
    }
  }
  for (size_t i = 0; i < n_lists; i++) L.moff[i + 1] += L.moff[i];
  if (with_pos) {
    for (size_t i = 0; i < n_lists; i++) L.lpos[i + 1] += L.lpos[i];
    if (L.lpos[n_lists] != n_positions) return MF_EINVAL;  // (before a single position is read)
  }
  const uint64_t n_post = L.moff[n_lists];
  L.mdoc.resize(n_post); L.mtf.assign((size_t)n_post * F, 0);
  if (with_pos) { L.pos.resize(n_positions); L.mnpos.assign(n_post, 0); L.mpend.assign(n_post, 0); }
  // pass 2: the merged postings' tf rows, their position counts and ends, the tagged pool
  for (uint32_t i = 0; i < n_lists; i++) {
    uint64_t m = L.moff[i], rel = 0;
    const uint64_t at = with_pos ? L.lpos[i] : 0;
    for (uint64_t j = offs[i]; j < offs[i + 1]; j++) {
      if (j != offs[i] && docs[j] != docs[j - 1]) m++;
      L.mdoc[m] = docs[j];
      L.mtf[(size_t)m * F + fields[j]] = tfs[j];
      if (!with_pos) continue;
      const uint32_t c = npos ? npos[j] : tfs[j];
      for (uint32_t x = 0; x < c; x++) {
        if (x && positions[at + rel + x] <= positions[at + rel + x - 1]) return MF_EINVAL;  // ascending inside an entry
        L.pos[at + rel + x] = ((uint32_t)fields[j] << MF_POS_FIELD_SHIFT) | positions[at + rel + x];
      }
      L.mnpos[m] += c;
      rel += c;
      L.mpend[m] = (uint32_t)rel;
    }
  }
  return MF_OK;
}
