// One committed level of an image with SEVERAL indexed fields (ss_bm25_commit_level_fields), as the host prepares it for the device:
// ONE pass over the level's own entries (term, doc, field, tf), sorted by (doc, field) inside a term.  HOST-ONLY and free of any
// device header, so that a stand-alone program can run it under sanitizers (tests/mf_level_check.cpp).
//   (term, field) lists   foff [n_terms * n_fields + 1], fdoc / ftf: the entries split by field (a stable split keeps docs ascending)
//   merged entries        moff [n_terms + 1], mdoc: the term's distinct docs; mtf [entry][n_fields]: the tf of every field, 0 = absent
//   positions (optional)  pos: the caller's positions in the caller's order, each tagged field << MF_POS_FIELD_SHIFT | position;
//                         mnpos / mprel per merged entry: its positions (all fields) and those of the term's earlier entries of the
//                         level; tpos [n_terms + 1]: the term's first position
// Nothing here depends on whether the image gets merged lists: that is decided per rebuild from the weights of ALL levels.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

constexpr int MF_OK = 0, MF_EINVAL = -1, MF_ENOTSUP = -4;  // (= SS_OK, SS_EINVAL, SS_ENOTSUP; api_image.hip asserts it)
constexpr uint32_t MF_POS_FIELD_SHIFT = 20u;               // (= BM_POS_FIELD_SHIFT)

struct mf_level_host {
  uint32_t n_docs = 0, n_terms = 0, n_fields = 0;
  std::vector<uint64_t> foff;
  std::vector<uint32_t> fdoc;
  std::vector<uint16_t> ftf;
  std::vector<uint64_t> moff;
  std::vector<uint32_t> mdoc;
  std::vector<uint16_t> mtf;
  bool with_pos = false;
  std::vector<uint32_t> pos, mnpos, mprel;
  std::vector<uint64_t> tpos;
};

// offs need not start at 0; docs / fields / tfs / npos are indexed by offs, positions from 0 at entry offs[0].  npos (may be null: tf)
// = positions per entry where that is not its tf.  positions null = a level without positions (npos and n_positions are then ignored).
// MF_EINVAL: offsets descending, a doc outside [level * 65536, + n_level_docs), tf 0, field >= n_fields, entries of a term not
// ascending by (doc, field), the counts' sum != n_positions, positions of an entry not ascending.  MF_ENOTSUP: a term with 2^32
// positions or more in one level.  `out` is meaningless unless MF_OK comes back.
inline int mf_level_prepare(uint32_t level, uint32_t n_level_docs, uint32_t n_fields, uint32_t n_terms, const uint64_t* offs, const uint32_t* docs,
                            const uint8_t* fields, const uint16_t* tfs, const uint16_t* npos, const uint16_t* positions, uint64_t n_positions,
                            mf_level_host* out) {
  if (!offs || !out || n_terms == 0 || n_level_docs == 0 || n_level_docs > 65536u || n_fields == 0 || n_fields > 8) return MF_EINVAL;
  for (uint32_t t = 0; t < n_terms; t++)
    if (offs[t + 1] < offs[t]) return MF_EINVAL;
  const uint64_t e0 = offs[0], n_ent = offs[n_terms] - e0;
  if (n_ent && (!docs || !fields || !tfs)) return MF_EINVAL;
  const bool with_pos = positions != nullptr;
  const uint64_t d_lo = (uint64_t)level * 65536u, d_hi = d_lo + n_level_docs;
  const size_t F = n_fields;
  mf_level_host& L = *out;
  L = mf_level_host();
  L.n_docs = n_level_docs; L.n_terms = n_terms; L.n_fields = n_fields; L.with_pos = with_pos;
  L.foff.assign((size_t)n_terms * F + 1, 0);
  L.moff.assign((size_t)n_terms + 1, 0);
  if (with_pos) L.tpos.assign((size_t)n_terms + 1, 0);
  // pass 1: validate the entries, count the lists
  for (uint32_t t = 0; t < n_terms; t++) {
    uint64_t pc = 0;
    for (uint64_t j = offs[t]; j < offs[t + 1]; j++) {
      if (docs[j] < d_lo || docs[j] >= d_hi || tfs[j] == 0 || fields[j] >= n_fields) return MF_EINVAL;
      const bool first = j == offs[t];
      if (!first && (docs[j] < docs[j - 1] || (docs[j] == docs[j - 1] && fields[j] <= fields[j - 1]))) return MF_EINVAL;
      L.foff[(size_t)t * F + fields[j] + 1]++;
      if (first || docs[j] != docs[j - 1]) L.moff[(size_t)t + 1]++;
      pc += npos ? npos[j] : tfs[j];
    }
    if (with_pos) {
      if (pc >= (1ull << 32)) return MF_ENOTSUP;
      L.tpos[(size_t)t + 1] = pc;
    }
  }
  for (size_t v = 0; v < (size_t)n_terms * F; v++) L.foff[v + 1] += L.foff[v];
  for (size_t t = 0; t < n_terms; t++) L.moff[t + 1] += L.moff[t];
  if (with_pos) {
    for (size_t t = 0; t < n_terms; t++) L.tpos[t + 1] += L.tpos[t];
    if (L.tpos[n_terms] != n_positions) return MF_EINVAL;  // (before a single position is read)
  }
  const uint64_t n_ment = L.moff[n_terms];
  L.fdoc.resize(n_ent); L.ftf.resize(n_ent);
  L.mdoc.resize(n_ment); L.mtf.assign((size_t)n_ment * F, 0);
  if (with_pos) { L.pos.resize(n_positions); L.mnpos.assign(n_ment, 0); L.mprel.assign(n_ment, 0); }
  // pass 2: split by field, derive the merged entries, tag the positions
  for (uint32_t t = 0; t < n_terms; t++) {
    uint64_t cur[8];
    for (size_t f = 0; f < F; f++) cur[f] = L.foff[(size_t)t * F + f];
    uint64_t m = L.moff[t], rel = 0;
    const uint64_t at = with_pos ? L.tpos[t] : 0;
    for (uint64_t j = offs[t]; j < offs[t + 1]; j++) {
      const uint64_t w = cur[fields[j]]++;
      L.fdoc[w] = docs[j];
      L.ftf[w] = tfs[j];
      if (j != offs[t] && docs[j] != docs[j - 1]) m++;
      L.mdoc[m] = docs[j];
      L.mtf[(size_t)m * F + fields[j]] = tfs[j];
      if (!with_pos) continue;
      const uint32_t c = npos ? npos[j] : tfs[j];
      if (j == offs[t] || docs[j] != docs[j - 1]) L.mprel[m] = (uint32_t)rel;
      for (uint32_t x = 0; x < c; x++) {
        if (x && positions[at + rel + x] <= positions[at + rel + x - 1]) return MF_EINVAL;  // ascending inside an entry
        L.pos[at + rel + x] = ((uint32_t)fields[j] << MF_POS_FIELD_SHIFT) | positions[at + rel + x];
      }
      L.mnpos[m] += c;
      rel += c;
    }
  }
  return MF_OK;
}
