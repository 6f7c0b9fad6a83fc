// The parsed index.bin handle (ss_index_bin_open, ref_format.hip) and the host decoder of a range of its terms, for the translation
// units that read them: ref_format.hip (the walker, the host decoders, the whole-image uploads) and ref_decode_dev.hip (the open level
// by level, decoded on the device).  Not part of the public ABI: callers hold an opaque ss_index_bin*.
#pragma once
#include <algorithm>
#include <memory>
#include <vector>

#include "ss_common.h"
#include "ss_threads.h"

struct ss_index_bin {
  const uint8_t* bytes = nullptr;
  uint64_t len = 0;
  uint32_t n_fields = 1, key_head_size = 20, seg_bits = 11;
  uint64_t n_docs = 0, positions_sum = 0;
  uint32_t n_ngram_keys = 0;
  uint16_t longest_field_id = 0;
  std::vector<const uint8_t*> doclen;  // per level: indexed_field_count arrays of 65 536 bytes
  struct Blk {
    uint64_t key;
    ss_ref_block b;
    uint8_t n_comp, comp;              // n-gram key: one entry per component term (2 or 3), SingleTerm: 1 / 0
    uint8_t df_byte;                   // posting_count_ngram_{comp+1}_compressed of the key head
  };                                   // (trivially constructible: see NoInitAlloc)
  std::vector<Blk, NoInitAlloc<Blk>> blocks;  // sorted by (key, component, block_id)
  std::vector<uint64_t> keys;          // ascending; term id = index.  An n-gram key appears once per component, in order
  std::vector<uint8_t> term_comp, term_ncomp, term_df_byte;  // per term; df byte of the LAST level (commit.rs:646-653)
  std::vector<uint64_t> term_block_off;
  uint32_t n_dense = 0xFFFFFFFFu;      // ss_index_bin_tier: terms [0, n_dense) go to the dense image, the rest to the sparse tier
};

// decoded postings of the terms [t0, t1): CSR offsets relative to the range, docs / tfs (+ positions and their per-posting counts).
// The arrays are NOT value-initialised (a vector would zero a gigabyte on one thread first): the worker that decodes a range touches
// its pages.
template <class T>
struct RawBuf {
  std::unique_ptr<T[]> p;
  size_t n = 0;
  void alloc(size_t m) { p.reset(new T[std::max<size_t>(m, 1)]); n = m; }
  T* data() { return p.get(); }
  const T* data() const { return p.get(); }
  size_t size() const { return n; }
  T& operator[](size_t i) { return p[i]; }
  const T& operator[](size_t i) const { return p[i]; }
};
struct DecodedRange {
  std::vector<uint64_t> offs;  // [t1 - t0 + 1]
  RawBuf<uint32_t> docs;
  RawBuf<uint16_t> tfs, pos, npos;
};
int ssi_index_bin_decode_range(const ss_index_bin* ix, uint32_t t0, uint32_t t1, bool with_positions, DecodedRange* out);
// ... of an index of SEVERAL indexed fields: the entries (doc, field, tf) of every term, sorted by (doc, field), with the positions of
// every entry in that order and their number per entry (an n-gram key's own stand behind its first component)
struct DecodedFields {
  std::vector<uint64_t> offs;  // [t1 - t0 + 1]
  NoInitVec<uint32_t> docs;
  NoInitVec<uint8_t> fields;
  NoInitVec<uint16_t> tfs, pos, npos;
};
int ssi_index_bin_decode_fields_range(const ss_index_bin* ix, uint32_t t0, uint32_t t1, bool with_positions, DecodedFields* out);
