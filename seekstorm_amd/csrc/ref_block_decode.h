// One posting of one index.bin block, decoded on its own: decode_block of ref_format.hip restated rank by rank, so that a GPU lane (or a
// host loop) can take posting r of a block without walking the postings before it.  A block = one (key, 65 536-doc level) pair: the
// key head's fields + the segment's key-body bytes (layout: ref_format.hip, top).  One indexed field, SingleTerm and n-gram keys.
//
// Shared by hipcc (__host__ __device__) and plain g++ (tests/ref_block_decode_check.cpp): no std::, no allocation.  Every byte is
// bounds-checked against byte_array_len BEFORE it is read; a failed check is an error code, never a read.
//
//   rbd_head_check   the head against the bytes: container type, where pointers and container lie, that they fit
//   rbd_doc_*        doc of rank r: Array directly; Bitmap / Rle by select over prefixes the CALLER supplies (a workgroup scans them in
//                    LDS, a host loop calls rbd_prefix_build)
//   rbd_tf           tf of rank r from its rank/position pointer
// Codes are those of include/seekstorm_hip.h: RBD_EINVAL = SS_EINVAL, RBD_ENOTSUP = SS_ENOTSUP (Delta containers).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RBD_FN __host__ __device__ inline
#else
#define RBD_FN inline
#endif

enum { RBD_OK = 0, RBD_EINVAL = -1, RBD_ENOTSUP = -4 };
constexpr uint32_t RBD_BITMAP_WORDS = 1024u;  // 8192 bytes as 64-bit words

struct rbd_block {
  const uint8_t* a;           // the segment's key bodies (ss_ref_block::byte_array)
  uint64_t len;               // byte_array_len
  uint32_t ctp;               // compression_type_pointer
  uint32_t count;             // posting_count_m1 + 1
  uint32_t pivot;             // pointer_pivot_p_docid
  uint32_t n_comp, comp;      // n-gram key: components of the key (2 / 3) and which one's tf is wanted; SingleTerm: 1 / 0
};
struct rbd_head {
  uint32_t ctype;             // 1 Array, 2 Bitmap, 3 Rle
  uint32_t runs;              // Rle: its runs
  uint64_t range, cont;       // rank_position_pointer_range, compressed_doc_id_range
};

RBD_FN uint32_t rbd_rd16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
RBD_FN uint32_t rbd_rd24(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16); }
RBD_FN uint64_t rbd_rd64(const uint8_t* p) {
  uint64_t v = 0;
  for (int i = 7; i >= 0; i--) v = (v << 8) | p[i];
  return v;
}

RBD_FN int rbd_head_check(const rbd_block& b, rbd_head* h) {
  if (!b.a || b.count == 0u || b.count > 65536u || b.n_comp < 1u || b.n_comp > 3u || b.comp >= b.n_comp) return RBD_EINVAL;
  h->ctype = b.ctp >> 30;
  h->range = b.ctp & 0x3FFFFFFFu;
  h->runs = 0u;
  // pointer array size (intersection.rs:219-226)
  const uint64_t ptr_bytes = (uint64_t)b.pivot * 2u + (b.pivot < b.count ? (uint64_t)(b.count - b.pivot) * 3u : 0u);
  h->cont = h->range + ptr_bytes;
  if (h->cont > b.len) return RBD_EINVAL;
  if (h->ctype == 1u) {
    if (h->cont + (uint64_t)b.count * 2u > b.len) return RBD_EINVAL;
  } else if (h->ctype == 2u) {
    if (h->cont + 8192u > b.len) return RBD_EINVAL;
  } else if (h->ctype == 3u) {
    if (h->cont + 2u > b.len) return RBD_EINVAL;
    h->runs = rbd_rd16(b.a + h->cont);
    if (h->cont + 2u + (uint64_t)h->runs * 4u > b.len) return RBD_EINVAL;
  } else {
    return RBD_ENOTSUP;  // Delta: its writer is disabled in the reference (compress_postinglist.rs:242)
  }
  return RBD_OK;
}

// ---- Array
RBD_FN uint32_t rbd_doc_array(const rbd_block& b, const rbd_head& h, uint32_t r) { return rbd_rd16(b.a + h.cont + 2u * (uint64_t)r); }

// ---- Bitmap: bit d <-> byte d >> 3, bit d & 7.  prefix [RBD_BITMAP_WORDS + 1]: set bits before every 64-bit word, the total last
RBD_FN uint64_t rbd_bitmap_word(const rbd_block& b, const rbd_head& h, uint32_t w) { return rbd_rd64(b.a + h.cont + 8u * (uint64_t)w); }
RBD_FN uint32_t rbd_popcount64(uint64_t x) { return (uint32_t)__builtin_popcountll((unsigned long long)x); }
// the element i with prefix[i] <= r < prefix[i + 1] of a non-decreasing prefix [n + 1] (the caller knows r < prefix[n])
RBD_FN uint32_t rbd_prefix_find(const uint32_t* prefix, uint32_t n, uint32_t r) {
  uint32_t lo = 0u, hi = n;  // answer in [lo, hi)
  while (hi - lo > 1u) {
    const uint32_t m = (lo + hi) >> 1;
    if (prefix[m] <= r) lo = m; else hi = m;
  }
  return lo;
}
RBD_FN uint32_t rbd_doc_bitmap(const rbd_block& b, const rbd_head& h, const uint32_t* prefix, uint32_t r) {
  const uint32_t w = rbd_prefix_find(prefix, RBD_BITMAP_WORDS, r);
  const uint64_t x = rbd_bitmap_word(b, h, w);
  uint32_t k = r - prefix[w], at = 0u;  // the k-th set bit of x: halve the window
  for (uint32_t width = 32u; width; width >>= 1) {
    const uint32_t c = rbd_popcount64((x >> at) & ((1ull << width) - 1ull));
    if (k >= c) { k -= c; at += width; }
  }
  return w * 64u + at;
}

// ---- Rle: u16 runs, then per run (u16 start, u16 length): docs start ..= start + length.  prefix [runs + 1]: docs before every run
RBD_FN void rbd_rle_run(const rbd_block& b, const rbd_head& h, uint32_t run, uint32_t* start, uint32_t* length) {
  const uint8_t* p = b.a + h.cont + 2u + 4u * (uint64_t)run;
  *start = rbd_rd16(p);
  *length = rbd_rd16(p + 2);
}
// a run against the level and the run before it: inside 65 536, behind its predecessor's last doc
RBD_FN int rbd_rle_run_check(const rbd_block& b, const rbd_head& h, uint32_t run) {
  uint32_t s, l;
  rbd_rle_run(b, h, run, &s, &l);
  if (s + l > 65535u) return RBD_EINVAL;
  if (run) {
    uint32_t ps, pl;
    rbd_rle_run(b, h, run - 1u, &ps, &pl);
    if (s <= ps + pl) return RBD_EINVAL;
  }
  return RBD_OK;
}
RBD_FN uint32_t rbd_doc_rle(const rbd_block& b, const rbd_head& h, const uint32_t* prefix, uint32_t r) {
  const uint32_t run = rbd_prefix_find(prefix, h.runs, r);
  uint32_t s, l;
  rbd_rle_run(b, h, run, &s, &l);
  return s + (r - prefix[run]);
}

// The prefixes of a Bitmap (RBD_BITMAP_WORDS + 1 entries) or Rle (runs + 1 entries) block, built serially, with the checks a whole-block
// decode makes on the container: count = popcount / sum of runs, runs ascending and inside the level.  Array: nothing to build.
RBD_FN int rbd_prefix_build(const rbd_block& b, const rbd_head& h, uint32_t* prefix) {
  if (h.ctype == 2u) {
    uint32_t n = 0u;
    for (uint32_t w = 0; w < RBD_BITMAP_WORDS; w++) { prefix[w] = n; n += rbd_popcount64(rbd_bitmap_word(b, h, w)); }
    prefix[RBD_BITMAP_WORDS] = n;
    return n == b.count ? RBD_OK : RBD_EINVAL;
  }
  if (h.ctype == 3u) {
    uint32_t n = 0u;
    for (uint32_t run = 0; run < h.runs; run++) {
      if (rbd_rle_run_check(b, h, run)) return RBD_EINVAL;
      uint32_t s, l;
      rbd_rle_run(b, h, run, &s, &l);
      prefix[run] = n;
      n += l + 1u;
    }
    prefix[h.runs] = n;
    return n == b.count ? RBD_OK : RBD_EINVAL;
  }
  return RBD_OK;
}

// doc of rank r, whatever the container, with the per-posting checks: ascending (Array: against the neighbour's doc; Bitmap and Rle
// ascend by construction once their prefixes passed) and inside the level's level_docs docs
RBD_FN int rbd_doc(const rbd_block& b, const rbd_head& h, const uint32_t* prefix, uint32_t r, uint32_t level_docs, uint32_t* doc) {
  uint32_t d;
  if (h.ctype == 1u) {
    d = rbd_doc_array(b, h, r);
    if (r && d <= rbd_doc_array(b, h, r - 1u)) return RBD_EINVAL;
  } else if (h.ctype == 2u) {
    d = rbd_doc_bitmap(b, h, prefix, r);
  } else {
    d = rbd_doc_rle(b, h, prefix, r);
  }
  if (d >= level_docs) return RBD_EINVAL;
  *doc = d;
  return RBD_OK;
}

// ---- tf of rank r from its rank/position pointer (add_result.rs:2044-2180)
// read_singlefield_value (add_result.rs:2584-2606): 1-3 bytes, 7 bits each, most significant group first, the LAST byte carries the stop
// bit 0x80; *size = its bytes
RBD_FN bool rbd_read_vint(const uint8_t* a, uint64_t len, uint64_t pos, uint32_t* out, uint32_t* size) {
  if (pos >= len) return false;
  const uint32_t v = a[pos];
  if (v & 0x80u) { *out = v & 0x7Fu; *size = 1u; return true; }
  if (pos + 1u >= len) return false;
  const uint32_t b2 = a[pos + 1u];
  if (b2 & 0x80u) { *out = ((v & 0x7Fu) << 7) | (b2 & 0x7Fu); *size = 2u; return true; }
  if (pos + 2u >= len) return false;
  *out = ((v & 0x7Fu) << 14) | ((b2 & 0x7Fu) << 7) | (a[pos + 2u] & 0x7Fu);
  *size = 3u;
  return true;
}
// a record behind a non-embedded pointer: [n-gram keys: tf of each component,] positions count, positions
RBD_FN bool rbd_record_tf(const rbd_block& b, const rbd_head& h, uint64_t back, uint32_t* tf) {
  if (back > h.range) return false;
  uint64_t pos = h.range - back;
  for (uint32_t c = 0; c < b.n_comp; c++) {
    uint32_t v, size;
    if (!rbd_read_vint(b.a, b.len, pos, &v, &size)) return false;
    if (c == b.comp) { *tf = v; return true; }
    pos += size;
  }
  return false;
}
RBD_FN int rbd_tf(const rbd_block& b, const rbd_head& h, uint32_t r, uint32_t* tf_out) {
  const bool ngram = b.n_comp > 1u;
  uint32_t tf = 0u;
  if (r < b.pivot) {  // 2-byte pointer
    const uint64_t at = h.range + (uint64_t)r * 2u;
    if (at + 2u > b.len) return RBD_EINVAL;
    const uint32_t p = rbd_rd16(b.a + at);
    if (p & 0x8000u) {  // embedded: 10 -> one position, 11 -> two
      if (ngram) return RBD_EINVAL;  // n-gram postings are never embedded (index_posting.rs:445)
      tf = (p >> 14) == 2u ? 1u : 2u;
    } else if (!rbd_record_tf(b, h, p & 0x7FFFu, &tf)) {
      return RBD_EINVAL;
    }
  } else {  // 3-byte pointer
    const uint64_t at = h.range + (uint64_t)r * 3u - b.pivot;
    if (at + 3u > b.len) return RBD_EINVAL;
    const uint32_t p = rbd_rd24(b.a + at);
    if (p & 0x800000u) {  // embedded: 100 / 101 / 110 / 111 -> 1..4 positions
      if (ngram) return RBD_EINVAL;
      tf = (p >> 21) - 3u;
    } else if (!rbd_record_tf(b, h, p & 0x7FFFFFu, &tf)) {
      return RBD_EINVAL;
    }
  }
  if (tf == 0u || tf > 65535u) return RBD_EINVAL;  // positions_count >= 1 always; component tfs likewise
  *tf_out = tf;
  return RBD_OK;
}
