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
//   rbd_npos         ... and how many positions the posting carries (an n-gram key's stand behind its first component)
//   rbd_positions    the posting's positions, absolute, from an embedded pointer or from the record behind the pointer
//   rbd_chunk_*      a record's position bytes taken 64 at a time (a wave of the device; a host loop in the tests)
//   rbd_field_vec    several indexed fields: the tf of every field of rank r (rbd_tf .. rbd_chunk_* above read one-field blocks only)
// Codes are those of include/seekstorm_hip.h: RBD_EINVAL = SS_EINVAL, RBD_ENOTSUP = SS_ENOTSUP (Delta containers).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RBD_FN __host__ __device__ inline
#define RBD_FN_FLAT __host__ __device__ inline __attribute__((always_inline))  // small helpers with out-parameters: inlined, so that those stay in registers
#else
#define RBD_FN inline
#define RBD_FN_FLAT inline
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

// ---- positions of rank r (decode_positions_multiterm_singlefield's embedded_positions / positions_pointer, add_result.rs:2036-2197)
// a POSITION of a record (compress_positions, compress_postinglist.rs:948-976; get_next_position_singlefield / _multifield,
// add_result.rs:36-88): one and two bytes like the VINT above, but the THREE-byte form keeps bit 13 twice -- the writer stores
// delta >> 13, (delta >> 7) & 0x7F, delta & 0x7F and the reader ORs b0 << 13 | b1 << 7 | b2 -- so it is not the count's VINT
RBD_FN uint32_t rbd_position_value(uint32_t b0, uint32_t b1, uint32_t b2, uint32_t size) {  // b2 = the value's last byte, b1 / b0 those before
  return size == 1u ? (b2 & 0x7Fu) : size == 2u ? ((b1 << 7) | (b2 & 0x7Fu)) : ((b0 << 13) | (b1 << 7) | (b2 & 0x7Fu));
}
RBD_FN bool rbd_read_position(const uint8_t* a, uint64_t len, uint64_t pos, uint32_t* out, uint32_t* size) {
  if (pos >= len) return false;
  const uint32_t v = a[pos];
  if (v & 0x80u) { *out = rbd_position_value(0u, 0u, v, 1u); *size = 1u; return true; }
  if (pos + 1u >= len) return false;
  const uint32_t b2 = a[pos + 1u];
  if (b2 & 0x80u) { *out = rbd_position_value(0u, v, b2, 2u); *size = 2u; return true; }
  if (pos + 2u >= len) return false;
  *out = rbd_position_value(v, b2, a[pos + 2u], 3u);
  *size = 3u;
  return true;
}
// the rank/position pointer of rank r: 2 bytes below the pivot, 3 from it on
RBD_FN_FLAT int rbd_pointer(const rbd_block& b, const rbd_head& h, uint32_t r, uint32_t* p, bool* wide) {
  if (r < b.pivot) {
    const uint64_t at = h.range + (uint64_t)r * 2u;
    if (at + 2u > b.len) return RBD_EINVAL;
    *p = rbd_rd16(b.a + at);
    *wide = false;
  } else {
    const uint64_t at = h.range + (uint64_t)r * 3u - b.pivot;
    if (at + 3u > b.len) return RBD_EINVAL;
    *p = rbd_rd24(b.a + at);
    *wide = true;
  }
  return RBD_OK;
}
RBD_FN bool rbd_pointer_embedded(uint32_t p, bool wide) { return (p & (wide ? 0x800000u : 0x8000u)) != 0u; }
// the record behind a non-embedded pointer: where its positions begin (behind the component tfs of an n-gram key and the count) and
// how many there are (1 .. 65 535)
RBD_FN_FLAT int rbd_record_area(const rbd_block& b, const rbd_head& h, uint32_t p, bool wide, uint64_t* at, uint32_t* count) {
  const uint64_t back = p & (wide ? 0x7FFFFFu : 0x7FFFu);
  if (back > h.range) return RBD_EINVAL;
  uint64_t pos = h.range - back;
  uint32_t v = 0u, size;
  for (uint32_t c = 0; c <= (b.n_comp > 1u ? b.n_comp : 0u); c++) {  // (component tfs,) the count
    if (!rbd_read_vint(b.a, b.len, pos, &v, &size)) return RBD_EINVAL;
    pos += size;
  }
  if (v == 0u || v > 65535u) return RBD_EINVAL;
  *at = pos;
  *count = v;
  return RBD_OK;
}
// tf as rbd_tf gives it, and the posting's own positions: the tf for a SingleTerm key; an n-gram key's positions_count behind its first
// component, none behind the others
RBD_FN_FLAT int rbd_npos(const rbd_block& b, const rbd_head& h, uint32_t r, uint32_t* tf_out, uint32_t* npos_out) {
  int rc = rbd_tf(b, h, r, tf_out);
  if (rc != RBD_OK) return rc;
  if (b.n_comp == 1u) { *npos_out = *tf_out; return RBD_OK; }
  *npos_out = 0u;
  if (b.comp != 0u) return RBD_OK;
  uint32_t p;
  bool wide;
  uint64_t at;
  if ((rc = rbd_pointer(b, h, r, &p, &wide)) != RBD_OK) return rc;
  return rbd_record_area(b, h, p, wide, &at, npos_out);  // (rbd_tf refused an embedded pointer of an n-gram key)
}
// The positions of rank r, ABSOLUTE (the first as stored, every later one previous + stored + 1), at most cap of them: *n = how many.
// RBD_ENOTSUP: a position above 65 535; RBD_EINVAL: everything else, more than cap positions among it.  (Component lists of an n-gram
// key other than the first: none.)
RBD_FN int rbd_positions(const rbd_block& b, const rbd_head& h, uint32_t r, uint16_t* out, uint32_t cap, uint32_t* n_out) {
  *n_out = 0u;
  if (b.n_comp > 1u && b.comp != 0u) return RBD_OK;
  uint32_t p, n = 0u, at = 0u;
  bool wide;
  int rc = rbd_pointer(b, h, r, &p, &wide);
  if (rc != RBD_OK) return rc;
  if (rbd_pointer_embedded(p, wide)) {
    if (b.n_comp > 1u) return RBD_EINVAL;
    // widths as decode_positions_multiterm_singlefield unpacks them: 14 | 7 + 7; 21 | 10 + 11 | 7 + 7 + 7 | 5 + 5 + 5 + 6
    uint32_t tf, d0, d1 = 0u, d2 = 0u, d3 = 0u;
    if (!wide) {
      if ((p >> 14) == 2u) { tf = 1u; d0 = p & 0x3FFFu; }
      else { tf = 2u; d0 = (p >> 7) & 0x7Fu; d1 = p & 0x7Fu; }
    } else {
      tf = (p >> 21) - 3u;
      if (tf == 1u) { d0 = p & 0x1FFFFFu; }
      else if (tf == 2u) { d0 = (p >> 11) & 0x3FFu; d1 = p & 0x7FFu; }
      else if (tf == 3u) { d0 = (p >> 14) & 0x7Fu; d1 = (p >> 7) & 0x7Fu; d2 = p & 0x7Fu; }
      else { d0 = (p >> 16) & 0x1Fu; d1 = (p >> 11) & 0x1Fu; d2 = (p >> 6) & 0x1Fu; d3 = p & 0x3Fu; }
    }
    if (tf > cap) return RBD_EINVAL;
    at = d0;
    if (at > 65535u) return RBD_ENOTSUP;
    out[n++] = (uint16_t)at;
    if (tf > 1u) { at += d1 + 1u; out[n++] = (uint16_t)at; }  // (7 + 11 + ... bits: far below 65 536)
    if (tf > 2u) { at += d2 + 1u; out[n++] = (uint16_t)at; }
    if (tf > 3u) { at += d3 + 1u; out[n++] = (uint16_t)at; }
    *n_out = n;
    return RBD_OK;
  }
  uint64_t pos;
  uint32_t count;
  if ((rc = rbd_record_area(b, h, p, wide, &pos, &count)) != RBD_OK) return rc;
  for (uint32_t i = 0; i < count; i++) {
    uint32_t v, size;
    if (!rbd_read_position(b.a, b.len, pos, &v, &size)) return RBD_EINVAL;
    pos += size;
    at = i == 0u ? v : at + v + 1u;
    if (at > 65535u) return RBD_ENOTSUP;
    if (n >= cap) return RBD_EINVAL;
    out[n++] = (uint16_t)at;
    *n_out = n;
  }
  return RBD_OK;
}

// ---- SEVERAL indexed fields: the field vector of rank r -- the tf of every field, 0 where the posting does not hold the key there
// (decode_block_fields / read_field_vec of ref_format.hip restated rank by rank; add_result.rs:1485-2034, 2200-2293).  The vector is
// kept PACKED while it is decoded, 16 bits a field in two 64-bit words (fields 0 - 3, 4 - 7): an array indexed by a field id read from
// the bytes would live in scratch memory on the device.
RBD_FN uint32_t rbd_field_id_bits(uint32_t n_fields) {  // bit length of n_fields - 1 (index.rs:2569-2570)
  uint32_t bits = 0u;
  while ((1u << bits) < n_fields) bits++;
  return bits;
}
struct rbd_fvec { uint64_t lo, hi; int32_t last; };  // last: the highest field stored so far (-1: none)
RBD_FN uint32_t rbd_fvec_tf(const rbd_fvec& v, uint32_t f) { return (uint32_t)((f < 4u ? v.lo >> (16u * f) : v.hi >> (16u * (f - 4u))) & 0xFFFFu); }
// an entry joins the vector: its field inside n_fields and behind the entry before, its tf 1 .. 65 535
RBD_FN_FLAT bool rbd_fvec_put(rbd_fvec* v, uint32_t field, uint32_t tf, uint32_t n_fields) {
  if (field >= n_fields || (int32_t)field <= v->last || tf == 0u || tf > 65535u) return false;
  if (field < 4u) v->lo |= (uint64_t)tf << (16u * field); else v->hi |= (uint64_t)tf << (16u * (field - 4u));
  v->last = (int32_t)field;
  return true;
}
// One written field vector at *pos (read_multifield_vec): only the longest field -- 0x40 set, the count in 6 + 7 (+ 7) bits --, or up to
// eight (field, tf) values of 1 - 3 bytes with FIELD_STOP_BIT_1 / _2 on the last.  *pos moves behind it.  keep: the entries join *v
// and are judged; else the vector is only stepped over, as the host decoder steps over the components in front of the wanted one.
RBD_FN_FLAT bool rbd_read_field_vec(const uint8_t* a, uint64_t len, uint64_t* pos_io, uint32_t id_bits, uint32_t n_fields, uint32_t longest, bool keep,
                                    rbd_fvec* v) {
  uint64_t pos = *pos_io;
  if (pos >= len) return false;
  if (a[pos] & 0x40u) {
    uint32_t c = a[pos++];
    if (c & 0x80u) c &= 0x3Fu;
    else {
      if (pos >= len) return false;
      c = (c & 0x3Fu) << 7;
      const uint32_t c2 = a[pos++];
      if (c2 & 0x80u) c |= c2 & 0x7Fu;
      else {
        if (pos >= len) return false;
        c = (c << 7) | ((c2 & 0x7Fu) << 7) | (a[pos++] & 0x7Fu);
      }
    }
    if (keep && !rbd_fvec_put(v, longest, c, n_fields)) return false;
  } else {
    bool first = true, ok = true;
    for (uint32_t n = 0;; n++) {
      if (pos >= len || n >= 8u) return false;
      uint32_t b = a[pos++];
      const bool field_stop = (b & (first ? 0x20u : 0x40u)) != 0u;
      uint32_t x = b & (first ? 0x1Fu : 0x3Fu);
      if (!(b & 0x80u)) {
        if (pos >= len) return false;
        b = a[pos++];
        x = (x << 7) | (b & 0x7Fu);
        if (!(b & 0x80u)) {
          if (pos >= len) return false;
          b = a[pos++];
          x = (x << 7) | (b & 0x7Fu);
        }
      }
      // (a vector that is malformed as bytes is refused before one whose entries are: both answer RBD_EINVAL)
      if (keep && ok) ok = rbd_fvec_put(v, x & ((1u << id_bits) - 1u), x >> id_bits, n_fields);
      first = false;
      if ((b & 0x80u) && field_stop) break;
    }
    if (!ok) return false;
  }
  *pos_io = pos;
  return true;
}
// The field vector of rank r, packed.  A record behind a non-embedded pointer: the vectors of the components 0 .. comp of an n-gram key
// one after the other, the last one kept (SingleTerm: the posting's own).  Embedded pointers (never an n-gram key's): the 2-byte tags
// 0x8 .. 0xF and the 3-byte tags 0x10 .. 0x1F, field ids in id_bits-wide slots below the tag.
RBD_FN_FLAT int rbd_field_vec_packed(const rbd_block& b, const rbd_head& h, uint32_t r, uint32_t n_fields, uint32_t longest, rbd_fvec* out) {
  if (n_fields < 2u || n_fields > 8u || longest >= n_fields) return RBD_EINVAL;
  const uint32_t id_bits = rbd_field_id_bits(n_fields), id_mask = (1u << id_bits) - 1u;
  rbd_fvec v{0ull, 0ull, -1};
  uint32_t p;
  bool wide;
  const int rc = rbd_pointer(b, h, r, &p, &wide);
  if (rc != RBD_OK) return rc;
  bool ok;
  if (!rbd_pointer_embedded(p, wide)) {
    const uint64_t back = p & (wide ? 0x7FFFFFu : 0x7FFFu);
    if (back > h.range) return RBD_EINVAL;
    uint64_t at = h.range - back;
    ok = true;
    for (uint32_t c = 0; ok && c <= (b.n_comp > 1u ? b.comp : 0u); c++)
      ok = rbd_read_field_vec(b.a, b.len, &at, id_bits, n_fields, longest, c == (b.n_comp > 1u ? b.comp : 0u), &v);
  } else if (b.n_comp > 1u) {
    return RBD_EINVAL;  // n-gram postings are never embedded (index_posting.rs:445)
  } else if (!wide) {  // tag = bits 15 .. 12 (add_result.rs:1606-1737)
    const uint32_t tag = p >> 12, pb = 12u - id_bits, pb2 = 12u - 2u * id_bits;
    if (tag >= 0xCu) ok = rbd_fvec_put(&v, longest, tag >= 0xEu ? 2u : 1u, n_fields);
    else if (tag <= 0xAu) ok = rbd_fvec_put(&v, (p >> pb) & id_mask, tag - 7u, n_fields);
    else ok = rbd_fvec_put(&v, (p >> (pb2 + id_bits)) & id_mask, 1u, n_fields) && rbd_fvec_put(&v, (p >> pb2) & id_mask, 1u, n_fields);
  } else {  // tag = bits 23 .. 19 (add_result.rs:1738-2017)
    const uint32_t tag = p >> 19, pb = 19u - id_bits, pb2 = 19u - 2u * id_bits, pb3 = 19u - 3u * id_bits;
    if (tag >= 0x18u) ok = rbd_fvec_put(&v, longest, ((tag - 0x18u) >> 1) + 1u, n_fields);
    else if (tag <= 0x13u) ok = rbd_fvec_put(&v, (p >> pb) & id_mask, tag - 0x0Fu, n_fields);
    else if (tag <= 0x16u)
      ok = rbd_fvec_put(&v, (p >> (pb2 + id_bits)) & id_mask, tag == 0x16u ? 2u : 1u, n_fields) &&
           rbd_fvec_put(&v, (p >> pb2) & id_mask, tag == 0x15u ? 2u : 1u, n_fields);
    else
      ok = rbd_fvec_put(&v, (p >> (pb3 + 2u * id_bits)) & id_mask, 1u, n_fields) && rbd_fvec_put(&v, (p >> (pb3 + id_bits)) & id_mask, 1u, n_fields) &&
           rbd_fvec_put(&v, (p >> pb3) & id_mask, 1u, n_fields);
  }
  if (!ok) return RBD_EINVAL;
  *out = v;
  return RBD_OK;
}
// ... as the tf of every field: tf_out[f] for f < n_fields, 0 = absent; the entries behind n_fields are 0
RBD_FN int rbd_field_vec(const rbd_block& b, const rbd_head& h, uint32_t r, uint32_t n_fields, uint32_t longest_field_id, uint32_t tf_out[8]) {
  rbd_fvec v;
  const int rc = rbd_field_vec_packed(b, h, r, n_fields, longest_field_id, &v);
  if (rc != RBD_OK) return rc;
  for (uint32_t f = 0; f < 8u; f++) tf_out[f] = rbd_fvec_tf(v, f);
  return RBD_OK;
}

// ---- a record's position bytes, up to 64 consecutive ones at a time.  stops: bit i = byte i of the chunk has bit 7 set; carry: the
// bytes of an unfinished value in front of the chunk (0 .. 2).  A value ends at a stop byte, or at the third byte of a value without
// one (read_position looks at no stop bit there); it is made of that byte and the at most two before it, back to the previous end.
// rbd_chunk_size: bytes of the value that ends at byte i (1 .. 3), 0 where none ends
RBD_FN uint32_t rbd_chunk_size(uint64_t stops, uint32_t i, uint32_t carry) {
  const uint64_t below = i ? stops & (~0ull >> (64u - i)) : 0ull;
  // bytes since the last stop byte (or since the chunk began, plus the carry): whole values of three among them
  const uint32_t d = below ? i - (64u - (uint32_t)__builtin_clzll((unsigned long long)below)) : i + carry;
  if ((stops >> i) & 1ull) return d % 3u + 1u;
  return d % 3u == 2u ? 3u : 0u;
}
// the carry behind a chunk of n bytes (1 .. 64)
RBD_FN uint32_t rbd_chunk_carry(uint64_t stops, uint32_t n, uint32_t carry) {
  const uint32_t i = n - 1u;
  if (rbd_chunk_size(stops, i, carry)) return 0u;
  const uint64_t below = i ? stops & (~0ull >> (64u - i)) : 0ull;
  const uint32_t d = below ? i - (64u - (uint32_t)__builtin_clzll((unsigned long long)below)) : i + carry;
  return d % 3u + 1u;
}
