// Stand-alone check of the POSITIONS functions of seekstorm_amd/csrc/ref_block_decode.h (built by tests/test_ref_block_positions_cpu.py
// with the host compiler under AddressSanitizer and UBSan): every case of the file given as argv[1] is walked RANK BY RANK through
// rbd_npos / rbd_positions in the host decoder's order -- the container first, then the ranks ascending, the block's cap on its positions
// applied as they accumulate -- and compared with what the library's whole-block host decoder (ss_ref_decode_block_positions /
// _ngram_positions) answered for the same bytes: counts and positions, or the refusal code.  Variants of a case truncate its
// byte_array_len or flip one byte; the bytes behind byte_array_len are poisoned while a variant runs.
//
// Every recorded posting that decodes is decoded a second time the way a wave of the device takes it: its record's position bytes 64 at a
// time, value ends and sizes from rbd_chunk_size, the carry from rbd_chunk_carry, the last two bytes of the chunk before carried along --
// that must give the positions rbd_positions gave.
//
// File (little endian): u32 magic, u32 n_cases; per case: u32 ctp, count, pivot, n_comp, body_len; the body; u32 n_variants; per variant:
// u32 kind (0 as is, 1 byte_array_len = a, 2 byte a ^= b), u32 a, u32 b, i32 rc (the host's posting count or its error code), and when
// rc >= 0: u32 n_pos, u16 npos[rc], u16 pos[n_pos].
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../seekstorm_amd/csrc/ref_block_decode.h"

#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/asan_interface.h>
#define POISON(p, n) ASAN_POISON_MEMORY_REGION(p, n)
#define UNPOISON(p, n) ASAN_UNPOISON_MEMORY_REGION(p, n)
#else
#define POISON(p, n) ((void)0)
#define UNPOISON(p, n) ((void)0)
#endif

static std::vector<uint8_t> g_file;
static size_t g_at = 0;
static uint32_t rd32() {
  if (g_at + 4 > g_file.size()) { fprintf(stderr, "case file truncated\n"); exit(2); }
  uint32_t v;
  memcpy(&v, g_file.data() + g_at, 4);
  g_at += 4;
  return v;
}

static uint32_t g_prefix[65537];
static uint16_t g_npos[65536];
static std::vector<uint16_t> g_pos, g_wave;
static uint64_t g_chunked = 0, g_chunk_bad = 0;

// one record the way rbd_pos_long_kernel takes it: 64 bytes at a time, a lane per byte.  want [np]: what rbd_positions gave
static bool chunked_equals(const rbd_block& b, const rbd_head& h, uint32_t r, const uint16_t* want, uint32_t np) {
  uint32_t p, count;
  bool wide;
  uint64_t at;
  if (rbd_pointer(b, h, r, &p, &wide) || rbd_pointer_embedded(p, wide) || rbd_record_area(b, h, p, wide, &at, &count) || count != np) return false;
  g_wave.assign(np, 0);
  uint32_t done = 0, sum = 0, carry = 0, last1 = 0, last2 = 0;
  while (done < np) {
    if (at >= b.len) return false;
    const uint32_t n_valid = (uint32_t)(b.len - at < 64u ? b.len - at : 64u);
    uint32_t byte[64];
    uint64_t stops = 0;
    for (uint32_t l = 0; l < 64u; l++) {
      byte[l] = l < n_valid ? b.a[at + l] : 0u;
      if (l < n_valid && (byte[l] & 0x80u)) stops |= 1ull << l;
    }
    for (uint32_t l = 0; l < n_valid && done < np; l++) {
      const uint32_t size = rbd_chunk_size(stops, l, carry);
      if (!size) continue;
      const uint32_t b1 = l >= 1u ? byte[l - 1u] : last1, b0 = l >= 2u ? byte[l - 2u] : l == 1u ? last1 : last2;
      sum += rbd_position_value(b0, b1, byte[l], size) + 1u;
      if (sum - 1u > 65535u) return false;
      g_wave[done++] = (uint16_t)(sum - 1u);
    }
    if (done < np && n_valid < 64u) return false;
    carry = rbd_chunk_carry(stops, 64u, carry);
    last1 = byte[63]; last2 = byte[62];
    at += 64u;
  }
  return memcmp(g_wave.data(), want, 2u * (size_t)np) == 0;
}

// the whole block through the per-posting functions, in the host decoder's order: the posting count or the first error
static int decode_by_rank(const rbd_block& b, uint64_t* n_pos_out) {
  rbd_head h;
  int rc = rbd_head_check(b, &h);
  if (rc) return rc;
  rc = rbd_prefix_build(b, h, g_prefix);
  if (rc) return rc;
  for (uint32_t r = 0; r < b.count; r++) {
    uint32_t doc;
    if ((rc = rbd_doc(b, h, g_prefix, r, 65536u, &doc))) return rc;
  }
  const uint64_t pos_cap = b.len + 4ull * 65536ull;  // decode_block's: a position takes a byte, an embedded pointer holds four at most
  g_pos.resize((size_t)pos_cap + 4u * 65536u + 8u);  // (embedded positions come on top of the cap)
  uint64_t total = 0;
  for (uint32_t r = 0; r < b.count; r++) {
    uint32_t tf, np, n = 0, p = 0;
    bool wide = false;
    if ((rc = rbd_pointer(b, h, r, &p, &wide))) return rc;
    const bool embedded = rbd_pointer_embedded(p, wide);
    // (the host decoder pushes embedded positions without asking, and refuses a record's position once the block holds pos_cap; it reads
    // a posting's positions before it looks at the range of its tf)
    const uint64_t room = embedded ? 4u : (total < pos_cap ? pos_cap - total : 0u);
    rc = rbd_positions(b, h, r, g_pos.data() + total, (uint32_t)(room < 65535u ? room : 65535u), &n);
    if (rc) return rc;
    if ((rc = rbd_npos(b, h, r, &tf, &np))) return rc;
    if (n != np) return -1000;  // rbd_npos and rbd_positions disagree
    if (!embedded && np) {
      g_chunked++;
      if (!chunked_equals(b, h, r, g_pos.data() + total, np)) g_chunk_bad++;
    }
    g_npos[r] = (uint16_t)np;
    total += np;
  }
  *n_pos_out = total;
  return (int)b.count;
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  fseek(f, 0, SEEK_END);
  const long size = ftell(f);
  fseek(f, 0, SEEK_SET);
  g_file.resize((size_t)size);
  if (fread(g_file.data(), 1, (size_t)size, f) != (size_t)size) { fprintf(stderr, "short read\n"); return 2; }
  fclose(f);
  if (rd32() != 0x32444252u) { fprintf(stderr, "not a case file\n"); return 2; }
  const uint32_t n_cases = rd32();
  uint64_t n_variants_all = 0, n_ok = 0, n_err = 0;
  int failures = 0;
  for (uint32_t c = 0; c < n_cases; c++) {
    rbd_block b;
    b.ctp = rd32(); b.count = rd32(); b.pivot = rd32(); b.n_comp = rd32(); b.comp = 0u;
    const uint32_t body_len = rd32();
    if (g_at + body_len > g_file.size()) { fprintf(stderr, "case file truncated\n"); return 2; }
    const size_t cap = ((size_t)body_len + 8u) & ~(size_t)7u;  // (room for the poisoned tail of the untruncated body, 8-byte granules)
    uint8_t* body = (uint8_t*)malloc(cap);
    memset(body, 0xA5, cap);
    memcpy(body, g_file.data() + g_at, body_len);
    g_at += body_len;
    b.a = body;
    const uint32_t n_variants = rd32();
    for (uint32_t v = 0; v < n_variants; v++, n_variants_all++) {
      const uint32_t kind = rd32(), a = rd32(), x = rd32();
      const int want = (int)rd32();
      uint32_t want_pos = 0;
      const uint8_t* want_bytes = nullptr;  // npos [want], then pos [want_pos] (maybe unaligned in the file)
      if (want >= 0) {
        want_pos = rd32();
        const size_t bytes = 2u * ((size_t)want + want_pos);
        if (g_at + bytes > g_file.size()) { fprintf(stderr, "case file truncated\n"); return 2; }
        want_bytes = g_file.data() + g_at;
        g_at += bytes;
      }
      b.len = kind == 1 ? a : body_len;
      if (b.len > body_len) { fprintf(stderr, "case %u variant %u: length beyond the body\n", c, v); return 2; }
      if (kind == 2) body[a] ^= (uint8_t)x;
      POISON(body + b.len, cap - b.len);
      uint64_t got_pos = 0;
      const int got = decode_by_rank(b, &got_pos);
      UNPOISON(body, cap);
      if (kind == 2) body[a] ^= (uint8_t)x;
      bool same = got == want;
      if (same && want >= 0)
        same = got_pos == want_pos && memcmp(want_bytes, g_npos, 2u * (size_t)want) == 0 &&
               memcmp(want_bytes + 2u * (size_t)want, g_pos.data(), 2u * (size_t)want_pos) == 0;
      (want >= 0 ? n_ok : n_err)++;
      if (!same && failures++ < 20)
        fprintf(stderr, "case %u variant %u (kind %u, %u, %u): the host decoder answered %d (%u positions), the per-posting decoder %d (%llu)%s\n", c, v,
                kind, a, x, want, want_pos, got, (unsigned long long)got_pos, got == want ? " with other counts or positions" : "");
    }
    free(body);
  }
  if (g_at != g_file.size()) { fprintf(stderr, "trailing bytes in the case file\n"); return 2; }
  if (g_chunk_bad) { fprintf(stderr, "%llu records decode differently 64 bytes at a time\n", (unsigned long long)g_chunk_bad); return 1; }
  if (failures) { fprintf(stderr, "%d variants differ\n", failures); return 1; }
  printf("ref_block_positions ok: %u cases, %llu variants (%llu decoded, %llu refused), %llu records also 64 bytes at a time\n", n_cases,
         (unsigned long long)n_variants_all, (unsigned long long)n_ok, (unsigned long long)n_err, (unsigned long long)g_chunked);
  return 0;
}
