// Stand-alone check of the field-vector decoder of seekstorm_amd/csrc/ref_block_decode.h (rbd_field_vec; built by
// tests/test_ref_block_fields_cpu.py with g++ under AddressSanitizer and UBSan): every case of the file given as argv[1] -- a block of an
// index of SEVERAL indexed fields -- is decoded RANK BY RANK with rbd_doc + rbd_field_vec and compared with what the library's whole-block
// host decoder (ss_ref_decode_block_fields[_ngram]) answered for the same bytes, recorded in the file by the test.  Variants of a case
// truncate its byte_array_len or flip one byte; the bytes behind byte_array_len are poisoned while a variant runs, so a read the header
// did not bounds-check is a sanitizer report.
//
// File (little endian): u32 magic, u32 n_cases; per case: u32 ctp, count, pivot, n_comp, comp, n_fields, longest_field_id, body_len; the
// body; u32 n_variants; per variant: u32 kind (0 as is, 1 byte_array_len = a, 2 byte a ^= b), u32 a, u32 b, i32 rc (the host's posting
// count or its error code), and when rc >= 0: u16 docs[rc], u16 tf[rc][n_fields] (0 = the posting does not hold the key in that field).
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
static uint16_t g_docs[65536], g_tfs[65536 * 8];

// the whole block through the per-posting functions: the posting count or the first error
static int decode_by_rank(const rbd_block& b, uint32_t n_fields, uint32_t longest) {
  rbd_head h;
  int rc = rbd_head_check(b, &h);
  if (rc) return rc;
  rc = rbd_prefix_build(b, h, g_prefix);
  if (rc) return rc;
  // (the host decoder walks the whole container before the first pointer: so does this loop)
  for (uint32_t r = 0; r < b.count; r++) {
    uint32_t doc;
    if ((rc = rbd_doc(b, h, g_prefix, r, 65536u, &doc))) return rc;
    g_docs[r] = (uint16_t)doc;
  }
  for (uint32_t r = 0; r < b.count; r++) {
    uint32_t tf[8];
    if ((rc = rbd_field_vec(b, h, r, n_fields, longest, tf))) return rc;
    for (uint32_t f = n_fields; f < 8u; f++)
      if (tf[f]) return -1000;  // (nothing behind n_fields)
    for (uint32_t f = 0; f < n_fields; f++) g_tfs[(size_t)r * n_fields + f] = (uint16_t)tf[f];
  }
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
  if (rd32() != 0x46444252u) { fprintf(stderr, "not a case file\n"); return 2; }
  const uint32_t n_cases = rd32();
  uint64_t n_variants_all = 0, n_ok = 0, n_err = 0;
  int failures = 0;
  for (uint32_t c = 0; c < n_cases; c++) {
    rbd_block b;
    b.ctp = rd32(); b.count = rd32(); b.pivot = rd32(); b.n_comp = rd32(); b.comp = rd32();
    const uint32_t n_fields = rd32(), longest = rd32(), body_len = rd32();
    if (n_fields < 2 || n_fields > 8 || g_at + body_len > g_file.size()) { fprintf(stderr, "case file truncated\n"); return 2; }
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
      const uint8_t* want_bytes = nullptr;  // docs [want], then tf [want][n_fields] (maybe unaligned in the file)
      const size_t want_size = want >= 0 ? 2u * (size_t)want * (1u + n_fields) : 0u;
      if (want >= 0) {
        if (g_at + want_size > g_file.size()) { fprintf(stderr, "case file truncated\n"); return 2; }
        want_bytes = g_file.data() + g_at;
        g_at += want_size;
      }
      b.len = kind == 1 ? a : body_len;
      if (b.len > body_len || (kind == 2 && a >= body_len)) { fprintf(stderr, "case %u variant %u: beyond the body\n", c, v); return 2; }
      if (kind == 2) body[a] ^= (uint8_t)x;
      POISON(body + b.len, cap - b.len);
      const int got = decode_by_rank(b, n_fields, longest);
      UNPOISON(body, cap);
      if (kind == 2) body[a] ^= (uint8_t)x;
      bool same = got == want;
      if (same && want >= 0)
        same = memcmp(want_bytes, g_docs, 2u * (size_t)want) == 0 && memcmp(want_bytes + 2u * (size_t)want, g_tfs, 2u * (size_t)want * n_fields) == 0;
      (want >= 0 ? n_ok : n_err)++;
      if (!same && failures++ < 20)
        fprintf(stderr, "case %u variant %u (kind %u, %u, %u): the host decoder answered %d, the per-posting decoder %d%s\n", c, v, kind, a, x, want,
                got, got == want ? " with other field vectors" : "");
    }
    free(body);
  }
  if (g_at != g_file.size()) { fprintf(stderr, "trailing bytes in the case file\n"); return 2; }
  if (failures) { fprintf(stderr, "%d variants differ\n", failures); return 1; }
  printf("ref_block_fields ok: %u cases, %llu variants (%llu decoded, %llu refused)\n", n_cases, (unsigned long long)n_variants_all,
         (unsigned long long)n_ok, (unsigned long long)n_err);
  return 0;
}
