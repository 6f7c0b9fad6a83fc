// Stand-alone check of seekstorm_amd/csrc/ref_block_decode.h (built by tests/test_ref_block_decode_cpu.py with g++ under
// AddressSanitizer and UBSan): every case of the file given as argv[1] is decoded RANK BY RANK and compared with what the library's
// whole-block host decoder answered for the same bytes (recorded in the file by the test).  Variants of a case truncate its
// byte_array_len or flip one byte; the bytes behind byte_array_len are poisoned while a variant runs, so a read the header did not
// bounds-check is a sanitizer report.
//
// File (little endian): u32 magic, u32 n_cases; per case: u32 ctp, count, pivot, n_comp, comp, body_len; the body; u32 n_variants; per
// variant: u32 kind (0 as is, 1 byte_array_len = a, 2 byte a ^= b, 3 level_docs = a), u32 a, u32 b, i32 rc (the host's posting count or
// its error code), and when rc >= 0: u16 docs[rc], u16 tfs[rc].
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
static uint16_t g_docs[65536], g_tfs[65536];

// the whole block through the per-posting functions: the posting count or the first error
static int decode_by_rank(const rbd_block& b, uint32_t level_docs) {
  rbd_head h;
  int rc = rbd_head_check(b, &h);
  if (rc) return rc;
  rc = rbd_prefix_build(b, h, g_prefix);
  if (rc) return rc;
  for (uint32_t r = 0; r < b.count; r++) {
    uint32_t doc, tf;
    if ((rc = rbd_doc(b, h, g_prefix, r, level_docs, &doc))) return rc;
    if ((rc = rbd_tf(b, h, r, &tf))) return rc;
    g_docs[r] = (uint16_t)doc;
    g_tfs[r] = (uint16_t)tf;
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
  if (rd32() != 0x31444252u) { fprintf(stderr, "not a case file\n"); return 2; }
  const uint32_t n_cases = rd32();
  uint64_t n_variants_all = 0, n_ok = 0, n_err = 0;
  int failures = 0;
  for (uint32_t c = 0; c < n_cases; c++) {
    rbd_block b;
    b.ctp = rd32(); b.count = rd32(); b.pivot = rd32(); b.n_comp = rd32(); b.comp = rd32();
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
      const uint8_t* want_bytes = nullptr;  // docs [want], then tfs [want] (maybe unaligned in the file)
      if (want >= 0) {
        if (g_at + 4u * (size_t)want > g_file.size()) { fprintf(stderr, "case file truncated\n"); return 2; }
        want_bytes = g_file.data() + g_at;
        g_at += 4u * (size_t)want;
      }
      b.len = kind == 1 ? a : body_len;
      if (b.len > body_len) { fprintf(stderr, "case %u variant %u: length beyond the body\n", c, v); return 2; }
      if (kind == 2) body[a] ^= (uint8_t)x;
      POISON(body + b.len, cap - b.len);
      const int got = decode_by_rank(b, kind == 3 ? a : 65536u);
      UNPOISON(body, cap);
      if (kind == 2) body[a] ^= (uint8_t)x;
      bool same = got == want;
      if (same && want >= 0) {
        same = memcmp(want_bytes, g_docs, 2u * (size_t)want) == 0 && memcmp(want_bytes + 2u * (size_t)want, g_tfs, 2u * (size_t)want) == 0;
      }
      (want >= 0 ? n_ok : n_err)++;
      if (!same && failures++ < 20)
        fprintf(stderr, "case %u variant %u (kind %u, %u, %u): the host decoder answered %d, the per-posting decoder %d%s\n", c, v, kind, a, x, want,
                got, got == want ? " with other postings" : "");
    }
    free(body);
  }
  if (g_at != g_file.size()) { fprintf(stderr, "trailing bytes in the case file\n"); return 2; }
  if (failures) { fprintf(stderr, "%d variants differ\n", failures); return 1; }
  printf("ref_block_decode ok: %u cases, %llu variants (%llu decoded, %llu refused)\n", n_cases, (unsigned long long)n_variants_all,
         (unsigned long long)n_ok, (unsigned long long)n_err);
  return 0;
}
