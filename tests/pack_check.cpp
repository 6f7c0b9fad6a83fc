// Stand-alone check of the packed query form (seekstorm_amd/csrc/bm25_pack.h), built with -fsanitize=address,undefined by
// tests/test_pack_cpu.py: every buffer is a heap block of exactly the size the library would give it, so a write past the end
// is the sanitizer's to report.  Expected layout: worked out here in two passes (W first, then every query at i * stride).
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../seekstorm_amd/csrc/bm25_pack.h"

static uint32_t rnd_state = 12345u;
static uint32_t rnd() { return rnd_state = rnd_state * 1664525u + 1013904223u; }

static ss_bm25_query make_query(uint32_t np, uint32_t n_not, uint32_t op) {
  ss_bm25_query q;
  memset(&q, 0xAB, sizeof(q));  // whatever the caller left in the unused slots must not travel
  q.n_terms = np;
  q.op = op | SS_OP_NOT_TERMS(n_not);
  for (uint32_t t = 0; t < np + n_not; t++) {
    q.term[t] = rnd();
    q.idf[t] = 0.25f + (float)(rnd() % 1000u);
  }
  return q;
}

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

// packs qs into a heap block of cap_bytes; compares with the two-pass layout; returns the width (0: the packer gave up)
static uint32_t run(const std::vector<ss_bm25_query>& qs, size_t cap_bytes) {
  uint32_t* buf = (uint32_t*)malloc(cap_bytes ? cap_bytes : 1);
  bm_packer pk;
  pk.dst = buf;
  pk.cap_dwords = cap_bytes / sizeof(uint32_t);
  uint32_t W = 0;
  for (const ss_bm25_query& q : qs) {
    const uint32_t all = q.n_terms + ((q.op >> 8) & 0xFFu);
    W = all > W ? all : W;
    pk.add(q, all);
  }
  uint32_t got = 0;
  if (pk.ok) {
    CHECK(pk.n == qs.size());
    CHECK(pk.W == W);
    CHECK(bm_pack_bytes(qs.size(), W) <= cap_bytes);
    const uint32_t S = bm_pack_stride(W);
    for (size_t i = 0; i < qs.size(); i++) {
      const ss_bm25_query& q = qs[i];
      const uint32_t all = q.n_terms + ((q.op >> 8) & 0xFFu);
      const uint32_t* p = buf + i * S;
      CHECK(p[0] == q.n_terms && p[1] == q.op);
      for (uint32_t t = 0; t < W; t++) {
        uint32_t idf_bits = 0;
        if (t < all) memcpy(&idf_bits, &q.idf[t], 4);
        CHECK(p[BM_PACK_HDR + t] == (t < all ? q.term[t] : 0u));
        CHECK(p[BM_PACK_HDR + W + t] == idf_bits);
      }
    }
    got = W;
  } else {
    CHECK(bm_pack_bytes(qs.size(), W) > cap_bytes);  // gives up for want of room only
  }
  free(buf);
  return got;
}

int main() {
  // every width 1 .. 32 at nq = 1 and nq = 1000, all queries of that width; the staging holds nq full queries (ss_api.hip)
  for (uint32_t W = 1; W <= (uint32_t)SS_MAX_QUERY_TERMS; W++)
    for (uint32_t nq : {1u, 1000u}) {
      std::vector<ss_bm25_query> qs;
      for (uint32_t i = 0; i < nq; i++) qs.push_back(make_query(W, 0, SS_OP_UNION));
      CHECK(run(qs, nq * sizeof(ss_bm25_query)) == W);
    }
  // NOT terms: the width is n_terms + NOT terms, whichever query has the most
  for (uint32_t nq : {1u, 1000u}) {
    std::vector<ss_bm25_query> qs;
    for (uint32_t i = 0; i < nq; i++) qs.push_back(make_query(1 + i % 3, i == nq / 2 ? 4 : i % 2, i % 2 ? SS_OP_UNION : SS_OP_INTERSECTION));
    CHECK(run(qs, nq * sizeof(ss_bm25_query)) == 1u + (nq / 2) % 3 + 4u);
  }
  // widths that grow one by one (31 re-strides), shrink, and alternate
  {
    std::vector<ss_bm25_query> up, down, mix;
    for (uint32_t i = 0; i < 1000; i++) {
      up.push_back(make_query(1 + i * 32 / 1000, 0, SS_OP_UNION));
      down.push_back(make_query(32 - i * 32 / 1000, 0, SS_OP_UNION));
      mix.push_back(make_query(1 + rnd() % 16, rnd() % 17, SS_OP_UNION));
    }
    CHECK(run(up, 1000 * sizeof(ss_bm25_query)) == 32);
    CHECK(run(down, 1000 * sizeof(ss_bm25_query)) == 32);
    CHECK(run(mix, 1000 * sizeof(ss_bm25_query)) != 0);
  }
  // the worst case against the capacity rule: the widest stride is no more than a full query, so nq full queries of room always do,
  // with the widest query arriving LAST (the re-stride moves 999 queries to the end of the block)
  static_assert(bm_pack_stride(SS_MAX_QUERY_TERMS) * 4 <= sizeof(ss_bm25_query), "capacity rule");
  {
    std::vector<ss_bm25_query> qs;
    for (uint32_t i = 0; i < 999; i++) qs.push_back(make_query(3, 0, SS_OP_UNION));
    qs.push_back(make_query(28, 4, SS_OP_UNION));
    CHECK(run(qs, bm_pack_bytes(1000, 32)) == 32);          // exactly the packed batch's bytes
    CHECK(run(qs, 1000 * sizeof(ss_bm25_query)) == 32);     // what the library allocates at least
    CHECK(run(qs, bm_pack_bytes(1000, 32) - 4) == 0);       // one dword short: gives up, writes nothing past the end
    CHECK(run(qs, 0) == 0);
  }
  // give_up(): nothing more is written
  {
    uint32_t* buf = (uint32_t*)malloc(bm_pack_bytes(1, 3));
    bm_packer pk;
    pk.dst = buf;
    pk.cap_dwords = bm_pack_stride(3);
    const ss_bm25_query a = make_query(3, 0, SS_OP_UNION), b = make_query(5, 0, SS_OP_UNION);
    pk.add(a, 3);
    CHECK(pk.ok && pk.n == 1);
    pk.give_up();
    pk.add(b, 5);
    CHECK(!pk.ok && pk.n == 1);
    free(buf);
  }
  // a width outside 1 .. SS_MAX_QUERY_TERMS is refused, not packed
  {
    uint32_t* buf = (uint32_t*)malloc(sizeof(ss_bm25_query));
    bm_packer pk;
    pk.dst = buf;
    pk.cap_dwords = sizeof(ss_bm25_query) / 4;
    const ss_bm25_query a = make_query(3, 0, SS_OP_UNION);
    pk.add(a, 33);
    CHECK(!pk.ok && pk.n == 0);
    free(buf);
  }
  if (failures) return 1;
  printf("pack ok\n");
  return 0;
}
