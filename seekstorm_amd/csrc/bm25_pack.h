// The PACKED form of a host-pointer BM25 batch: what a batch without phrase queries travels to the device in.  Host-only C++, no HIP
// (tests/test_pack_cpu.py compiles it by itself); bm25.hip reads the layout constants.
//
// A public query (ss_bm25_query) is 280 bytes -- 32 term slots, 32 idf slots, the phrase fields -- of which a three-term union uses 32.
// Packed, query i stands at dword i * bm_pack_stride(W):
//   [0] n_terms   [1] op   [2 .. 2 + W) term ids   [2 + W .. 2 + 2 W) idfs (bit patterns)
// with W = the largest n_terms + NOT terms of the batch, so the stride is uniform; slots past a query's own terms are zero.
// bm_packer fills a buffer query by query, in the pass that validates the batch (ss_api.hip check_queries): W is only known at the end
// of that pass, so the packer starts narrow and re-strides what it holds when a wider query arrives (at most 31 times, in practice
// once or twice near the start of the batch).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/seekstorm_hip.h"

constexpr uint32_t BM_PACK_HDR = 2u;  // dwords in front of the term ids
constexpr uint32_t bm_pack_stride(uint32_t W) { return BM_PACK_HDR + 2u * W; }  // dwords per query
constexpr size_t bm_pack_bytes(size_t nq, uint32_t W) { return nq * bm_pack_stride(W) * sizeof(uint32_t); }
// the widest packed query is no larger than the full form: a staging buffer sized for nq full queries holds any packed batch of nq
static_assert(bm_pack_bytes(1, SS_MAX_QUERY_TERMS) <= sizeof(ss_bm25_query), "packed form larger than the full form");

struct bm_packer {
  uint32_t* dst = nullptr;  // room for cap_dwords dwords
  size_t cap_dwords = 0;
  uint32_t W = 0;           // slots per query so far
  uint32_t n = 0;           // queries held
  bool ok = true;           // false: given up (no room, or the caller said so) -- the batch travels in the full form

  void give_up() { ok = false; }
  // query n of the batch; all = n_terms + NOT terms, 1 .. SS_MAX_QUERY_TERMS (the caller has validated it)
  void add(const ss_bm25_query& Q, uint32_t all) {
    if (!ok) return;
    if (all == 0 || all > (uint32_t)SS_MAX_QUERY_TERMS) { ok = false; return; }
    const uint32_t Wn = all > W ? all : W;
    if (((size_t)n + 1) * bm_pack_stride(Wn) > cap_dwords) { ok = false; return; }
    if (Wn != W) widen(Wn);
    uint32_t* p = dst + (size_t)n * bm_pack_stride(W);
    p[0] = Q.n_terms;
    p[1] = Q.op;
    memcpy(p + BM_PACK_HDR, Q.term, all * sizeof(uint32_t));
    memcpy(p + BM_PACK_HDR + W, Q.idf, all * sizeof(uint32_t));
    for (uint32_t t = all; t < W; t++) p[BM_PACK_HDR + t] = p[BM_PACK_HDR + W + t] = 0u;
    n++;
  }

 private:
  // the n queries held move from stride(W) to stride(Wn), last first: query i's new place starts at or behind its old one and
  // ends in front of nothing that has not moved yet
  void widen(uint32_t Wn) {
    const uint32_t So = bm_pack_stride(W), Sn = bm_pack_stride(Wn);
    uint32_t tmp[bm_pack_stride(SS_MAX_QUERY_TERMS)];
    for (uint32_t i = n; i-- > 0;) {
      memcpy(tmp, dst + (size_t)i * So, So * sizeof(uint32_t));
      uint32_t* p = dst + (size_t)i * Sn;
      p[0] = tmp[0];
      p[1] = tmp[1];
      for (uint32_t t = 0; t < Wn; t++) {
        p[BM_PACK_HDR + t] = t < W ? tmp[BM_PACK_HDR + t] : 0u;
        p[BM_PACK_HDR + Wn + t] = t < W ? tmp[BM_PACK_HDR + W + t] : 0u;
      }
    }
    W = Wn;
  }
};
