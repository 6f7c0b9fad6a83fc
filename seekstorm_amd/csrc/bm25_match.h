// Match sets of queries that name terms of the SPARSE tier (bm25_match.hip): what facet counts, sort pivots and result sorts walk
// when the probe index's bit records alone (ssi_bm25_match_bits, bm25.hip) do not hold the whole query.  Internal.
#pragma once
#include <vector>

#include "ss_common.h"

// How a batch of <= 64 queries splits over the two tiers (ssi_bm25_tier_plan).  Query i is TIERED when one of its terms, scored or
// NOT, is a sparse list.  sub[i] (has_sub[i] != 0) is the part of query i that the bit records answer: an all-dense query whole; a
// tiered union's dense terms with the dense NOT terms; a query whose scored terms are all dense without its sparse NOT terms.
// Intersections and single terms with a sparse scored term have none: their shortest sparse list drives.
struct BmTierPlan {
  std::vector<ss_bm25_query> sub;
  std::vector<uint8_t> has_sub, tiered;
  bool any_tiered = false;
};

// Validates the batch as bm25_search_tiered does (term ids below n_dense + sp_n, positive idf, unique terms) and fills the plan.
// SS_ENOTSUP for what the tiered match set does not answer: phrases, SS_OP_ALL_TERMS_FREQUENT and unions of several terms under a
// field filter that name a sparse term; several indexed fields without merged lists.  All-dense queries are left to check_queries.
int ssi_bm25_tier_plan(const ss_shard* s, uint32_t nq, const ss_bm25_query* q, BmTierPlan* plan);

// The contract of ssi_bm25_match_bits for a planned batch: d_bits [nq][n_sub * BM_SUB / 64] match sets after NOT terms and the
// exclusion bitmap in force, d_total [nq] their exact sizes.  d_q: the batch on the device; d_sub: room for nq queries (the plan's
// dense parts are staged there).  The plan must outlive the stream's work.  SS_ENOTSUP: a dense list of a tiered query has no
// probe row (the caller ran ssi_bm25_ensure_probe_rows first).
int ssi_bm25_match_bits_tiered(ss_shard* s, const BmTierPlan& plan, const ss_bm25_query* h_q, const ss_bm25_query* d_q, ss_bm25_query* d_sub,
                               unsigned long long* d_bits, unsigned long long* d_total, hipStream_t st, uint32_t nq);

// PHRASES (bm25_phrase_bits.hip).  The match set of a phrase = the match set of its INTERSECTION FORM (ssi_bm25_phrase_stage: the same
// terms and NOT terms, no field-filter bits -- a phrase reads the merged lists, its filter is a test on positions), built by the
// calls above, then refined: ssi_bm25_phrase_refine clears every doc of d_bits [nq][n_sub * BM_SUB / 64] whose positions do not carry
// the phrase and takes it off d_total [nq].  d_q: the batch as the caller gave it, on the device; its queries that are no phrases are
// left alone.  ssi_bm25_phrase_check: SS_OK when the refine can answer the phrase on this image; SS_ENOTSUP for what stays with the
// caller's own path -- no positions in the image (or in the sparse tier, for a phrase naming a sparse term), several indexed fields
// without merged lists, a phrase the search refuses as well (a place naming unique term SS_MAX_PHRASE or later; more than 6 unique terms
// with a sparse one among them); SS_EINVAL for a malformed phrase.
int ssi_bm25_phrase_check(const ss_shard* s, const ss_bm25_query& q);
void ssi_bm25_phrase_stage(const ss_bm25_query& q, ss_bm25_query* out);
int ssi_bm25_phrase_refine(ss_shard* s, const ss_bm25_query* d_q, unsigned long long* d_bits, unsigned long long* d_total, hipStream_t st, uint32_t nq);
