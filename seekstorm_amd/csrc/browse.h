// The empty query of a shard (ss_docs_search; browse.hip): "every live doc" as a match bitmap in ssi_bm25_match_bits' layout, and the
// selection of a bitmap's docs by doc id.  Internal.
#pragma once
#include "ss_common.h"
#include "facet_commit.h"

constexpr uint32_t BROWSE_SLICE = 256;  // 64-bit words of a bitmap per slice (= per workgroup): 16384 docs
inline uint64_t browse_slices(uint64_t groups) { return (groups + BROWSE_SLICE - 1) / BROWSE_SLICE; }

// d_bits [groups = bm_n_sub * BM_SUB / 64]: bit d = doc d is below bm_n_docs and not excluded by the bitmap in force (s->d_deleted:
// tombstones, or what with_facet_filter installed); d_slice_cnt [browse_slices(groups)]: the popcount of every slice; *d_total (zeroed
// by the caller) += the popcount of the whole set
int ssi_browse_bits(ss_shard* s, unsigned long long* d_bits, uint32_t* d_slice_cnt, unsigned long long* d_total, hipStream_t st);
// The docs of a bitmap by doc id: rank 0 = the largest id (descending) or the smallest; the set bits of rank [skip, skip + take) go to
// d_out_doc in rank order, *d_out_n = their number = min(take, matches - skip), and nothing is written beyond them.  No bit of d_bits
// stands at or beyond bm_n_docs.  d_slice_cnt / d_slice_begin [browse_slices(groups)]: scratch.
int ssi_browse_select(ss_shard* s, const unsigned long long* d_bits, bool descending, uint64_t skip, uint64_t take, uint32_t* d_slice_cnt,
                      unsigned long long* d_slice_begin, bool slices_counted, uint32_t* d_out_doc, uint32_t* d_out_n, hipStream_t st);
// d_bits &= ~{d_docs[0 .. n)}, *d_count -= n: a pass of a deep sorted page leaves the match set
int ssi_browse_clear(ss_shard* s, unsigned long long* d_bits, const uint32_t* d_docs, uint32_t n, unsigned long long* d_count, hipStream_t st);
// facet.hip: the compose step of a sorted browse (sort_compose_kernel's browse instances)
int ssi_sort_compose_browse(ss_shard* s, const uint32_t* a_doc, const uint32_t* a_cnt, const uint32_t* c_doc, const uint32_t* c_cnt,
                            const unsigned long long* d_total, uint32_t n_sorts, const ss_result_sort* sorts, const ss_sort_sources& src, uint32_t k,
                            bool doc_ascending, uint32_t* out_doc, uint32_t* out_count, unsigned long long* out_total, hipStream_t st);
