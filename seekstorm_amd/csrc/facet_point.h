// Point (geo) facets: the facet routines of ss_common.h with the base point the distances are measured from
// (facet.hip; nullptr = the facet's stored bits, as the declarations in ss_common.h behave).
#pragma once
#include "ss_common.h"
#include "filter_rows.h"  // ssi_facet_width and the host's checks of a filter

// exclusion ROWS for a batch whose queries each carry their own filter set (filter_rows.h groups the sets; facet.hip).  d_rows
// [rows.n_rows][row_words] u32: bit set = doc excluded (a failed filter of the row's set, a tombstone, a doc at or beyond the lexical
// image's); row_words = 2 * n_sub * (BM_SUB / 64), the layout ExclSwap::per_query() consumers read.  d_sets: room for
// ssi_filter_rows_bytes(rows) bytes, the sets as the kernel reads them -- staged from h_stage, which lives until the stream has passed.
size_t ssi_filter_rows_bytes(const ss_filter_rows& rows);
int ssi_facet_build_rows(ss_shard* s, const ss_filter_rows& rows, void* d_sets, std::vector<uint8_t>* h_stage, uint32_t* d_rows, uint32_t row_words,
                         hipStream_t st);
// E[i] &= ~X[row_of[i]] over nq match sets of `groups` u64 words, d_total[i] = the docs left (d_row_of: row per query, on the device);
// d_Xq (may be null) [nq][groups]: every query's row copied out, the one-bitmap-per-query layout of ExclSwap::per_query()
int ssi_match_exclude_rows(ss_shard* s, uint32_t nq, unsigned long long* d_E, const unsigned long long* d_X, const uint32_t* d_row_of, uint64_t groups,
                           unsigned long long* d_total, unsigned long long* d_Xq, hipStream_t st);

int ssi_facet_kth(ss_shard* s, const unsigned long long* d_bits, uint64_t n_docs, uint64_t n_matches, uint32_t offset, uint32_t type,
                  bool descending, uint64_t k, unsigned long long* d_hist, uint64_t* value_bits, uint64_t* n_better, uint64_t* n_equal,
                  const ss_facet_point* point, hipStream_t st);
int ssi_facet_values(ss_shard* s, const uint32_t* d_docs, uint32_t n, uint32_t offset, uint32_t type, unsigned long long* d_out,
                     const ss_facet_point* point, hipStream_t st);
int ssi_facet_count(ss_shard* s, const unsigned long long* d_bits, uint64_t n_docs, uint32_t offset, uint32_t type, uint32_t n_buckets,
                    const uint64_t* d_bounds, unsigned long long* d_counts, const ss_facet_point* point, hipStream_t st);
// every facet of every query of a batch in one launch (facet.hip: "Facet counts of a BATCH")
int ssi_facet_count_multi(ss_shard* s, uint32_t nq, const unsigned long long* d_bits, uint32_t n_facets, const uint32_t* offset, const uint32_t* type,
                          const uint32_t* n_buckets, const ss_facet_point* bases, const uint64_t* d_bounds, unsigned long long* d_counts,
                          hipStream_t st);
