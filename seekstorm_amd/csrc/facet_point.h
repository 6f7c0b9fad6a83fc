// Point (geo) facets: the facet routines of ss_common.h with the base point the distances are measured from
// (facet.hip; nullptr = the facet's stored bits, as the declarations in ss_common.h behave).
#pragma once
#include "ss_common.h"

// bytes a facet of `type` (<= SS_FACET_POINT, checked by the caller) takes in the record; a Point is its 8-byte Morton code.  (The
// sorts never read a string's id: a string sort field resolves to its u32 rank column, facet_commit.h, or is refused.)  The kernels keep their own device-side tables.
inline uint32_t ssi_facet_width(uint32_t type) {
  static const uint8_t width[] = {1, 2, 4, 8, 1, 2, 4, 8, 4, 8, 2, 4, 8};
  return width[type];
}

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
