// Facet records committed level by level, string ranks kept on the device, tombstones added in place (facet_commit.hip; the entry
// points are ss_facet_append_level / _reserve / _info, ss_facet_set_string_ranks / _string_ranks and ss_add_deleted in api_image.hip).
//
// What these need beyond ss_shard's d_facets / facet_docs / facet_record_size lives BESIDE the shard, as the multi-field levels do
// (bm25_image.h ssi_mf_levels): from the first call that needs it until ssi_facet_side_drop (ss_shard_destroy, and ss_facet_upload,
// which replaces the image the state describes).  Read and written under the shard lock.
#pragma once
#include "ss_common.h"
#include "facet_point.h"

struct ss_facet_rank {
  uint32_t offset = 0, type = 0;  // the String16 / String32 facet the table belongs to
  uint32_t n_ids = 0;
  uint32_t* d_rank = nullptr;     // [n_ids] rank of each value id's string (the host's table)
  uint32_t* d_col = nullptr;      // [capacity docs] rank of each doc's string: the u32 key a sort by the facet reads; rows [0, facet_docs) valid
};
struct ss_facet_side {
  uint64_t cap_docs = 0;  // docs d_facets and every d_col have room for; 0: exactly facet_docs (the image of an ss_facet_upload).
                          // Without an image: the room ss_facet_reserve asked for, taken when the first level creates the image
  uint32_t n_ranks = 0;
  ss_facet_rank ranks[SS_MAX_STRING_RANKS];
};
ss_facet_side* ssi_facet_side(const ss_shard* s, bool create);  // null: the shard has none (and create is false)
void ssi_facet_side_drop(const ss_shard* s);                   // frees the tables and columns too
// the rank column of a registered (offset, type), else null.  The sort kernels read it as a U32 facet: (base = column, stride 4, offset 0)
const uint32_t* ssi_facet_rank_column(const ss_shard* s, uint32_t offset, uint32_t type);

// Where the key of each field of a result sort is read: a numeric or Point field in the facet records; a String16 / String32 field in
// its rank column -- to the sort kernels an ordinary U32 facet of 4-byte records.  Resolved ONCE per call by the entry point, under the
// shard lock (the lookup takes the side states' mutex), and handed down to ssi_sort_select / ssi_sort_compose[_browse] (facet.hip).
struct ss_sort_sources {
  const uint8_t* base[SS_MAX_SORT_FIELDS];
  uint32_t stride[SS_MAX_SORT_FIELDS], offset[SS_MAX_SORT_FIELDS], type[SS_MAX_SORT_FIELDS];
};
int ssi_sort_resolve(const ss_shard* s, uint32_t n_sorts, const ss_result_sort* sorts, ss_sort_sources* out);  // SS_ENOTSUP: a string field without a table
int ssi_sort_select(ss_shard* s, uint32_t nq, unsigned long long* d_E, unsigned long long* d_B, unsigned long long* d_ex_b, unsigned long long* d_ex_e,
                    const unsigned long long* d_total, unsigned long long* d_hist, void* d_state, uint32_t n_sorts, const ss_result_sort* sorts,
                    const ss_sort_sources& src, uint32_t k, hipStream_t st, bool byte0_counted = false);
// the facet counters of a batch (ssi_facet_count_multi's arguments and counters) and byte 0 of sort field 0's radix select in ONE launch:
// d_hist [nq][256] then holds what ssi_sort_select's first pass would count -- call it with byte0_counted = true
int ssi_facet_sort_first(ss_shard* s, uint32_t nq, const unsigned long long* d_bits, uint32_t n_facets, const uint32_t* offset, const uint32_t* type,
                         const uint32_t* n_buckets, const ss_facet_point* bases, const uint64_t* d_bounds, unsigned long long* d_counts,
                         const ss_result_sort* sorts, const ss_sort_sources& src, unsigned long long* d_hist, hipStream_t st);
int ssi_sort_compose(ss_shard* s, uint32_t nq, const uint32_t* a_doc, const float* a_score, const uint32_t* a_cnt, const uint32_t* c_doc,
                     const float* c_score, const uint32_t* c_cnt, const unsigned long long* d_total, uint32_t n_sorts, const ss_result_sort* sorts,
                     const ss_sort_sources& src, uint32_t k, uint32_t* out_doc, float* out_score, uint32_t* out_count, unsigned long long* out_total,
                     hipStream_t st);

// col[d] = rank[id(d)] for the n records at `records`; *d_bad (zeroed by the caller) += records whose id is >= n_ids (their col: 0xFFFFFFFF)
int ssi_facet_rank_gather(const uint8_t* records, uint32_t record_size, uint32_t offset, uint32_t type, uint64_t n, const uint32_t* d_rank,
                          uint32_t n_ids, uint32_t* d_col, unsigned long long* d_bad, hipStream_t st);
// out[i] = col[docs[i]] (0xFFFFFFFF for a doc beyond n_docs)
int ssi_facet_rank_read(const uint32_t* d_col, uint64_t n_docs, const uint32_t* d_docs, uint32_t n, uint32_t* d_out, hipStream_t st);
// bits[id >> 5] |= 1 << (id & 31) for n ids (every id inside the bitmap); *d_new (zeroed by the caller) += bits that were clear before
int ssi_deleted_scatter(uint32_t* d_bits, const uint32_t* d_ids, uint64_t n, unsigned long long* d_new, hipStream_t st);
