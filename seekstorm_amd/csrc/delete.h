// delete_documents_by_query on the device (ss_bm25_delete_by_query; api_delete.hip): the kernels between "match sets of a batch" and
// "tombstones, counted and listed" (delete.hip).  Internal.
// All work of a call goes into a PENDING bitmap of the image's match-set width: `groups` u64 groups in ssi_bm25_match_bits' layout,
// the same bytes viewed as 2 * groups u32 words the tombstone bitmap's layout.  Both views 16-byte aligned, `groups` even.
#pragma once
#include "ss_common.h"

// pending[g] |= OR over the rows r of `row_mask` (bit r = row r, r < 64) of d_bits[r * groups + g]: the whole match sets of a chunk
int ssi_delete_collect(unsigned long long* d_pending, const unsigned long long* d_bits, uint64_t groups, uint64_t row_mask, hipStream_t st);
// over the u32 words w < pend_words: fresh = pending[w] & ~deleted[w] (a word at or beyond del_words reads as 0), pending[w] = fresh,
// *d_count (zeroed by the caller) += popc(fresh); with `commit` also deleted[w] |= fresh for w < del_words.  The only writer of the
// live bitmap; no word outside either bitmap is read or written
int ssi_delete_commit(uint32_t* d_pending, uint64_t pend_words, uint32_t* d_deleted, uint64_t del_words, bool commit, unsigned long long* d_count,
                      hipStream_t st);
