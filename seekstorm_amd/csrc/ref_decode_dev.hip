// index.bin opened LEVEL BY LEVEL, its blocks decoded ON THE DEVICE, ready to commit to (ss_bm25_open_index_bin_levels; the seam is the
// end of open_shard, index.rs:3796, followed by commits, commit.rs:142-148).
//
// A block of index.bin is one (key, 65 536-doc level) pair and a raw level of an incremental image (ss_raw_level) is the per-term
// (doc, tf) CSR of one level: the file is already cut the way the incremental image wants it, and a posting decodes independently of
// every other posting of its block (ref_block_decode.h).  So the file's bytes go to HBM one level at a time, a descriptor per block
// says where its postings belong -- a dense term's in its level's d_doc / d_tf, a rare term's in the sparse tier's whole lists --, the
// kernels below write them there, and ONE ssi_bm25_rebuild_from_raw builds the image over all levels.
//
// POSITIONS go the same way (SS_OPEN_POSITIONS_DEVICE): a posting's positions decode independently of every other posting's, and where
// they land is a prefix sum over the postings' counts.  Sweep 1 also stores every posting's count; a 64-bit scan in posting order gives
// d_tpos / d_prel / n_pos of a level -- and, over all levels, the ends of the tier's pool --; a guard refuses a block whose counts add up to
// more than its bytes can hold BEFORE anything is sized by the sum; then rbd_pos_kernel (a lane per posting of at most 64 positions) and
// rbd_pos_long_kernel (a wave per longer posting, its record's bytes 64 at a time) write the positions.
//
// SEVERAL indexed fields go the same way (ss_bm25_open_index_bin_levels_fields, further down): a posting is a merged entry of its level,
// the fields instantiations of the two decode kernels write its doc and the tf of every field, and a scan over per-field flags places
// the per-field lists.
//
// Work goes by POSTING, not by block: on a text-shaped index nearly every block holds 1 - 5 postings.  rbd_flat_kernel: a lane takes
// posting p of a launch and finds its (Array) block by binary search over the blocks' first postings.  Bitmap and Rle blocks are few and
// long: rbd_wg_kernel gives each a workgroup, which scans the words' popcounts / the runs' lengths in LDS and then writes ranks.
#include <atomic>
#include <chrono>
#include <cstring>
#include <memory>

#include "ref_block_decode.h"
#include "ref_index_bin.h"
#include "sparse_levels.h"
#include "bm25_image.h"
#include "api_internal.h"

namespace {

static_assert(RBD_EINVAL == SS_EINVAL && RBD_ENOTSUP == SS_ENOTSUP, "ref_block_decode.h");

// one block of a launch
struct RbdDesc {
  uint64_t body;        // the segment's key bodies: offset in the staged bytes
  uint64_t dst;         // its first posting's index in the destination arrays
  uint32_t body_len;    // byte_array_len
  uint32_t ctp;         // compression_type_pointer
  uint32_t first;       // flat launch: postings of the launch's blocks before this one
  uint16_t count_m1, pivot;
  uint8_t n_comp, comp;
  uint8_t sparse;       // 1: a rare key, its postings go to the tier's whole lists
  uint8_t pad;
};
// where a launch writes: a level's arrays (dense terms) and the tier's (rare terms; a posting's upper word is coded later)
struct RbdDst {
  uint32_t* doc; uint16_t* tf;
  uint64_t* sp_post; uint16_t* sp_tf;
  uint16_t* npos; uint16_t* sp_npos;  // the positions instantiation: every posting's count, beside its tf
  uint32_t doc_base, level_docs;  // first doc of the level, docs it holds
  // the fields instantiation (several indexed fields; a posting = one merged entry of its level): its doc, the tf of every field, and
  // per field a flag "held there" in (term, field, rank) order -- the order of the level's (term, field) lists
  uint32_t* mdoc; uint16_t* mtf; uint16_t* flag;
  uint32_t n_fields, longest;
};
// what a decode kernel takes from a posting beside its doc: the tf; tf + position count; the field vector
enum { RBD_TF = 0, RBD_TF_NPOS = 1, RBD_FIELDS = 2 };
constexpr uint32_t RBD_CHUNK = 2048;  // items (bitmap words, runs) a workgroup scans at a time; the writer's Rle containers hold at most
                                      // that many runs (compress_postinglist.rs:256-332), longer ones take several rounds

__device__ __forceinline__ rbd_block rbd_block_of(const uint8_t* __restrict__ bytes, const RbdDesc& d) {
  rbd_block b;
  b.a = bytes + d.body; b.len = d.body_len; b.ctp = d.ctp; b.count = (uint32_t)d.count_m1 + 1u; b.pivot = d.pivot;
  b.n_comp = d.n_comp; b.comp = d.comp;
  return b;
}
// (the largest code wins: a file that holds a Delta container AND a malformed block answers SS_ENOTSUP, where the host decoder answers
// with whichever it meets first)
__device__ __forceinline__ void rbd_fail(uint32_t* status, int rc) { atomicMax(status, (uint32_t)(-rc)); }
template <bool POS>
__device__ __forceinline__ void rbd_store(const RbdDst& D, const RbdDesc& d, uint32_t r, uint32_t doc, uint32_t tf, uint32_t np) {
  if (d.sparse) {
    D.sp_post[d.dst + r] = (uint64_t)(D.doc_base + doc); D.sp_tf[d.dst + r] = (uint16_t)tf;
    if (POS) D.sp_npos[d.dst + r] = (uint16_t)np;
  } else {
    D.doc[d.dst + r] = D.doc_base + doc; D.tf[d.dst + r] = (uint16_t)tf;
    if (POS) D.npos[d.dst + r] = (uint16_t)np;
  }
}

// the posting of rank r behind its doc, decoded and stored
template <int KIND>
__device__ __forceinline__ int rbd_posting(const RbdDst& D, const RbdDesc& d, const rbd_block& b, const rbd_head& h, uint32_t r, uint32_t doc) {
  if constexpr (KIND == RBD_FIELDS) {
    rbd_fvec v;
    const int rc = rbd_field_vec_packed(b, h, r, D.n_fields, D.longest, &v);
    if (rc != RBD_OK) return rc;
    const uint64_t j = d.dst + r, n = (uint64_t)d.count_m1 + 1u;  // (r < n: the callers' guard)
    D.mdoc[j] = D.doc_base + doc;
    for (uint32_t f = 0; f < D.n_fields; f++) {
      const uint32_t tf = rbd_fvec_tf(v, f);
      D.mtf[j * D.n_fields + f] = (uint16_t)tf;
      D.flag[d.dst * D.n_fields + f * n + r] = tf ? 1u : 0u;
    }
    return RBD_OK;
  } else {
    uint32_t tf = 0u, np = 0u;
    const int rc = KIND == RBD_TF_NPOS ? rbd_npos(b, h, r, &tf, &np) : rbd_tf(b, h, r, &tf);
    if (rc != RBD_OK) return rc;
    rbd_store<KIND == RBD_TF_NPOS>(D, d, r, doc, tf, np);
    return RBD_OK;
  }
}

// Array blocks, one lane per posting
template <int KIND>
__global__ void __launch_bounds__(256) rbd_flat_kernel(const uint8_t* __restrict__ bytes, const RbdDesc* __restrict__ desc, uint32_t n_blocks,
                                                       uint32_t n_post, RbdDst D, uint32_t* __restrict__ status) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= n_post) return;
  uint32_t lo = 0u, hi = n_blocks;  // the block with first <= p < the next block's first
  while (hi - lo > 1u) {
    const uint32_t m = (lo + hi) >> 1;
    if (desc[m].first <= p) lo = m; else hi = m;
  }
  const RbdDesc d = desc[lo];
  const uint32_t r = p - d.first;
  const rbd_block b = rbd_block_of(bytes, d);
  rbd_head h;
  uint32_t doc = 0u;
  int rc = rbd_head_check(b, &h);
  if (rc == RBD_OK && (h.ctype != 1u || r >= b.count)) rc = RBD_EINVAL;  // (the host sends Array blocks here, with their counts)
  if (rc == RBD_OK) rc = rbd_doc(b, h, nullptr, r, D.level_docs, &doc);
  if (rc == RBD_OK) rc = rbd_posting<KIND>(D, d, b, h, r, doc);
  if (rc != RBD_OK) rbd_fail(status, rc);
}

// Bitmap / Rle blocks (and whatever else the head names: refused), one workgroup per block.  The items -- 64-bit bitmap words / runs --
// go through the LDS table RBD_CHUNK at a time (a Bitmap is one chunk; an Rle container of more runs than that, which the writer would
// have made a Bitmap, takes several): their sizes are scanned, then the chunk's ranks are written.  A store is guarded by the key
// head's count; count != popcount / sum of runs is known after the last chunk, and the arrays written are nobody's until the call succeeds.
template <int KIND>
__global__ void __launch_bounds__(256) rbd_wg_kernel(const uint8_t* __restrict__ bytes, const RbdDesc* __restrict__ desc, RbdDst D,
                                                     uint32_t* __restrict__ status) {
  __shared__ uint32_t prefix[RBD_CHUNK + 1];
  __shared__ uint32_t wave_sum[4];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const RbdDesc d = desc[blockIdx.x];
  const rbd_block b = rbd_block_of(bytes, d);
  rbd_head h;
  int rc = rbd_head_check(b, &h);  // (uniform over the workgroup)
  if (rc == RBD_OK && h.ctype == 1u) rc = RBD_EINVAL;  // (Array blocks go to the flat kernel)
  if (rc != RBD_OK) { if (tid == 0) rbd_fail(status, rc); return; }
  const bool bitmap = h.ctype == 2u;
  const uint32_t per = bitmap ? RBD_BITMAP_WORDS / 256u : RBD_CHUNK / 256u, n_items = bitmap ? RBD_BITMAP_WORDS : h.runs;
  uint32_t base = 0u;  // postings of the chunks before (uniform)
  for (uint32_t c0 = 0; c0 < n_items; c0 += per * 256u) {
    const uint32_t m = min(per * 256u, n_items - c0);  // items of this chunk
    uint32_t size[RBD_CHUNK / 256u], mine = 0u;
    for (uint32_t k = 0; k < RBD_CHUNK / 256u; k++) {
      const uint32_t i = tid * per + k;
      size[k] = 0u;
      if (k < per && i < m) {
        if (bitmap) size[k] = rbd_popcount64(rbd_bitmap_word(b, h, i));
        else {
          uint32_t s, l;
          rbd_rle_run(b, h, c0 + i, &s, &l);
          size[k] = l + 1u;
          if (rbd_rle_run_check(b, h, c0 + i)) rbd_fail(status, RBD_EINVAL);  // out of the level, or not behind the run before
        }
      }
      mine += size[k];
    }
    uint32_t incl = mine;
    for (int o = 1; o < 64; o <<= 1) { const uint32_t x = __shfl_up(incl, o); if ((int)lane >= o) incl += x; }
    if (lane == 63u) wave_sum[wave] = incl;
    __syncthreads();
    uint32_t run = incl - mine;
    for (uint32_t w = 0; w < wave; w++) run += wave_sum[w];
    for (uint32_t k = 0; k < per; k++) {
      const uint32_t i = tid * per + k;
      if (i < m) prefix[i] = run;
      run += size[k];
    }
    const uint32_t total = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
    if (tid == 0) prefix[m] = total;
    __syncthreads();
    for (uint32_t q = tid; q < total && base + q < b.count; q += 256u) {  // rank base + q of the block = rank q of the chunk
      uint32_t doc;
      if (bitmap) doc = rbd_doc_bitmap(b, h, prefix, q);
      else {
        const uint32_t i = rbd_prefix_find(prefix, m, q);
        uint32_t s, l;
        rbd_rle_run(b, h, c0 + i, &s, &l);
        doc = s + (q - prefix[i]);
      }
      rc = doc >= D.level_docs ? (int)RBD_EINVAL : rbd_posting<KIND>(D, d, b, h, base + q, doc);
      if (rc != RBD_OK) rbd_fail(status, rc);
    }
    base += total;
    __syncthreads();  // (the next chunk overwrites the table)
  }
  if (base != b.count && tid == 0) rbd_fail(status, RBD_EINVAL);  // count != popcount / sum of runs
}

// ---- the scan over the postings' position counts, 64-bit, in posting order: tiles of RBD_SCAN_TILE counts, three launches (a tile's sum;
// the tiles' sums, one workgroup; the tile again on top of its base).  EXCL: out [n + 1], out[i] = counts before i, out[n] = all;
// else out [n], out[i] = counts up to and including i.  tile [n_tiles + 1]: its last entry receives the sum of all.
constexpr uint32_t RBD_SCAN_PER = 16u, RBD_SCAN_TILE = 256u * RBD_SCAN_PER;

__device__ __forceinline__ uint32_t rbd_wave_incl(uint32_t x, uint32_t lane) {
  for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(x, o); if ((int)lane >= o) x += y; }
  return x;
}
// the counts of a thread (RBD_SCAN_PER in a row) and, returned, what the workgroup's threads before it hold; *total = the tile's sum
__device__ __forceinline__ uint32_t rbd_scan_tile(const uint16_t* __restrict__ cnt, uint64_t n, uint32_t (&v)[RBD_SCAN_PER], uint32_t* wave_sum, uint32_t* total) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint64_t i0 = (uint64_t)blockIdx.x * RBD_SCAN_TILE + (uint64_t)tid * RBD_SCAN_PER;
  uint32_t mine = 0u;
#pragma unroll
  for (uint32_t k = 0; k < RBD_SCAN_PER; k++) { v[k] = i0 + k < n ? (uint32_t)cnt[i0 + k] : 0u; mine += v[k]; }
  const uint32_t incl = rbd_wave_incl(mine, lane);  // (a tile holds less than 2^28 positions)
  if (lane == 63u) wave_sum[wave] = incl;
  __syncthreads();
  uint32_t before = incl - mine;
  for (uint32_t w = 0; w < wave; w++) before += wave_sum[w];
  *total = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
  return before;
}
__global__ void __launch_bounds__(256) rbd_scan_sums_kernel(const uint16_t* __restrict__ cnt, uint64_t n, uint64_t* __restrict__ tile) {
  __shared__ uint32_t wave_sum[4];
  uint32_t v[RBD_SCAN_PER], total;
  (void)rbd_scan_tile(cnt, n, v, wave_sum, &total);
  if (threadIdx.x == 0) tile[blockIdx.x] = total;
}
__global__ void __launch_bounds__(256) rbd_scan_tiles_kernel(uint64_t* __restrict__ tile, uint32_t n_tiles) {  // one workgroup: exclusive, in place
  __shared__ uint64_t wave_sum[4];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  uint64_t base = 0ull;
  for (uint32_t c0 = 0; c0 < n_tiles; c0 += 256u) {
    const uint64_t mine = c0 + tid < n_tiles ? tile[c0 + tid] : 0ull;
    uint64_t incl = mine;
    for (int o = 1; o < 64; o <<= 1) { const uint64_t y = __shfl_up(incl, o); if ((int)lane >= o) incl += y; }
    if (lane == 63u) wave_sum[wave] = incl;
    __syncthreads();
    uint64_t before = base + incl - mine;
    for (uint32_t w = 0; w < wave; w++) before += wave_sum[w];
    if (c0 + tid < n_tiles) tile[c0 + tid] = before;
    base += wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
    __syncthreads();  // (the next round overwrites the waves' sums)
  }
  if (tid == 0) tile[n_tiles] = base;
}
template <bool EXCL>
__global__ void __launch_bounds__(256) rbd_scan_write_kernel(const uint16_t* __restrict__ cnt, uint64_t n, const uint64_t* __restrict__ tile, uint32_t n_tiles,
                                                             uint64_t* __restrict__ out) {
  __shared__ uint32_t wave_sum[4];
  uint32_t v[RBD_SCAN_PER], total;
  uint64_t run = tile[blockIdx.x] + rbd_scan_tile(cnt, n, v, wave_sum, &total);
  const uint64_t i0 = (uint64_t)blockIdx.x * RBD_SCAN_TILE + (uint64_t)threadIdx.x * RBD_SCAN_PER;
#pragma unroll
  for (uint32_t k = 0; k < RBD_SCAN_PER; k++) {
    if (i0 + k < n) out[i0 + k] = EXCL ? run : run + v[k];
    run += v[k];
  }
  if (EXCL && blockIdx.x == 0 && threadIdx.x == 0) out[n] = tile[n_tiles];
}
// a level's d_tpos: the scan at every term's first posting (the last entry: all the level's positions)
__global__ void __launch_bounds__(256) rbd_tpos_kernel(const uint64_t* __restrict__ off, uint32_t n_terms, const uint64_t* __restrict__ scan, uint64_t* __restrict__ tpos) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t <= n_terms) tpos[t] = scan[off[t]];
}

// ---- several indexed fields: the (term, field) lists of a level from its merged entries.  scan [n_ment * F + 1] = the exclusive scan
// of the flags the fields instantiation wrote, in (term, field, rank) order: entries of the level in front of every flag.
// d_foff: the scan at every list's first flag (a lane per list; the last entry: all the level's entries)
__global__ void __launch_bounds__(256) rbd_foff_kernel(const uint64_t* __restrict__ moff, uint32_t n_terms, uint32_t n_fields, const uint64_t* __restrict__ scan,
                                                       uint64_t* __restrict__ foff) {
  const uint64_t v = (uint64_t)blockIdx.x * 256u + threadIdx.x, n = (uint64_t)n_terms * n_fields;
  if (v > n) return;
  if (v == n) { foff[v] = scan[moff[n_terms] * n_fields]; return; }
  const uint64_t t = v / n_fields, f = v - t * n_fields, m0 = moff[t];
  foff[v] = scan[m0 * n_fields + f * (moff[t + 1] - m0)];
}
// d_fdoc / d_ftf: a lane per merged entry finds its term (the last one that begins at or before it) and writes the entry of every
// field it holds where the scan says; nothing is written at or behind n_ent
__global__ void __launch_bounds__(256) rbd_fsplit_kernel(const uint64_t* __restrict__ moff, uint32_t n_terms, uint32_t n_fields, uint64_t n_ment,
                                                         const uint32_t* __restrict__ mdoc, const uint16_t* __restrict__ mtf, const uint64_t* __restrict__ scan,
                                                         uint32_t* __restrict__ fdoc, uint16_t* __restrict__ ftf, uint64_t n_ent) {
  const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (j >= n_ment) return;
  uint32_t lo = 0u, hi = n_terms;
  while (hi - lo > 1u) {
    const uint32_t m = lo + ((hi - lo) >> 1);
    if (moff[m] <= j) lo = m; else hi = m;
  }
  const uint64_t m0 = moff[lo], cnt = moff[lo + 1u] - m0, r = j - m0;
  const uint32_t doc = mdoc[j];
  for (uint32_t f = 0; f < n_fields; f++) {
    const uint16_t tf = mtf[j * n_fields + f];
    if (!tf) continue;
    const uint64_t w = scan[m0 * n_fields + f * cnt + r];
    if (w < n_ent) { fdoc[w] = doc; ftf[w] = tf; }
  }
}

// where the positions of a launch's postings go: posting i (a level's d_npos index / the tier's posting index) has cnt[i] positions from
// scan[i] on (incl: scan holds ENDS, the start is the end before)
struct RbdPos {
  const uint16_t* cnt; const uint64_t* scan; uint32_t incl;
  uint16_t* pos; uint64_t n_pos;   // the destination and its size: nothing is written at or behind n_pos
  uint32_t* prel;                  // a level's d_prel (null: the tier)
  uint32_t* long_list; uint32_t* n_long; uint32_t long_cap;  // the postings of more than 64 positions, by their number in the launch
};
__device__ __forceinline__ uint64_t rbd_pos_start(const RbdPos& P, uint64_t i) { return P.incl ? (i ? P.scan[i - 1u] : 0ull) : P.scan[i]; }
__device__ __forceinline__ uint32_t rbd_desc_find(const RbdDesc* __restrict__ desc, uint32_t n_blocks, uint32_t p) {
  uint32_t lo = 0u, hi = n_blocks;  // the block with first <= p < the next block's first
  while (hi - lo > 1u) {
    const uint32_t m = (lo + hi) >> 1;
    if (desc[m].first <= p) lo = m; else hi = m;
  }
  return lo;
}
// The overlap guard, a lane per block: a position takes at least a byte of its record and an embedded pointer holds at most four, so a
// block whose counts add up to more than body_len + 4 * 65 536 (decode_block's pos_cap) has pointers sharing bytes -- refused before
// anything is sized by the sum
__global__ void __launch_bounds__(256) rbd_guard_kernel(const RbdDesc* __restrict__ desc, uint32_t n_blocks, RbdPos P, uint32_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n_blocks) return;
  const RbdDesc d = desc[i];
  const uint64_t n = (uint64_t)d.count_m1 + 1u;
  const uint64_t sum = (P.incl ? P.scan[d.dst + n - 1u] : P.scan[d.dst + n]) - rbd_pos_start(P, d.dst);
  if (sum > (uint64_t)d.body_len + 4ull * 65536ull) rbd_fail(status, RBD_EINVAL);
}
// Positions, a lane per posting of the launch (every container: only rank, pointer and destination matter here).  Postings of more than
// 64 positions are listed for rbd_pos_long_kernel, so the loop of rbd_positions runs 64 times at most whatever the file says.
__global__ void __launch_bounds__(256) rbd_pos_kernel(const uint8_t* __restrict__ bytes, const RbdDesc* __restrict__ desc, uint32_t n_blocks, uint32_t n_post,
                                                      RbdPos P, uint32_t* __restrict__ status) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= n_post) return;
  const RbdDesc d = desc[rbd_desc_find(desc, n_blocks, p)];
  const uint32_t r = p - d.first;
  const uint64_t i = d.dst + r, start = rbd_pos_start(P, i);
  const uint32_t np = P.cnt[i];
  if (P.prel) P.prel[i] = (uint32_t)(start - rbd_pos_start(P, d.dst));
  if (np == 0u) return;
  if (start + np > P.n_pos) { rbd_fail(status, RBD_EINVAL); return; }
  if (np > 64u) {
    const uint32_t k = atomicAdd(P.n_long, 1u);
    if (k < P.long_cap) P.long_list[k] = p; else rbd_fail(status, RBD_EINVAL);
    return;
  }
  const rbd_block b = rbd_block_of(bytes, d);
  rbd_head h;
  uint32_t n = 0u;
  int rc = rbd_head_check(b, &h);
  if (rc == RBD_OK && r >= b.count) rc = RBD_EINVAL;
  if (rc == RBD_OK) rc = rbd_positions(b, h, r, P.pos + start, np, &n);
  if (rc == RBD_OK && n != np) rc = RBD_EINVAL;
  if (rc != RBD_OK) rbd_fail(status, rc);
}
// ... a wave per posting of more than 64 positions (always a record: a pointer embeds four at most).  The record's position bytes come
// 64 at a time, a lane each; the stop bits are balloted; a lane where a value ends assembles it from its byte and the at most two
// before it (ref_block_decode.h rbd_chunk_size; the last two bytes of the chunk before come along); a wave prefix sum of value + 1 on top
// of the running sum gives the absolute positions, stored in a row.
__global__ void __launch_bounds__(256) rbd_pos_long_kernel(const uint8_t* __restrict__ bytes, const RbdDesc* __restrict__ desc, uint32_t n_blocks, RbdPos P,
                                                           uint32_t* __restrict__ status) {
  const uint32_t lane = threadIdx.x & 63u, n_waves = gridDim.x * 4u;
  const uint32_t n_long = min(*P.n_long, P.long_cap);
  for (uint32_t li = blockIdx.x * 4u + (threadIdx.x >> 6); li < n_long; li += n_waves) {  // (uniform over the wave)
    const uint32_t p = P.long_list[li];
    const RbdDesc d = desc[rbd_desc_find(desc, n_blocks, p)];
    const uint32_t r = p - d.first;
    const uint64_t i = d.dst + r, start = rbd_pos_start(P, i);
    const uint32_t np = P.cnt[i];
    const rbd_block b = rbd_block_of(bytes, d);
    rbd_head h;
    uint32_t ptr = 0u, count = 0u;
    bool wide = false;
    uint64_t at = 0ull;
    int rc = start + np > P.n_pos ? (int)RBD_EINVAL : rbd_head_check(b, &h);
    if (rc == RBD_OK && r >= b.count) rc = RBD_EINVAL;
    if (rc == RBD_OK) rc = rbd_pointer(b, h, r, &ptr, &wide);
    if (rc == RBD_OK && rbd_pointer_embedded(ptr, wide)) rc = RBD_EINVAL;
    if (rc == RBD_OK) rc = rbd_record_area(b, h, ptr, wide, &at, &count);
    if (rc == RBD_OK && count != np) rc = RBD_EINVAL;
    uint32_t done = 0u, sum = 0u, carry = 0u, last1 = 0u, last2 = 0u;  // values stored; sum of value + 1 so far: a position = sum - 1
    while (rc == RBD_OK && done < np) {
      if (at >= b.len) { rc = RBD_EINVAL; break; }
      const uint32_t n_valid = (uint32_t)min((uint64_t)64u, b.len - at);
      const uint32_t byte = lane < n_valid ? (uint32_t)b.a[at + lane] : 0u;
      const uint64_t stops = __ballot(lane < n_valid && (byte & 0x80u));
      const uint32_t size = lane < n_valid ? rbd_chunk_size(stops, lane, carry) : 0u;
      uint32_t b1 = __shfl_up(byte, 1), b0 = __shfl_up(byte, 2);
      if (lane == 0u) { b1 = last1; b0 = last2; }
      if (lane == 1u) b0 = last1;
      const uint64_t ends = __ballot(size != 0u);
      const uint32_t k = done + (uint32_t)__builtin_popcountll(ends & ((1ull << lane) - 1ull));
      const bool take = size != 0u && k < np;
      const uint32_t incl = rbd_wave_incl(take ? rbd_position_value(b0, b1, byte, size) + 1u : 0u, lane);  // (64 values below 2^21)
      const bool over = take && sum + incl - 1u > 65535u;
      if (__ballot(over)) { rc = RBD_ENOTSUP; break; }
      if (take) P.pos[start + k] = (uint16_t)(sum + incl - 1u);
      sum += __shfl(incl, 63);
      done += (uint32_t)__builtin_popcountll(ends);
      if (done < np && n_valid < 64u) { rc = RBD_EINVAL; break; }
      carry = rbd_chunk_carry(stops, 64u, carry);
      last1 = __shfl(byte, 63); last2 = __shfl(byte, 62);
      at += 64u;
    }
    if (rc != RBD_OK && lane == 0u) rbd_fail(status, rc);
  }
}
// the tier's lists' first positions and what the last level brought to every list, from the ends of the pool
__global__ void __launch_bounds__(256) rbd_tier_gather_kernel(const uint64_t* __restrict__ base, const uint32_t* __restrict__ last_n, uint32_t n_lists,
                                                              const uint64_t* __restrict__ pos_end, uint64_t* __restrict__ pbase, uint32_t* __restrict__ last_pos) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i > n_lists) return;
  const uint64_t e0 = base[i];
  pbase[i] = e0 ? pos_end[e0 - 1u] : 0ull;
  if (i == n_lists) return;
  const uint64_t e = base[i + 1u], ln = last_n[i];  // (ln <= e - e0)
  last_pos[i] = ln ? (uint32_t)(pos_end[e - 1u] - (e - ln ? pos_end[e - ln - 1u] : 0ull)) : 0u;
}

struct DevBuf {  // a device block freed when the call returns
  void* p = nullptr;
  size_t cap = 0;
  ~DevBuf() { if (p) (void)hipFree(p); }
  int reserve(size_t bytes) {
    if (bytes <= cap) return SS_OK;
    if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
    SS_HIP(hipMalloc(&p, bytes + bytes / 4 + 256));
    cap = bytes + bytes / 4 + 256;
    return SS_OK;
  }
};

inline uint64_t rd64(const uint8_t* p) { uint64_t v; std::memcpy(&v, p, 8); return v; }

// what the open builds before the swap: released on every way out until the shard has taken it
struct OpenState {
  std::vector<ss_raw_level> levels;
  ss_sparse_tier_built tier;
  std::unique_ptr<ss_shard> img{new ss_shard};
  ss_shard* owner = nullptr;
  hipStream_t st = nullptr;
  bool taken = false;
  ~OpenState() {
    if (!taken) {
      for (ss_raw_level& L : levels) raw_level_free(L);
      ssi_bm25_sparse_tier_drop(&tier);
      bm_image_arrays(img.get(), [&](auto*& p) { if (p && !owner->blocks.release(p)) (void)hipFree(p); });
    }
    if (st) (void)hipStreamDestroy(st);
  }
};

// a block of the file as the walk found it, with what its level's launch needs: read once in term order, written to its level's run,
// so that the per-level pass below reads its blocks in a row (the block table itself is in term order: 40 bytes a block, a cache miss each)
struct LevelEntry { RbdDesc d; const uint8_t* body; uint32_t term; };

// what an open did (ss_bm25_open_info)
struct OpenCounts { uint64_t post_dev = 0, pos_dev = 0, pos_host = 0; };

// the 64-bit scan of n counts on `st` (kernels above): tiles needs room for n / RBD_SCAN_TILE + 2 sums; its last one receives the total
template <bool EXCL>
int rbd_scan_launch(const uint16_t* cnt, uint64_t n, DevBuf& tiles, uint64_t* out, hipStream_t st, const uint64_t** d_total) {
  const uint64_t n_tiles = (n + RBD_SCAN_TILE - 1u) / RBD_SCAN_TILE;
  if (n_tiles > 0x7FFFFFFFull) return SS_ENOTSUP;
  SS_TRY(tiles.reserve((n_tiles + 1u) * sizeof(uint64_t)));
  uint64_t* t = (uint64_t*)tiles.p;
  if (n_tiles) rbd_scan_sums_kernel<<<(uint32_t)n_tiles, 256, 0, st>>>(cnt, n, t);
  rbd_scan_tiles_kernel<<<1, 256, 0, st>>>(t, (uint32_t)n_tiles);
  if (n_tiles) rbd_scan_write_kernel<EXCL><<<(uint32_t)n_tiles, 256, 0, st>>>(cnt, n, t, (uint32_t)n_tiles, out);
  else if (EXCL) SS_HIP(hipMemsetAsync(out, 0, sizeof(uint64_t), st));
  SS_HIP(hipGetLastError());
  *d_total = t + n_tiles;
  return SS_OK;
}
constexpr uint32_t RBD_LONG_GRID = 1024u;  // workgroups of rbd_pos_long_kernel at most: its waves stride over the list

// the device decoder: every level's postings of the dense terms into the level's arrays, the rare terms' into the tier's; pos: with the
// positions of both
int decode_levels_device(const ss_index_bin* ix, uint32_t n_dense, uint32_t n_all, const std::vector<uint32_t>& level_docs, OpenState& O, bool pos,
                         OpenCounts* counts) {
  static const bool trace = getenv("SS_LOAD_TRACE") != nullptr;
  const auto t_0 = std::chrono::steady_clock::now();
  const uint32_t nl = (uint32_t)level_docs.size();
  hipStream_t st = O.st;
  // ---- the blocks, level by level, in term order; a rare term's postings follow each other level after level in its list
  std::vector<uint64_t> lvl_first((size_t)nl + 1, 0);
  for (const ss_index_bin::Blk& e : ix->blocks) {
    if (e.b.block_id >= nl) return SS_EINVAL;
    lvl_first[e.b.block_id + 1]++;
  }
  for (uint32_t l = 0; l < nl; l++) lvl_first[l + 1] += lvl_first[l];
  NoInitVec<LevelEntry> ent(ix->blocks.size());
  ss_sparse_tier_built& T = O.tier;
  const uint32_t n_rare = n_all - n_dense;
  {
    std::vector<uint64_t> at(lvl_first.begin(), lvl_first.end() - 1);
    if (n_rare) { T.h_base.assign((size_t)n_rare + 1, 0); T.h_last_n.assign(n_rare, 0); }
    uint64_t sp_at = 0;
    for (uint32_t t = 0; t < n_all; t++) {
      for (uint64_t bi = ix->term_block_off[t]; bi < ix->term_block_off[t + 1]; bi++) {
        const ss_index_bin::Blk& e = ix->blocks[bi];
        const ss_ref_block& b = e.b;
        const uint32_t n = (uint32_t)b.posting_count_m1 + 1u;
        if (b.byte_array_len > 0xFFFFFFFFull) return SS_EINVAL;
        LevelEntry& E = ent[at[b.block_id]++];
        E.d = RbdDesc{};
        E.d.dst = t < n_dense ? 0ull : sp_at;
        E.d.body_len = (uint32_t)b.byte_array_len;
        E.d.ctp = b.compression_type_pointer;
        E.d.count_m1 = b.posting_count_m1; E.d.pivot = b.pointer_pivot_p_docid;
        E.d.n_comp = e.n_comp; E.d.comp = e.comp;
        E.d.sparse = t < n_dense ? 0 : 1;
        E.body = b.byte_array;
        E.term = t;
        if (t >= n_dense) {
          sp_at += n;
          if (b.block_id == nl - 1u) T.h_last_n[t - n_dense] = n;
        }
      }
      if (t >= n_dense) T.h_base[t - n_dense + 1] = sp_at;
    }
  }
  if (n_rare) {
    const uint64_t tot = T.h_base[n_rare];
    T.n_lists = n_rare; T.last_level = nl - 1u;
    SS_HIP(hipMalloc(&T.d_base, ((size_t)n_rare + 1) * sizeof(uint64_t)));
    SS_HIP(hipMalloc(&T.d_post, std::max<uint64_t>(tot, 1) * sizeof(uint64_t)));
    SS_HIP(hipMalloc(&T.d_tf, std::max<uint64_t>(tot, 1) * sizeof(uint16_t)));
    SS_HIP(hipMemcpyAsync(T.d_base, T.h_base.data(), ((size_t)n_rare + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  }
  // positions: the tier's pool is list after list, each list level after level, so its destinations need the counts of ALL levels -- the
  // rare postings' counts go to a tier-wide array in sweep 1, and every level's staged bytes and rare blocks stay in HBM for sweep 2
  const bool keep = pos && n_rare != 0;
  const uint64_t sp_tot = n_rare ? T.h_base[n_rare] : 0;
  DevBuf d_sp_cnt, d_scan, d_tiles, d_dpos, d_long, d_nlong;
  std::vector<DevBuf> kept_stage(keep ? nl : 0), kept_desc(keep ? nl : 0);
  std::vector<uint32_t> kept_blocks(keep ? nl : 0), kept_post(keep ? nl : 0);
  NoInitVec<RbdDesc> dpos, spos;
  uint64_t n_pos_all = 0;
  if (pos) {
    SS_TRY(d_nlong.reserve(sizeof(uint32_t)));
    if (keep) SS_TRY(d_sp_cnt.reserve(std::max<uint64_t>(sp_tot, 1) * sizeof(uint16_t)));
  }
  DevBuf d_stage, d_flat, d_wg, d_status;
  SS_TRY(d_status.reserve(sizeof(uint32_t)));
  SS_HIP(hipMemsetAsync(d_status.p, 0, sizeof(uint32_t), st));
  std::vector<uint64_t> offs((size_t)n_dense + 1);
  NoInitVec<RbdDesc> flat, wg;
  double ms_host = 0, ms_dev = 0;
  uint64_t n_post_all = 0, n_bytes_all = 0;
  O.levels.resize(nl);
  for (uint32_t l = 0; l < nl; l++) {
    const auto t_a = std::chrono::steady_clock::now();
    // the level's bytes: from its length bytes to the next level's (the last one: to the end of the file)
    const uint8_t* lv_begin = ix->doclen[l];
    const uint8_t* lv_end = l + 1 < nl ? ix->doclen[l + 1] : ix->bytes + ix->len;
    const uint64_t lv_bytes = (uint64_t)(lv_end - lv_begin);
    const LevelEntry* E = ent.data() + lvl_first[l];
    const uint64_t ne = lvl_first[l + 1] - lvl_first[l];
    // the level's CSR over the dense terms
    std::fill(offs.begin(), offs.end(), 0ull);
    for (uint64_t i = 0; i < ne && E[i].term < n_dense; i++) offs[E[i].term + 1] = (uint64_t)E[i].d.count_m1 + 1u;
    for (uint32_t t = 0; t < n_dense; t++) offs[t + 1] += offs[t];
    flat.clear(); wg.clear(); dpos.clear(); spos.clear();
    uint64_t n_flat_post = 0, n_sp_post = 0;
    if (pos && offs[n_dense] > 0xFFFFFFFFull) return SS_ENOTSUP;  // (2^32 postings in one level)
    for (uint64_t i = 0; i < ne; i++) {
      if (E[i].body < lv_begin || E[i].body + E[i].d.body_len > lv_end) return SS_EINVAL;
      RbdDesc d = E[i].d;
      d.body = (uint64_t)(E[i].body - lv_begin);
      if (!d.sparse) d.dst = offs[E[i].term];
      if (pos) {  // the positions kernels number a level's dense postings as its arrays do, its rare ones block after block
        RbdDesc q = d;
        if (d.sparse) {
          if (n_sp_post + 65536u > 0xFFFFFFFFull) return SS_ENOTSUP;
          q.first = (uint32_t)n_sp_post;
          n_sp_post += (uint64_t)d.count_m1 + 1u;
          spos.push_back(q);
        } else {
          q.first = (uint32_t)d.dst;
          dpos.push_back(q);
        }
      }
      if ((d.ctp >> 30) == 1u) {
        if (n_flat_post + 65536u > 0xFFFFFFFFull) return SS_ENOTSUP;  // (2^32 postings in the Array blocks of one level)
        d.first = (uint32_t)n_flat_post;
        n_flat_post += (uint64_t)d.count_m1 + 1u;
        flat.push_back(d);
      } else {
        wg.push_back(d);
      }
    }
    ss_raw_level& L = O.levels[l];
    L.n_docs = level_docs[l]; L.n_terms = n_dense; L.n_post = offs[n_dense];
    const uint64_t np1 = std::max<uint64_t>(L.n_post, 1);
    SS_HIP(hipMalloc(&L.d_off, ((size_t)n_dense + 1) * sizeof(uint64_t)));
    SS_HIP(hipMalloc(&L.d_doc, np1 * sizeof(uint32_t)));
    SS_HIP(hipMalloc(&L.d_tf, np1 * sizeof(uint16_t)));
    DevBuf& stage = keep ? kept_stage[l] : d_stage;
    SS_TRY(stage.reserve(lv_bytes));
    if (pos) {
      SS_HIP(hipMalloc(&L.d_npos, np1 * sizeof(uint16_t)));
      SS_HIP(hipMalloc(&L.d_prel, np1 * sizeof(uint32_t)));
      SS_HIP(hipMalloc(&L.d_tpos, ((size_t)n_dense + 1) * sizeof(uint64_t)));
      SS_TRY(d_scan.reserve((L.n_post + 1) * sizeof(uint64_t)));
      SS_TRY(d_dpos.reserve(std::max<size_t>(dpos.size(), 1) * sizeof(RbdDesc)));
      if (keep) {
        SS_TRY(kept_desc[l].reserve(std::max<size_t>(spos.size(), 1) * sizeof(RbdDesc)));
        kept_blocks[l] = (uint32_t)spos.size(); kept_post[l] = (uint32_t)n_sp_post;
      }
    }
    SS_TRY(d_flat.reserve(std::max<size_t>(flat.size(), 1) * sizeof(RbdDesc)));
    SS_TRY(d_wg.reserve(std::max<size_t>(wg.size(), 1) * sizeof(RbdDesc)));
    const auto t_b = std::chrono::steady_clock::now();
    SS_HIP(hipMemcpyAsync(L.d_off, offs.data(), ((size_t)n_dense + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    SS_HIP(hipMemcpyAsync(stage.p, lv_begin, lv_bytes, hipMemcpyHostToDevice, st));
    if (!flat.empty()) SS_HIP(hipMemcpyAsync(d_flat.p, flat.data(), flat.size() * sizeof(RbdDesc), hipMemcpyHostToDevice, st));
    if (!wg.empty()) SS_HIP(hipMemcpyAsync(d_wg.p, wg.data(), wg.size() * sizeof(RbdDesc), hipMemcpyHostToDevice, st));
    RbdDst D{L.d_doc, L.d_tf, T.d_post, T.d_tf, L.d_npos, (uint16_t*)d_sp_cnt.p, l << 16, level_docs[l], nullptr, nullptr, nullptr, 1u, 0u};
    const uint8_t* d_bytes = (const uint8_t*)stage.p;
    const uint32_t flat_grid = (uint32_t)((n_flat_post + 255u) / 256u);
    if (n_flat_post && pos)
      rbd_flat_kernel<RBD_TF_NPOS><<<flat_grid, 256, 0, st>>>(d_bytes, (const RbdDesc*)d_flat.p, (uint32_t)flat.size(), (uint32_t)n_flat_post, D, (uint32_t*)d_status.p);
    else if (n_flat_post)
      rbd_flat_kernel<RBD_TF><<<flat_grid, 256, 0, st>>>(d_bytes, (const RbdDesc*)d_flat.p, (uint32_t)flat.size(), (uint32_t)n_flat_post, D, (uint32_t*)d_status.p);
    if (!wg.empty() && pos) rbd_wg_kernel<RBD_TF_NPOS><<<(uint32_t)wg.size(), 256, 0, st>>>(d_bytes, (const RbdDesc*)d_wg.p, D, (uint32_t*)d_status.p);
    else if (!wg.empty()) rbd_wg_kernel<RBD_TF><<<(uint32_t)wg.size(), 256, 0, st>>>(d_bytes, (const RbdDesc*)d_wg.p, D, (uint32_t*)d_status.p);
    SS_HIP(hipGetLastError());
    if (pos) {
      // the level's counts scanned in posting order -- the order of d_pos --, its d_tpos, and the guard: all before n_pos sizes anything
      if (!dpos.empty()) SS_HIP(hipMemcpyAsync(d_dpos.p, dpos.data(), dpos.size() * sizeof(RbdDesc), hipMemcpyHostToDevice, st));
      if (keep && !spos.empty()) SS_HIP(hipMemcpyAsync(kept_desc[l].p, spos.data(), spos.size() * sizeof(RbdDesc), hipMemcpyHostToDevice, st));
      const uint64_t* d_total = nullptr;
      SS_TRY(rbd_scan_launch<true>(L.d_npos, L.n_post, d_tiles, (uint64_t*)d_scan.p, st, &d_total));
      rbd_tpos_kernel<<<n_dense / 256u + 1u, 256, 0, st>>>(L.d_off, n_dense, (const uint64_t*)d_scan.p, L.d_tpos);
      RbdPos P{L.d_npos, (const uint64_t*)d_scan.p, 0u, nullptr, 0, L.d_prel, nullptr, (uint32_t*)d_nlong.p, 0u};
      if (!dpos.empty()) rbd_guard_kernel<<<(uint32_t)((dpos.size() + 255u) / 256u), 256, 0, st>>>((const RbdDesc*)d_dpos.p, (uint32_t)dpos.size(), P, (uint32_t*)d_status.p);
      SS_HIP(hipGetLastError());
      uint32_t status_l = 0;
      SS_HIP(hipMemcpyAsync(&status_l, d_status.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
      SS_HIP(hipMemcpyAsync(&L.n_pos, d_total, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
      SS_HIP(hipStreamSynchronize(st));
      if (status_l) return status_l == (uint32_t)(-SS_ENOTSUP) ? SS_ENOTSUP : SS_EINVAL;  // (counts of a refused level size nothing)
      SS_HIP(hipMalloc(&L.d_pos, std::max<uint64_t>(L.n_pos, 1) * sizeof(uint16_t)));
      if (L.n_pos / 65u + 1u > 0xFFFFFFFFull) return SS_ENOTSUP;
      P.pos = L.d_pos; P.n_pos = L.n_pos; P.long_cap = (uint32_t)(L.n_pos / 65u + 1u);  // (a listed posting holds 65 positions at least)
      SS_TRY(d_long.reserve((size_t)P.long_cap * sizeof(uint32_t)));
      P.long_list = (uint32_t*)d_long.p;
      SS_HIP(hipMemsetAsync(d_nlong.p, 0, sizeof(uint32_t), st));
      if (L.n_post) {
        rbd_pos_kernel<<<(uint32_t)((L.n_post + 255u) / 256u), 256, 0, st>>>(d_bytes, (const RbdDesc*)d_dpos.p, (uint32_t)dpos.size(), (uint32_t)L.n_post, P,
                                                                           (uint32_t*)d_status.p);
        rbd_pos_long_kernel<<<std::min<uint32_t>((P.long_cap + 3u) / 4u, RBD_LONG_GRID), 256, 0, st>>>(d_bytes, (const RbdDesc*)d_dpos.p, (uint32_t)dpos.size(), P,
                                                                                                      (uint32_t*)d_status.p);
      }
      SS_HIP(hipGetLastError());
      n_pos_all += L.n_pos;
    }
    SS_HIP(hipStreamSynchronize(st));  // (the host arrays and the staging serve the next level)
    const auto t_c = std::chrono::steady_clock::now();
    ms_host += std::chrono::duration<double, std::milli>(t_b - t_a).count();
    ms_dev += std::chrono::duration<double, std::milli>(t_c - t_b).count();
    for (const RbdDesc& d : wg) n_post_all += (uint64_t)d.count_m1 + 1u;
    n_post_all += n_flat_post;
    n_bytes_all += lv_bytes;
  }
  uint32_t status = 0;
  SS_HIP(hipMemcpy(&status, d_status.p, sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (trace)
    fprintf(stderr, "[load] open levels: block lists %.0f ms; %u levels, %llu postings, %llu file bytes: descriptors %.0f ms, copies + decode kernels %.0f ms\n",
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_0).count() - ms_host - ms_dev, nl,
            (unsigned long long)n_post_all, (unsigned long long)n_bytes_all, ms_host, ms_dev);
  if (status) return status == (uint32_t)(-SS_ENOTSUP) ? SS_ENOTSUP : SS_EINVAL;
  if (keep) {
    // ---- sweep 2: the ends of the tier's pool from the counts of all levels, the guard, the lists' starts and what the last level brought;
    // then the positions of every level's rare blocks from the bytes kept
    const auto t_s = std::chrono::steady_clock::now();
    T.with_pos = true;
    SS_HIP(hipMalloc(&T.d_pos_end, std::max<uint64_t>(sp_tot, 1) * sizeof(uint64_t)));
    const uint64_t* d_total = nullptr;
    SS_TRY(rbd_scan_launch<false>((const uint16_t*)d_sp_cnt.p, sp_tot, d_tiles, T.d_pos_end, st, &d_total));
    RbdPos P{(const uint16_t*)d_sp_cnt.p, T.d_pos_end, 1u, nullptr, 0, nullptr, nullptr, (uint32_t*)d_nlong.p, 0u};
    for (uint32_t l = 0; l < nl; l++)
      if (kept_blocks[l])
        rbd_guard_kernel<<<(kept_blocks[l] + 255u) / 256u, 256, 0, st>>>((const RbdDesc*)kept_desc[l].p, kept_blocks[l], P, (uint32_t*)d_status.p);
    DevBuf d_pbase, d_last_n, d_last_pos;
    SS_TRY(d_pbase.reserve(((size_t)n_rare + 1) * sizeof(uint64_t)));
    SS_TRY(d_last_n.reserve((size_t)n_rare * sizeof(uint32_t)));
    SS_TRY(d_last_pos.reserve((size_t)n_rare * sizeof(uint32_t)));
    SS_HIP(hipMemcpyAsync(d_last_n.p, T.h_last_n.data(), (size_t)n_rare * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    rbd_tier_gather_kernel<<<n_rare / 256u + 1u, 256, 0, st>>>(T.d_base, (const uint32_t*)d_last_n.p, n_rare, T.d_pos_end, (uint64_t*)d_pbase.p,
                                                             (uint32_t*)d_last_pos.p);
    SS_HIP(hipGetLastError());
    T.h_pbase.assign((size_t)n_rare + 1, 0); T.h_last_pos.assign(n_rare, 0);
    SS_HIP(hipMemcpyAsync(&status, d_status.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    SS_HIP(hipMemcpyAsync(&T.pos_n, d_total, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    SS_HIP(hipMemcpyAsync(T.h_pbase.data(), d_pbase.p, ((size_t)n_rare + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    SS_HIP(hipMemcpyAsync(T.h_last_pos.data(), d_last_pos.p, (size_t)n_rare * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    SS_HIP(hipStreamSynchronize(st));
    if (status) return status == (uint32_t)(-SS_ENOTSUP) ? SS_ENOTSUP : SS_EINVAL;
    SS_HIP(hipMalloc(&T.d_pos, std::max<uint64_t>(T.pos_n, 1) * sizeof(uint16_t)));
    if (T.pos_n / 65u + 1u > 0xFFFFFFFFull) return SS_ENOTSUP;
    P.pos = T.d_pos; P.n_pos = T.pos_n; P.long_cap = (uint32_t)(T.pos_n / 65u + 1u);
    SS_TRY(d_long.reserve((size_t)P.long_cap * sizeof(uint32_t)));
    P.long_list = (uint32_t*)d_long.p;
    for (uint32_t l = 0; l < nl; l++) {
      if (!kept_post[l]) continue;
      SS_HIP(hipMemsetAsync(d_nlong.p, 0, sizeof(uint32_t), st));
      rbd_pos_kernel<<<(kept_post[l] + 255u) / 256u, 256, 0, st>>>((const uint8_t*)kept_stage[l].p, (const RbdDesc*)kept_desc[l].p, kept_blocks[l], kept_post[l], P,
                                                                 (uint32_t*)d_status.p);
      rbd_pos_long_kernel<<<std::min<uint32_t>((P.long_cap + 3u) / 4u, RBD_LONG_GRID), 256, 0, st>>>((const uint8_t*)kept_stage[l].p, (const RbdDesc*)kept_desc[l].p,
                                                                                                    kept_blocks[l], P, (uint32_t*)d_status.p);
    }
    SS_HIP(hipGetLastError());
    SS_HIP(hipMemcpyAsync(&status, d_status.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    SS_HIP(hipStreamSynchronize(st));
    if (trace)
      fprintf(stderr, "[load] open levels: tier positions %llu in %.0f ms\n", (unsigned long long)T.pos_n,
              std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_s).count());
    if (status) return status == (uint32_t)(-SS_ENOTSUP) ? SS_ENOTSUP : SS_EINVAL;
    n_pos_all += T.pos_n;
  }
  counts->post_dev = n_post_all; counts->pos_dev = n_pos_all;
  return SS_OK;
}

// with positions: the host decoder's postings and positions, cut per level (dense terms) / taken whole (rare terms)
int decode_levels_host_positions(const ss_index_bin* ix, uint32_t n_dense, uint32_t n_all, const std::vector<uint32_t>& level_docs, OpenState& O) {
  const uint32_t nl = (uint32_t)level_docs.size();
  hipStream_t st = O.st;
  {
    DecodedRange D;
    SS_TRY(ssi_index_bin_decode_range(ix, 0, n_dense, true, &D));
    // a term's first position in D.pos, and per (term, level) where its postings and positions begin: the blocks tell the postings
    std::vector<uint64_t> tpos((size_t)n_dense + 1, 0);
    ss_parallel_for(n_dense, 256, [&](size_t a, size_t b, unsigned) {
      for (size_t t = a; t < b; t++) {
        uint64_t c = 0;
        for (uint64_t j = D.offs[t]; j < D.offs[t + 1]; j++) c += D.npos[j];
        tpos[t + 1] = c;
      }
    });
    for (uint32_t t = 0; t < n_dense; t++) tpos[t + 1] += tpos[t];
    if (tpos[n_dense] != D.pos.size()) return SS_EINVAL;
    const uint64_t nb = ix->term_block_off[n_dense];
    std::vector<uint64_t> blk_post(nb), blk_pos(nb), blk_npos(nb);  // per block of a dense term
    std::atomic<int> bad{0};
    ss_parallel_for(n_dense, 256, [&](size_t a, size_t b, unsigned) {
      for (size_t t = a; t < b; t++) {
        uint64_t j = D.offs[t], p = tpos[t];
        for (uint64_t bi = ix->term_block_off[t]; bi < ix->term_block_off[t + 1]; bi++) {
          const uint64_t n = (uint64_t)ix->blocks[bi].b.posting_count_m1 + 1u;
          if (ix->blocks[bi].b.block_id >= nl || j + n > D.offs[t + 1]) { bad.store(1); return; }
          uint64_t c = 0;
          for (uint64_t x = j; x < j + n; x++) c += D.npos[x];
          blk_post[bi] = j; blk_pos[bi] = p; blk_npos[bi] = c;
          j += n; p += c;
        }
      }
    });
    if (bad.load()) return SS_EINVAL;
    std::vector<uint64_t> cur(ix->term_block_off.begin(), ix->term_block_off.begin() + n_dense);  // every term's next block
    std::vector<uint64_t> offs((size_t)n_dense + 1), poff((size_t)n_dense + 1);
    std::vector<uint32_t> docs;
    std::vector<uint16_t> tfs, npos, pos;
    O.levels.resize(nl);
    for (uint32_t l = 0; l < nl; l++) {
      offs[0] = 0; poff[0] = 0;
      for (uint32_t t = 0; t < n_dense; t++) {
        const bool here = cur[t] < ix->term_block_off[t + 1] && ix->blocks[cur[t]].b.block_id == l;
        offs[t + 1] = offs[t] + (here ? (uint64_t)ix->blocks[cur[t]].b.posting_count_m1 + 1u : 0u);
        poff[t + 1] = poff[t] + (here ? blk_npos[cur[t]] : 0u);
      }
      docs.resize(std::max<uint64_t>(offs[n_dense], 1)); tfs.resize(docs.size()); npos.resize(docs.size());
      pos.resize(std::max<uint64_t>(poff[n_dense], 1));
      ss_parallel_for(n_dense, 256, [&](size_t a, size_t b, unsigned) {
        for (size_t t = a; t < b; t++) {
          const uint64_t n = offs[t + 1] - offs[t];
          if (!n) continue;
          const uint64_t bi = cur[t];
          std::memcpy(&docs[offs[t]], D.docs.data() + blk_post[bi], n * sizeof(uint32_t));
          std::memcpy(&tfs[offs[t]], D.tfs.data() + blk_post[bi], n * sizeof(uint16_t));
          std::memcpy(&npos[offs[t]], D.npos.data() + blk_post[bi], n * sizeof(uint16_t));
          if (blk_npos[bi]) std::memcpy(&pos[poff[t]], D.pos.data() + blk_pos[bi], blk_npos[bi] * sizeof(uint16_t));
        }
      });
      for (uint32_t t = 0; t < n_dense; t++)
        if (offs[t + 1] > offs[t]) cur[t]++;
      LevelPositions P;
      SS_TRY(ssi_level_positions_prepare(n_dense, offs.data(), tfs.data(), npos.data(), pos.data(), poff[n_dense], &P));
      ss_raw_level& L = O.levels[l];
      L.n_docs = level_docs[l]; L.n_terms = n_dense; L.n_post = offs[n_dense]; L.n_pos = poff[n_dense];
      const raw_level_positions rp{P.npos.data(), P.prel.data(), P.tpos.data(), pos.data(), poff[n_dense]};
      SS_TRY(raw_level_upload(L, offs.data(), docs.data(), tfs.data(), n_dense, &rp, st));
    }
  }
  if (n_dense == n_all) return SS_OK;
  // the rare keys: whole lists with their tfs and positions; what the last level brought is what a re-commit of it replaces
  DecodedRange R;
  SS_TRY(ssi_index_bin_decode_range(ix, n_dense, n_all, true, &R));
  const uint32_t n_rare = n_all - n_dense;
  const uint64_t tot = R.offs[n_rare], d_last = (uint64_t)(nl - 1u) << 16;
  ss_sparse_tier_built& T = O.tier;
  T.n_lists = n_rare; T.last_level = nl - 1u; T.with_pos = true;
  T.h_base.assign(R.offs.begin(), R.offs.end());
  T.h_pbase.assign((size_t)n_rare + 1, 0);
  T.h_last_n.assign(n_rare, 0); T.h_last_pos.assign(n_rare, 0);
  NoInitVec<uint64_t> post(std::max<uint64_t>(tot, 1)), pend(std::max<uint64_t>(tot, 1));
  ss_parallel_for(n_rare, 4096, [&](size_t a, size_t b, unsigned) {
    for (size_t i = a; i < b; i++) {
      uint64_t c = 0;
      for (uint64_t j = R.offs[i]; j < R.offs[i + 1]; j++) c += R.npos[j];
      T.h_pbase[i + 1] = c;
    }
  });
  for (uint32_t i = 0; i < n_rare; i++) T.h_pbase[i + 1] += T.h_pbase[i];
  if (T.h_pbase[n_rare] != R.pos.size()) return SS_EINVAL;
  ss_parallel_for(n_rare, 4096, [&](size_t a, size_t b, unsigned) {
    for (size_t i = a; i < b; i++) {
      uint64_t run = T.h_pbase[i];
      for (uint64_t j = R.offs[i]; j < R.offs[i + 1]; j++) {
        run += R.npos[j];
        post[j] = R.docs[j]; pend[j] = run;
        if (R.docs[j] >= d_last) { T.h_last_n[i]++; T.h_last_pos[i] += R.npos[j]; }
      }
    }
  });
  T.pos_n = R.pos.size();
  SS_HIP(hipMalloc(&T.d_base, ((size_t)n_rare + 1) * sizeof(uint64_t)));
  SS_HIP(hipMalloc(&T.d_post, post.size() * sizeof(uint64_t)));
  SS_HIP(hipMalloc(&T.d_tf, post.size() * sizeof(uint16_t)));
  SS_HIP(hipMalloc(&T.d_pos_end, post.size() * sizeof(uint64_t)));
  SS_HIP(hipMalloc(&T.d_pos, std::max<uint64_t>(T.pos_n, 1) * sizeof(uint16_t)));
  SS_HIP(hipMemcpyAsync(T.d_base, T.h_base.data(), ((size_t)n_rare + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  if (tot) {
    SS_HIP(hipMemcpyAsync(T.d_post, post.data(), tot * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    SS_HIP(hipMemcpyAsync(T.d_tf, R.tfs.data(), tot * sizeof(uint16_t), hipMemcpyHostToDevice, st));
    SS_HIP(hipMemcpyAsync(T.d_pos_end, pend.data(), tot * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  }
  if (T.pos_n) SS_HIP(hipMemcpyAsync(T.d_pos, R.pos.data(), T.pos_n * sizeof(uint16_t), hipMemcpyHostToDevice, st));
  SS_HIP(hipStreamSynchronize(st));  // (the host arrays die with this frame)
  return SS_OK;
}

// SS_OPEN_POSITIONS (1) takes the path the measurement of profiles/open_levels_positions_time.json prefers
constexpr int RBD_PREFERRED_POSITIONS_MODE = SS_OPEN_POSITIONS_DEVICE;

int open_levels_impl(ss_shard* s, const ss_index_bin* ix, int mode) {
  const int ran = mode == SS_OPEN_POSITIONS ? RBD_PREFERRED_POSITIONS_MODE : mode;
  const auto t_begin = std::chrono::steady_clock::now();
  static const bool trace = getenv("SS_LOAD_TRACE") != nullptr;
  const uint32_t n_all = (uint32_t)ix->keys.size(), n_dense = std::min<uint32_t>(ix->n_dense, n_all);  // ss_index_bin_tier
  if (n_dense == 0) return SS_EINVAL;  // the dense image needs at least one list
  const uint32_t nl = (uint32_t)ix->doclen.size();
  if (nl == 0 || ix->n_docs > 0xFFFFFFFFull || ix->n_docs <= (uint64_t)(nl - 1u) * 65536u || ix->n_docs > (uint64_t)nl * 65536u) return SS_EINVAL;
  // every level's docs and the sum of their lengths as the file states it: indexed_doc_count / positions_sum_normalized are cumulative
  // (commit.rs:298-311), so the levels' shares add up to what ss_bm25_upload_index_bin divides (index.rs:3480-3482)
  std::vector<uint32_t> level_docs(nl);
  std::vector<uint64_t> level_psum(nl);
  std::vector<uint8_t> doclen(ix->n_docs);
  uint64_t cum = 0;
  for (uint32_t l = 0; l < nl; l++) {
    level_docs[l] = (uint32_t)std::min<uint64_t>(65536u, ix->n_docs - (uint64_t)l * 65536u);
    const uint64_t c = rd64(ix->doclen[l] + 65536u + 8u);
    if (c < cum) return SS_EINVAL;
    level_psum[l] = c - cum;
    cum = c;
    std::memcpy(doclen.data() + (size_t)l * 65536u, ix->doclen[l], level_docs[l]);
  }
  // a term holds at most one block per level, levels ascending (ss_bm25_upload_ref_blocks asks the same): a key head that stands in two
  // segments of one level would send two blocks to one destination -- refused here, before anything is staged or launched
  {
    std::atomic<int> bad{0};
    ss_parallel_for(n_all, 16384, [&](size_t a, size_t b, unsigned) {
      for (size_t t = a; t < b; t++)
        for (uint64_t bi = ix->term_block_off[t]; bi < ix->term_block_off[t + 1]; bi++)
          if (ix->blocks[bi].b.block_id >= nl || (bi > ix->term_block_off[t] && ix->blocks[bi].b.block_id <= ix->blocks[bi - 1].b.block_id)) { bad.store(1); return; }
    });
    if (bad.load()) return SS_EINVAL;
  }
  SS_HIP(hipSetDevice(s->device));
  OpenState O;
  O.owner = s;
  if (const hipError_t e = hipStreamCreateWithFlags(&O.st, hipStreamNonBlocking)) return e == hipErrorOutOfMemory ? SS_ENOMEM : SS_EDEVICE;
  OpenCounts counts;
  if (ran == SS_OPEN_POSITIONS_HOST) {
    SS_TRY(decode_levels_host_positions(ix, n_dense, n_all, level_docs, O));
    for (const ss_raw_level& L : O.levels) counts.pos_host += L.n_pos;
    counts.pos_host += O.tier.pos_n;
  } else {
    SS_TRY(decode_levels_device(ix, n_dense, n_all, level_docs, O, ran == SS_OPEN_POSITIONS_DEVICE, &counts));
  }
  for (uint32_t l = 0; l < nl; l++) O.levels[l].psum = level_psum[l];
  const auto t_build = std::chrono::steady_clock::now();
  // ONE rebuild over all levels, beside the serving image (commits of one shard are the caller's to serialise, as for ss_bm25_append_level)
  SS_TRY(ssi_bm25_rebuild_from_raw(s, O.levels, n_dense, doclen.data(), doclen.size(), O.img.get(), O.st));
  const auto t_tier = std::chrono::steady_clock::now();
  const bool tier = n_dense < n_all;
  if (tier) SS_TRY(ssi_bm25_sparse_tier_code(&O.tier, O.img.get(), O.st));  // a weight the code cannot hold: SS_ENOTSUP, nothing changed
  const auto t_swap = std::chrono::steady_clock::now();
  auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  SS_TRY(ssi_bm25_install_levels(s, O.levels, doclen, O.img.get(), tier ? &O.tier : nullptr, ms(t_build, t_tier), ms(t_begin, std::chrono::steady_clock::now())));
  O.taken = true;
  {
    ShardLock g(s);
    s->open_mode_ran = ran; s->open_post_dev = counts.post_dev; s->open_pos_dev = counts.pos_dev; s->open_pos_host = counts.pos_host;
  }
  if (trace)
    fprintf(stderr, "[load] open levels: decode %.0f ms, rebuild %.0f ms, tier codes %.0f ms, swap %.0f ms\n", ms(t_begin, t_build), ms(t_build, t_tier),
            ms(t_tier, t_swap), ms(t_swap, std::chrono::steady_clock::now()));
  return SS_OK;
}

// ---- SEVERAL indexed fields (ss_bm25_open_index_bin_levels_fields): one ss_raw_level_mf per level of the file, ONE
// ssi_bm25_rebuild_from_raw_fields over all of them.  A posting of a block is one merged entry (term, doc) of its level, so d_moff
// follows from the key heads' counts; the fields instantiation of the decode kernels writes d_mdoc, the rows of d_mtf and a flag per
// (term, field, rank); the 64-bit scan over the flags gives every (term, field) list its place (rbd_foff_kernel) and every entry its own
// (rbd_fsplit_kernel) -- the level mf_level_prepare would make of the same entries, without a host pass over them.
struct OpenStateFields {
  std::vector<ss_raw_level_mf> levels;
  std::unique_ptr<ss_shard> img{new ss_shard};
  ss_shard* owner = nullptr;
  hipStream_t st = nullptr;
  bool taken = false;
  ~OpenStateFields() {
    if (!taken) {
      for (ss_raw_level_mf& L : levels) raw_level_mf_free(L);
      bm_image_arrays(img.get(), [&](auto*& p) { if (p && !owner->blocks.release(p)) (void)hipFree(p); });
    }
    if (st) (void)hipStreamDestroy(st);
  }
};

int decode_levels_fields_device(const ss_index_bin* ix, uint32_t n_terms, const std::vector<uint32_t>& level_docs, OpenStateFields& O, OpenCounts* counts) {
  static const bool trace = getenv("SS_LOAD_TRACE") != nullptr;
  const auto t_0 = std::chrono::steady_clock::now();
  const uint32_t nl = (uint32_t)level_docs.size(), F = ix->n_fields;
  hipStream_t st = O.st;
  // the blocks, level by level, in term order
  std::vector<uint64_t> lvl_first((size_t)nl + 1, 0);
  for (const ss_index_bin::Blk& e : ix->blocks) {
    if (e.b.block_id >= nl) return SS_EINVAL;
    lvl_first[e.b.block_id + 1]++;
  }
  for (uint32_t l = 0; l < nl; l++) lvl_first[l + 1] += lvl_first[l];
  NoInitVec<LevelEntry> ent(ix->blocks.size());
  {
    std::vector<uint64_t> at(lvl_first.begin(), lvl_first.end() - 1);
    for (uint32_t t = 0; t < n_terms; t++)
      for (uint64_t bi = ix->term_block_off[t]; bi < ix->term_block_off[t + 1]; bi++) {
        const ss_index_bin::Blk& e = ix->blocks[bi];
        if (e.b.byte_array_len > 0xFFFFFFFFull) return SS_EINVAL;
        LevelEntry& E = ent[at[e.b.block_id]++];
        E.d = RbdDesc{};
        E.d.body_len = (uint32_t)e.b.byte_array_len;
        E.d.ctp = e.b.compression_type_pointer;
        E.d.count_m1 = e.b.posting_count_m1; E.d.pivot = e.b.pointer_pivot_p_docid;
        E.d.n_comp = e.n_comp; E.d.comp = e.comp;
        E.body = e.b.byte_array;
        E.term = t;
      }
  }
  DevBuf d_stage, d_flat, d_wg, d_status, d_flag, d_scan, d_tiles;
  SS_TRY(d_status.reserve(sizeof(uint32_t)));
  SS_HIP(hipMemsetAsync(d_status.p, 0, sizeof(uint32_t), st));
  std::vector<uint64_t> moff((size_t)n_terms + 1);
  NoInitVec<RbdDesc> flat, wg;
  double ms_host = 0, ms_dev = 0;
  uint64_t n_post_all = 0, n_bytes_all = 0;
  O.levels.resize(nl);
  for (uint32_t l = 0; l < nl; l++) {
    const auto t_a = std::chrono::steady_clock::now();
    const uint8_t* lv_begin = ix->doclen[l];  // the level's bytes begin with its F x 65 536 length bytes
    const uint8_t* lv_end = l + 1 < nl ? ix->doclen[l + 1] : ix->bytes + ix->len;
    const uint64_t lv_bytes = (uint64_t)(lv_end - lv_begin);
    const LevelEntry* E = ent.data() + lvl_first[l];
    const uint64_t ne = lvl_first[l + 1] - lvl_first[l];
    std::fill(moff.begin(), moff.end(), 0ull);
    for (uint64_t i = 0; i < ne; i++) moff[E[i].term + 1] = (uint64_t)E[i].d.count_m1 + 1u;
    for (uint32_t t = 0; t < n_terms; t++) moff[t + 1] += moff[t];
    const uint64_t n_ment = moff[n_terms], n_flag = n_ment * F;
    flat.clear(); wg.clear();
    uint64_t n_flat_post = 0;
    for (uint64_t i = 0; i < ne; i++) {
      if (E[i].body < lv_begin || E[i].body + E[i].d.body_len > lv_end) return SS_EINVAL;
      RbdDesc d = E[i].d;
      d.body = (uint64_t)(E[i].body - lv_begin);
      d.dst = moff[E[i].term];
      if ((d.ctp >> 30) == 1u) {
        if (n_flat_post + 65536u > 0xFFFFFFFFull) return SS_ENOTSUP;  // (2^32 postings in the Array blocks of one level)
        d.first = (uint32_t)n_flat_post;
        n_flat_post += (uint64_t)d.count_m1 + 1u;
        flat.push_back(d);
      } else {
        wg.push_back(d);
      }
    }
    if ((n_ment + 255u) / 256u > 0x7FFFFFFFull) return SS_ENOTSUP;
    ss_raw_level_mf& L = O.levels[l];
    L.n_docs = level_docs[l]; L.n_terms = n_terms; L.n_fields = F; L.n_ment = n_ment;
    L.h_mdf.resize(n_terms);
    for (uint32_t t = 0; t < n_terms; t++) L.h_mdf[t] = (uint32_t)(moff[t + 1] - moff[t]);
    const uint64_t n_lists = (uint64_t)n_terms * F;
    SS_HIP(hipMalloc(&L.d_moff, ((size_t)n_terms + 1) * sizeof(uint64_t)));
    SS_HIP(hipMalloc(&L.d_foff, (n_lists + 1) * sizeof(uint64_t)));
    SS_HIP(hipMalloc(&L.d_mdoc, std::max<uint64_t>(n_ment, 1) * sizeof(uint32_t)));
    SS_HIP(hipMalloc(&L.d_mtf, std::max<uint64_t>(n_flag, 1) * sizeof(uint16_t)));
    SS_HIP(hipMalloc(&L.d_doclen, (size_t)F * L.n_docs));
    SS_TRY(d_stage.reserve(lv_bytes));
    SS_TRY(d_flag.reserve(std::max<uint64_t>(n_flag, 1) * sizeof(uint16_t)));
    SS_TRY(d_scan.reserve((n_flag + 1) * sizeof(uint64_t)));
    SS_TRY(d_flat.reserve(std::max<size_t>(flat.size(), 1) * sizeof(RbdDesc)));
    SS_TRY(d_wg.reserve(std::max<size_t>(wg.size(), 1) * sizeof(RbdDesc)));
    const auto t_b = std::chrono::steady_clock::now();
    SS_HIP(hipMemcpyAsync(L.d_moff, moff.data(), ((size_t)n_terms + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    SS_HIP(hipMemcpyAsync(d_stage.p, lv_begin, lv_bytes, hipMemcpyHostToDevice, st));
    if (!flat.empty()) SS_HIP(hipMemcpyAsync(d_flat.p, flat.data(), flat.size() * sizeof(RbdDesc), hipMemcpyHostToDevice, st));
    if (!wg.empty()) SS_HIP(hipMemcpyAsync(d_wg.p, wg.data(), wg.size() * sizeof(RbdDesc), hipMemcpyHostToDevice, st));
    const uint8_t* d_bytes = (const uint8_t*)d_stage.p;
    for (uint32_t f = 0; f < F; f++)  // [F][level docs] from the staged [F][65 536]
      SS_HIP(hipMemcpyAsync(L.d_doclen + (size_t)f * L.n_docs, d_bytes + (size_t)f * 65536u, L.n_docs, hipMemcpyDeviceToDevice, st));
    RbdDst D{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, l << 16, level_docs[l], L.d_mdoc, L.d_mtf, (uint16_t*)d_flag.p, F, ix->longest_field_id};
    if (n_flat_post)
      rbd_flat_kernel<RBD_FIELDS><<<(uint32_t)((n_flat_post + 255u) / 256u), 256, 0, st>>>(d_bytes, (const RbdDesc*)d_flat.p, (uint32_t)flat.size(),
                                                                                         (uint32_t)n_flat_post, D, (uint32_t*)d_status.p);
    if (!wg.empty()) rbd_wg_kernel<RBD_FIELDS><<<(uint32_t)wg.size(), 256, 0, st>>>(d_bytes, (const RbdDesc*)d_wg.p, D, (uint32_t*)d_status.p);
    SS_HIP(hipGetLastError());
    const uint64_t* d_total = nullptr;
    SS_TRY(rbd_scan_launch<true>((const uint16_t*)d_flag.p, n_flag, d_tiles, (uint64_t*)d_scan.p, st, &d_total));
    rbd_foff_kernel<<<(uint32_t)(n_lists / 256u + 1u), 256, 0, st>>>(L.d_moff, n_terms, F, (const uint64_t*)d_scan.p, L.d_foff);
    SS_HIP(hipGetLastError());
    uint32_t status_l = 0;
    SS_HIP(hipMemcpyAsync(&status_l, d_status.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    SS_HIP(hipMemcpyAsync(&L.n_ent, d_total, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    SS_HIP(hipStreamSynchronize(st));
    if (status_l) return status_l == (uint32_t)(-SS_ENOTSUP) ? SS_ENOTSUP : SS_EINVAL;  // (flags of a refused level size nothing)
    if (L.n_ent > n_flag) return SS_EDEVICE;
    SS_HIP(hipMalloc(&L.d_fdoc, std::max<uint64_t>(L.n_ent, 1) * sizeof(uint32_t)));
    SS_HIP(hipMalloc(&L.d_ftf, std::max<uint64_t>(L.n_ent, 1) * sizeof(uint16_t)));
    if (n_ment)
      rbd_fsplit_kernel<<<(uint32_t)((n_ment + 255u) / 256u), 256, 0, st>>>(L.d_moff, n_terms, F, n_ment, L.d_mdoc, L.d_mtf, (const uint64_t*)d_scan.p, L.d_fdoc,
                                                                          L.d_ftf, L.n_ent);
    SS_HIP(hipGetLastError());
    SS_HIP(hipStreamSynchronize(st));  // (the host arrays and the staging serve the next level)
    const auto t_c = std::chrono::steady_clock::now();
    ms_host += std::chrono::duration<double, std::milli>(t_b - t_a).count();
    ms_dev += std::chrono::duration<double, std::milli>(t_c - t_b).count();
    n_post_all += n_ment;
    n_bytes_all += lv_bytes;
  }
  if (trace)
    fprintf(stderr, "[load] open levels (fields): block lists %.0f ms; %u levels, %llu postings, %llu file bytes: descriptors %.0f ms, copies + decode kernels %.0f ms\n",
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_0).count() - ms_host - ms_dev, nl,
            (unsigned long long)n_post_all, (unsigned long long)n_bytes_all, ms_host, ms_dev);
  counts->post_dev = n_post_all;
  return SS_OK;
}

// with positions: the host decoder's entries and positions (what ss_bm25_upload_index_bin_fields_positions decodes), cut per level; every
// level through mf_level_prepare, as a commit of it
int decode_levels_fields_host(const ss_index_bin* ix, uint32_t n_terms, const std::vector<uint32_t>& level_docs, OpenStateFields& O, OpenCounts* counts) {
  const uint32_t nl = (uint32_t)level_docs.size(), F = ix->n_fields;
  DecodedFields D;
  SS_TRY(ssi_index_bin_decode_fields_range(ix, 0, n_terms, true, &D));
  if (D.offs.size() != (size_t)n_terms + 1 || D.npos.size() != D.docs.size()) return SS_EINVAL;
  // every term's next entry and its first position; entries of a term ascend by doc, so a level's are a run
  std::vector<uint64_t> cur_e(D.offs.begin(), D.offs.end() - 1), cur_p((size_t)n_terms + 1, 0);
  ss_parallel_for(n_terms, 256, [&](size_t a, size_t b, unsigned) {
    for (size_t t = a; t < b; t++) {
      uint64_t c = 0;
      for (uint64_t j = D.offs[t]; j < D.offs[t + 1]; j++) c += D.npos[j];
      cur_p[t + 1] = c;
    }
  });
  for (uint32_t t = 0; t < n_terms; t++) cur_p[t + 1] += cur_p[t];
  if (cur_p[n_terms] != D.pos.size()) return SS_EINVAL;
  std::vector<uint64_t> offs((size_t)n_terms + 1), poff((size_t)n_terms + 1);
  std::vector<uint32_t> docs;
  std::vector<uint8_t> fields, dl;
  std::vector<uint16_t> tfs, npos, pos;
  O.levels.resize(nl);
  for (uint32_t l = 0; l < nl; l++) {
    offs[0] = 0; poff[0] = 0;
    ss_parallel_for(n_terms, 256, [&](size_t a, size_t b, unsigned) {
      for (size_t t = a; t < b; t++) {
        uint64_t j = cur_e[t], c = 0;
        for (; j < D.offs[t + 1] && (D.docs[j] >> 16) == l; j++) c += D.npos[j];
        offs[t + 1] = j - cur_e[t]; poff[t + 1] = c;
      }
    });
    for (uint32_t t = 0; t < n_terms; t++) { offs[t + 1] += offs[t]; poff[t + 1] += poff[t]; }
    const uint64_t n_ent = offs[n_terms], n_pos = poff[n_terms];
    docs.resize(std::max<uint64_t>(n_ent, 1)); fields.resize(docs.size()); tfs.resize(docs.size()); npos.resize(docs.size());
    pos.resize(std::max<uint64_t>(n_pos, 1));
    ss_parallel_for(n_terms, 256, [&](size_t a, size_t b, unsigned) {
      for (size_t t = a; t < b; t++) {
        const uint64_t n = offs[t + 1] - offs[t], np = poff[t + 1] - poff[t];
        if (n) {
          std::memcpy(&docs[offs[t]], D.docs.data() + cur_e[t], n * sizeof(uint32_t));
          std::memcpy(&fields[offs[t]], D.fields.data() + cur_e[t], n);
          std::memcpy(&tfs[offs[t]], D.tfs.data() + cur_e[t], n * sizeof(uint16_t));
          std::memcpy(&npos[offs[t]], D.npos.data() + cur_e[t], n * sizeof(uint16_t));
        }
        if (np) std::memcpy(&pos[poff[t]], D.pos.data() + cur_p[t], np * sizeof(uint16_t));
        cur_e[t] += n; cur_p[t] += np;
      }
    });
    dl.resize((size_t)F * level_docs[l]);
    for (uint32_t f = 0; f < F; f++) std::memcpy(dl.data() + (size_t)f * level_docs[l], ix->doclen[l] + (size_t)f * 65536u, level_docs[l]);
    mf_level_host H;
    SS_TRY(mf_level_prepare(l, level_docs[l], F, n_terms, offs.data(), docs.data(), fields.data(), tfs.data(), npos.data(), pos.data(), n_pos, &H));
    SS_TRY(raw_level_mf_upload(O.levels[l], H, dl.data(), O.st));
    counts->pos_host += n_pos;
  }
  for (uint32_t t = 0; t < n_terms; t++)
    if (cur_e[t] != D.offs[t + 1]) return SS_EINVAL;  // an entry behind the last level
  return SS_OK;
}

int open_levels_fields_impl(ss_shard* s, const ss_index_bin* ix, const float* boost, int mode) {
  const int ran = mode == SS_OPEN_POSITIONS ? (int)SS_OPEN_POSITIONS_HOST : mode;
  const auto t_begin = std::chrono::steady_clock::now();
  static const bool trace = getenv("SS_LOAD_TRACE") != nullptr;
  const uint32_t n_terms = (uint32_t)ix->keys.size(), F = ix->n_fields;
  const uint32_t nl = (uint32_t)ix->doclen.size();
  if (nl == 0 || ix->n_docs > 0xFFFFFFFFull || ix->n_docs <= (uint64_t)(nl - 1u) * 65536u || ix->n_docs > (uint64_t)nl * 65536u) return SS_EINVAL;
  if (ix->longest_field_id >= F) return SS_EINVAL;
  // every level's docs and the sum of their lengths as the file states it (cumulative behind the level's F x 65 536 length bytes)
  std::vector<uint32_t> level_docs(nl);
  std::vector<uint64_t> level_psum(nl);
  uint64_t cum = 0;
  for (uint32_t l = 0; l < nl; l++) {
    level_docs[l] = (uint32_t)std::min<uint64_t>(65536u, ix->n_docs - (uint64_t)l * 65536u);
    const uint64_t c = rd64(ix->doclen[l] + (size_t)F * 65536u + 8u);
    if (c < cum) return SS_EINVAL;
    level_psum[l] = c - cum;
    cum = c;
  }
  // a term holds at most one block per level, levels ascending: a key head in two segments of one level would send two blocks to one
  // destination -- refused here, before anything is staged or launched
  {
    std::atomic<int> bad{0};
    ss_parallel_for(n_terms, 16384, [&](size_t a, size_t b, unsigned) {
      for (size_t t = a; t < b; t++)
        for (uint64_t bi = ix->term_block_off[t]; bi < ix->term_block_off[t + 1]; bi++)
          if (ix->blocks[bi].b.block_id >= nl || (bi > ix->term_block_off[t] && ix->blocks[bi].b.block_id <= ix->blocks[bi - 1].b.block_id)) { bad.store(1); return; }
    });
    if (bad.load()) return SS_EINVAL;
  }
  std::vector<float> b(F, 1.0f);
  if (boost) b.assign(boost, boost + F);
  ss_mf_levels* const M = ssi_mf_levels(s, true);
  std::lock_guard<std::mutex> commits(M->commit_mu);  // an open is a commit of every level: one after the other with the shard's commits
  SS_HIP(hipSetDevice(s->device));
  OpenStateFields O;
  O.owner = s;
  if (const hipError_t e = hipStreamCreateWithFlags(&O.st, hipStreamNonBlocking)) return e == hipErrorOutOfMemory ? SS_ENOMEM : SS_EDEVICE;
  OpenCounts counts;
  if (ran == SS_OPEN_POSITIONS_HOST) SS_TRY(decode_levels_fields_host(ix, n_terms, level_docs, O, &counts));
  else SS_TRY(decode_levels_fields_device(ix, n_terms, level_docs, O, &counts));
  for (uint32_t l = 0; l < nl; l++) O.levels[l].psum = level_psum[l];
  const auto t_build = std::chrono::steady_clock::now();
  SS_TRY(ssi_bm25_rebuild_from_raw_fields(s, O.levels, F, b.data(), O.img.get(), O.st));
  auto ms = [](std::chrono::steady_clock::time_point x, std::chrono::steady_clock::time_point y) { return std::chrono::duration<double, std::milli>(y - x).count(); };
  const auto t_swap = std::chrono::steady_clock::now();
  SS_TRY(ssi_bm25_install_levels_fields(s, O.levels, b, O.img.get(), ms(t_build, t_swap), ms(t_begin, t_swap)));
  O.taken = true;
  {
    ShardLock g(s);
    s->open_mode_ran = ran; s->open_post_dev = counts.post_dev; s->open_pos_dev = 0; s->open_pos_host = counts.pos_host;
  }
  if (trace)
    fprintf(stderr, "[load] open levels (fields): decode %.0f ms, rebuild %.0f ms, swap %.0f ms\n", ms(t_begin, t_build), ms(t_build, t_swap),
            ms(t_swap, std::chrono::steady_clock::now()));
  return SS_OK;
}

}  // namespace

extern "C" int ss_bm25_open_index_bin_levels_fields(ss_shard* s, const ss_index_bin* ix, const float* boost, int with_positions) {
  if (!s || !ix) return SS_EINVAL;
  if (ix->keys.empty() || ix->n_docs == 0) return SS_EINVAL;
  if (ix->n_fields < 2) return SS_EINVAL;  // one indexed field: ss_bm25_open_index_bin_levels
  if (ix->n_fields > 8) return SS_ENOTSUP;
  if (with_positions < SS_OPEN_NO_POSITIONS || with_positions > SS_OPEN_POSITIONS_DEVICE) return SS_EINVAL;
  if (with_positions == SS_OPEN_POSITIONS_DEVICE) return SS_ENOTSUP;  // field-tagged positions decoded on the device: not built
  if (ix->n_dense < ix->keys.size()) return SS_ENOTSUP;                // a tiered ix: a multi-field tier that takes levels is not built from whole lists
  return ss_guard([&] { return open_levels_fields_impl(s, ix, boost, with_positions); }, SS_ENOMEM, SS_EDEVICE);
}

extern "C" int ss_bm25_open_index_bin_levels(ss_shard* s, const ss_index_bin* ix, int with_positions) {
  if (!s || !ix) return SS_EINVAL;
  if (ix->keys.empty() || ix->n_docs == 0) return SS_EINVAL;
  if (ix->n_fields > 1) return SS_ENOTSUP;  // several indexed fields: ss_bm25_open_index_bin_levels_fields
  if (with_positions < SS_OPEN_NO_POSITIONS || with_positions > SS_OPEN_POSITIONS_DEVICE) return SS_EINVAL;
  return ss_guard([&] { return open_levels_impl(s, ix, with_positions); }, SS_ENOMEM, SS_EDEVICE);
}

extern "C" int ss_bm25_open_info(ss_shard* s, int* mode_ran, uint64_t* n_postings_dev, uint64_t* n_positions_dev, uint64_t* n_positions_host) {
  if (!s) return SS_EINVAL;
  ShardLock g(s);
  if (s->open_mode_ran < 0) return SS_ESTATE;
  if (mode_ran) *mode_ran = s->open_mode_ran;
  if (n_postings_dev) *n_postings_dev = s->open_post_dev;
  if (n_positions_dev) *n_positions_dev = s->open_pos_dev;
  if (n_positions_host) *n_positions_host = s->open_pos_host;
  return SS_OK;
}

namespace {
// n elements from the device, synchronously (the caller holds the shard lock; whatever wrote them has been waited for)
template <class T>
int read_dev(T* out, const T* d, uint64_t n) {
  if (n) SS_HIP(hipMemcpy(out, d, n * sizeof(T), hipMemcpyDeviceToHost));
  return SS_OK;
}
}  // namespace

extern "C" int ss_bm25_level_read(ss_shard* s, uint32_t level, uint32_t t0, uint32_t t1, uint64_t* offs_out, uint32_t* docs_out, uint16_t* tfs_out,
                                  uint16_t* npos_out, uint16_t* pos_out, uint64_t post_cap, uint64_t pos_cap, uint64_t* n_post, uint64_t* n_pos) {
  if (!s || !n_post || !n_pos) return SS_EINVAL;
  return ss_guard([&]() -> int {
    ShardLock g(s);
    if (level >= s->raw.size()) return SS_EINVAL;
    const ss_raw_level& L = s->raw[level];
    if (t0 > t1 || t1 > L.n_terms) return SS_EINVAL;
    SS_HIP(hipSetDevice(s->device));
    SS_HIP(hipDeviceSynchronize());
    std::vector<uint64_t> off((size_t)(t1 - t0) + 1);
    SS_TRY(read_dev(off.data(), L.d_off + t0, off.size()));
    const uint64_t j0 = off.front(), j1 = off.back();
    uint64_t p0 = 0, p1 = 0;
    if (L.d_tpos) { SS_TRY(read_dev(&p0, L.d_tpos + t0, 1)); SS_TRY(read_dev(&p1, L.d_tpos + t1, 1)); }
    if (j1 < j0 || j1 > L.n_post || p1 < p0 || p1 > L.n_pos) return SS_EDEVICE;
    *n_post = j1 - j0; *n_pos = p1 - p0;
    if (((docs_out || tfs_out || npos_out) && post_cap < *n_post) || (pos_out && pos_cap < *n_pos)) return SS_EINVAL;
    if (offs_out) for (size_t i = 0; i < off.size(); i++) offs_out[i] = off[i] - j0;
    if (docs_out) SS_TRY(read_dev(docs_out, L.d_doc + j0, *n_post));
    if (tfs_out) SS_TRY(read_dev(tfs_out, L.d_tf + j0, *n_post));
    if (npos_out && L.d_npos) SS_TRY(read_dev(npos_out, L.d_npos + j0, *n_post));
    if (pos_out && L.d_pos) SS_TRY(read_dev(pos_out, L.d_pos + p0, *n_pos));
    return SS_OK;
  }, SS_ENOMEM, SS_EDEVICE);
}

extern "C" int ss_bm25_level_read_fields(ss_shard* s, uint32_t level, uint32_t t0, uint32_t t1, uint64_t* foff_out, uint32_t* fdoc_out, uint16_t* ftf_out,
                                         uint64_t* moff_out, uint32_t* mdoc_out, uint16_t* mtf_out, uint32_t* mnpos_out, uint64_t* tpos_out, uint32_t* pos_out,
                                         uint8_t* doclen_out, uint64_t ent_cap, uint64_t ment_cap, uint64_t pos_cap, uint64_t doclen_cap, uint64_t* n_ent,
                                         uint64_t* n_ment, uint64_t* n_pos, uint32_t* n_fields, uint32_t* n_docs) {
  if (!s || !n_ent || !n_ment || !n_pos || !n_fields || !n_docs) return SS_EINVAL;
  return ss_guard([&]() -> int {
    const ss_mf_levels* M = ssi_mf_levels(s, false);
    ShardLock g(s);
    if (!M || M->raw.empty()) return SS_ESTATE;  // no levels of several indexed fields kept in HBM
    if (level >= M->raw.size()) return SS_EINVAL;
    const ss_raw_level_mf& L = M->raw[level];
    if (t0 > t1 || t1 > L.n_terms) return SS_EINVAL;
    SS_HIP(hipSetDevice(s->device));
    SS_HIP(hipDeviceSynchronize());
    const uint64_t F = L.n_fields;
    std::vector<uint64_t> fo((size_t)(t1 - t0) * F + 1), mo((size_t)(t1 - t0) + 1);
    SS_TRY(read_dev(fo.data(), L.d_foff + (size_t)t0 * F, fo.size()));
    SS_TRY(read_dev(mo.data(), L.d_moff + t0, mo.size()));
    const uint64_t e0 = fo.front(), e1 = fo.back(), m0 = mo.front(), m1 = mo.back();
    uint64_t p0 = 0, p1 = 0;
    if (L.d_tpos) { SS_TRY(read_dev(&p0, L.d_tpos + t0, 1)); SS_TRY(read_dev(&p1, L.d_tpos + t1, 1)); }
    if (e1 < e0 || e1 > L.n_ent || m1 < m0 || m1 > L.n_ment || p1 < p0 || p1 > L.n_pos) return SS_EDEVICE;
    *n_ent = e1 - e0; *n_ment = m1 - m0; *n_pos = p1 - p0; *n_fields = L.n_fields; *n_docs = L.n_docs;
    if (((fdoc_out || ftf_out) && ent_cap < *n_ent) || ((mdoc_out || mtf_out || mnpos_out) && ment_cap < *n_ment) || (pos_out && pos_cap < *n_pos) ||
        (doclen_out && doclen_cap < F * L.n_docs))
      return SS_EINVAL;
    if (foff_out) for (size_t i = 0; i < fo.size(); i++) foff_out[i] = fo[i] - e0;
    if (moff_out) for (size_t i = 0; i < mo.size(); i++) moff_out[i] = mo[i] - m0;
    if (fdoc_out) SS_TRY(read_dev(fdoc_out, L.d_fdoc + e0, *n_ent));
    if (ftf_out) SS_TRY(read_dev(ftf_out, L.d_ftf + e0, *n_ent));
    if (mdoc_out) SS_TRY(read_dev(mdoc_out, L.d_mdoc + m0, *n_ment));
    if (mtf_out) SS_TRY(read_dev(mtf_out, L.d_mtf + m0 * F, *n_ment * F));
    if (doclen_out) SS_TRY(read_dev(doclen_out, L.d_doclen, F * L.n_docs));
    if (L.d_tpos) {
      if (mnpos_out) SS_TRY(read_dev(mnpos_out, L.d_mnpos + m0, *n_ment));
      if (tpos_out) {
        std::vector<uint64_t> tp((size_t)(t1 - t0) + 1);
        SS_TRY(read_dev(tp.data(), L.d_tpos + t0, tp.size()));
        for (size_t i = 0; i < tp.size(); i++) tpos_out[i] = tp[i] - p0;
      }
      if (pos_out) SS_TRY(read_dev(pos_out, L.d_pos + p0, *n_pos));
    }
    return SS_OK;
  }, SS_ENOMEM, SS_EDEVICE);
}

extern "C" int ss_bm25_sparse_read(ss_shard* s, uint32_t l0, uint32_t l1, uint64_t* offs_out, uint32_t* docs_out, uint16_t* tfs_out, uint16_t* npos_out,
                                   uint16_t* pos_out, uint64_t post_cap, uint64_t pos_cap, uint64_t* n_post, uint64_t* n_pos) {
  if (!s || !n_post || !n_pos) return SS_EINVAL;
  return ss_guard([&]() -> int {
    ShardLock g(s);
    const uint16_t* d_tf = ssi_bm25_sparse_levels_tf(s);
    if (!d_tf || !s->d_sp_base || !s->d_sp_post) return SS_ESTATE;  // no tier of one indexed field that keeps its tfs
    if (l0 > l1 || l1 > s->sp_n) return SS_EINVAL;
    SS_HIP(hipSetDevice(s->device));
    SS_HIP(hipDeviceSynchronize());
    std::vector<uint64_t> off((size_t)(l1 - l0) + 1);
    SS_TRY(read_dev(off.data(), s->d_sp_base + l0, off.size()));
    const uint64_t j0 = off.front(), j1 = off.back();
    if (j1 < j0) return SS_EDEVICE;
    const bool with_pos = s->d_sp_pos_end && s->d_sp_pos && s->sp_pos_elem == sizeof(uint16_t);
    std::vector<uint64_t> end;  // the end before the first posting, then every posting's
    if (with_pos && j1 > j0) {
      end.assign((size_t)(j1 - j0) + 1, 0);
      SS_TRY(read_dev(end.data() + (j0 ? 0 : 1), s->d_sp_pos_end + (j0 ? j0 - 1 : 0), (j1 - j0) + (j0 ? 1 : 0)));
      for (size_t i = 1; i < end.size(); i++)
        if (end[i] < end[i - 1] || end[i] - end[i - 1] > 65535u || end[i] > s->sp_pos_n) return SS_EDEVICE;
    }
    *n_post = j1 - j0; *n_pos = end.empty() ? 0 : end.back() - end.front();
    if (((docs_out || tfs_out || npos_out) && post_cap < *n_post) || (pos_out && pos_cap < *n_pos)) return SS_EINVAL;
    if (offs_out) for (size_t i = 0; i < off.size(); i++) offs_out[i] = off[i] - j0;
    if (docs_out) {
      std::vector<uint64_t> post(*n_post);
      SS_TRY(read_dev(post.data(), s->d_sp_post + j0, *n_post));
      for (uint64_t j = 0; j < *n_post; j++) docs_out[j] = (uint32_t)post[j];  // (the upper word: the weight code)
    }
    if (tfs_out) SS_TRY(read_dev(tfs_out, d_tf + j0, *n_post));
    if (npos_out && !end.empty()) for (uint64_t j = 0; j < *n_post; j++) npos_out[j] = (uint16_t)(end[j + 1] - end[j]);
    if (pos_out && !end.empty()) SS_TRY(read_dev(pos_out, (const uint16_t*)s->d_sp_pos + end.front(), *n_pos));
    return SS_OK;
  }, SS_ENOMEM, SS_EDEVICE);
}
