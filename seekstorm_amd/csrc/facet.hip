// Facet filter of the lexical search (search.rs FacetFilter -> FilterSparse, add_result.rs:341-482 is_facet_filter) for gfx950.
//
// The reference keeps one fixed-size record per doc in facet.bin (facets_size_sum bytes, each facet at its offset) and,
// per candidate doc, drops the doc unless EVERY filtered facet passes: a numeric value inside the half-open Rust range
// [start, end), a string id (String16 / String32) inside the set of wanted ids.  A filtered doc neither counts nor ranks
// (add_result.rs:3499-3501 returns before the count) -- exactly what a tombstone does.  So the filter is evaluated ONCE per
// call over all docs into an exclusion bitmap (OR-ed with the tombstones: ~n_docs x record bytes read, 20-50 us at 10 M
// docs) and the search kernels run with that bitmap in place of the tombstone bitmap; nothing in them changes.
#include <algorithm>
#include <cstring>
#include <vector>

#include "facet_point.h"
#include "facet_commit.h"
#include "bit_select.h"

struct FacetFilters {
  uint32_t n;
  ss_facet_filter f[SS_MAX_FACET_FILTERS];
};

__device__ __forceinline__ unsigned long long facet_read(const uint8_t* p, uint32_t bytes) {
  unsigned long long v = 0;
  for (uint32_t b = 0; b < bytes; b++) v |= (unsigned long long)p[b] << (8u * b);  // little endian, any alignment
  return v;
}

// ---- Point facets (FieldType::Point, index.rs:1050-1056): the stored value is the 64-bit Morton code of (lat, lon) x 1e7
// as i32 (geo_search.rs:27-41: lat in the even bits, lon in the odd ones).  What filters, counts and sorts is a DISTANCE
// to a base point, in f64 like the reference, operation by operation in its order (no fused multiply-add):
//   unit km / miles: euclidian_distance(base, doc) = R * sqrt(x^2 + y^2), x = DEG2RAD*(dlon)*cos(DEG2RAD*(lat1+lat2)/2),
//                    y = DEG2RAD*(dlat)                                   (geo_search.rs:115-124; facet filter, facet count)
//   sort key:        simplified_distance(doc, base) = x^2 + y^2 without DEG2RAD and R (geo_search.rs:82-87, morton_ordering)
// cos / sqrt are the device library's f64 routines: a last-place difference from the host's libm can move a doc that sits
// within an ulp of a range bound, nothing else.
struct FacetPoint {
  double lat, lon, radius;  // radius 0: the sort key
};
__host__ __device__ inline uint32_t morton_compact(unsigned long long x) {  // the even bits of x, packed
  x &= 0x5555555555555555ull;
  x = (x ^ (x >> 1)) & 0x3333333333333333ull;
  x = (x ^ (x >> 2)) & 0x0F0F0F0F0F0F0F0Full;
  x = (x ^ (x >> 4)) & 0x00FF00FF00FF00FFull;
  x = (x ^ (x >> 8)) & 0x0000FFFF0000FFFFull;
  x = (x ^ (x >> 16)) & 0x00000000FFFFFFFFull;
  return (uint32_t)x;
}
// (the host's half -- morton_encode, the constants -- stands in filter_rows.h: ssi_filter_prepare computes a filter's Morton corners)

__device__ double facet_point_distance(const FacetPoint& b, unsigned long long code) {
#pragma clang fp contract(off)
  const double lat = (double)(int32_t)morton_compact(code) / 10000000.0;
  const double lon = (double)(int32_t)morton_compact(code >> 1) / 10000000.0;
  const double c = cos(kDeg2Rad * (b.lat + lat) / 2.0);
  if (b.radius != 0.0) {
    const double x = kDeg2Rad * (lon - b.lon) * c, y = kDeg2Rad * (lat - b.lat);
    return b.radius * sqrt(x * x + y * y);
  }
  const double x = (b.lon - lon) * c, y = b.lat - lat;
  return x * x + y * y;
}
// a facet's value as the bits the comparisons below work on: Point -> the f64 distance (from then on an F64 facet)
__device__ __forceinline__ unsigned long long facet_load(const uint8_t* p, uint32_t bytes, uint32_t& type, const FacetPoint& pt) {
  const unsigned long long v = facet_read(p, bytes);
  if (type != SS_FACET_POINT) return v;
  type = SS_FACET_F64;
  return (unsigned long long)__double_as_longlong(facet_point_distance(pt, v));
}
__host__ inline int facet_point_of(const ss_facet_point* p, FacetPoint* out) {
  if (!p || p->unit > SS_POINT_MILES) return SS_EINVAL;
  *out = FacetPoint{p->lat, p->lon, p->unit == SS_POINT_KM ? kEarthKm : p->unit == SS_POINT_MILES ? kEarthMi : 0.0};
  return SS_OK;
}

// lo <= v < hi as Rust's Range::contains; the two flag bits turn the ends around (the pivots of a result sort need
// "strictly above" and "equal to" for every type, and a 64-bit type has no value above its largest to write as an end)
template <typename T>
__device__ __forceinline__ bool facet_in(T v, T lo, T hi, uint32_t flags) {
  const bool above = (flags & SS_FACET_LO_EXCLUSIVE) ? v > lo : v >= lo;
  const bool below = (flags & SS_FACET_HI_INCLUSIVE) ? v <= hi : v < hi;
  return above && below;
}
__device__ bool facet_pass(const uint8_t* rec, const ss_facet_filter& f) {
  const uint8_t* p = rec + f.offset;
  const uint32_t fl = f.reserved;
  switch (f.type) {
    case SS_FACET_U8: return facet_in<unsigned long long>(facet_read(p, 1), f.lo, f.hi, fl);
    case SS_FACET_U16: return facet_in<unsigned long long>(facet_read(p, 2), f.lo, f.hi, fl);
    case SS_FACET_U32: return facet_in<unsigned long long>(facet_read(p, 4), f.lo, f.hi, fl);
    case SS_FACET_U64: return facet_in<unsigned long long>(facet_read(p, 8), f.lo, f.hi, fl);
    case SS_FACET_I8: return facet_in<long long>((int8_t)facet_read(p, 1), (long long)f.lo, (long long)f.hi, fl);
    case SS_FACET_I16: return facet_in<long long>((int16_t)facet_read(p, 2), (long long)f.lo, (long long)f.hi, fl);
    case SS_FACET_I32: return facet_in<long long>((int32_t)facet_read(p, 4), (long long)f.lo, (long long)f.hi, fl);
    case SS_FACET_I64: return facet_in<long long>((long long)facet_read(p, 8), (long long)f.lo, (long long)f.hi, fl);
    case SS_FACET_F32:
      return facet_in<float>(__uint_as_float((uint32_t)facet_read(p, 4)), __uint_as_float((uint32_t)f.lo), __uint_as_float((uint32_t)f.hi), fl);
    case SS_FACET_F64:
      return facet_in<double>(__longlong_as_double((long long)facet_read(p, 8)), __longlong_as_double((long long)f.lo),
                              __longlong_as_double((long long)f.hi), fl);
    case SS_FACET_STRING16:
    case SS_FACET_STRING32: {
      const uint32_t v = (uint32_t)facet_read(p, f.type == SS_FACET_STRING16 ? 2 : 4);
      if (f.n_values == SS_FACET_IDS_EXTERN)  // a set of any size: one bit per id (ssi_facet_build put it behind the exclusion bitmap)
        return v < f.hi && ((((const uint32_t*)(uintptr_t)f.lo)[v >> 5] >> (v & 31u)) & 1u) != 0u;
      for (uint32_t i = 0; i < f.n_values; i++)
        if (f.values[i] == v) return true;
      return false;
    }
    case SS_FACET_POINT: {  // FilterSparse::Point, add_result.rs:462-478: inside the Morton range AND inside the distance range
      const unsigned long long code = facet_read(p, 8);
      unsigned long long w[4];
      for (int i = 0; i < 4; i++) w[i] = (unsigned long long)f.values[2 * i] | ((unsigned long long)f.values[2 * i + 1] << 32);
      const FacetPoint b{__longlong_as_double((long long)w[0]), __longlong_as_double((long long)w[1]),
                         f.n_values == SS_POINT_KM ? kEarthKm : f.n_values == SS_POINT_MILES ? kEarthMi : 0.0};
      if (f.n_values != SS_POINT_SORTKEY && !(code >= w[2] && code < w[3])) return false;
      return facet_in<double>(facet_point_distance(b, code), __longlong_as_double((long long)f.lo), __longlong_as_double((long long)f.hi), fl);
    }
    default: return true;
  }
}

// one thread per doc, one bitmap word per 32 docs: bit set = the doc is excluded (a failed facet or a tombstone)
__global__ void facet_filter_kernel(const uint8_t* __restrict__ records, uint32_t record_size, unsigned long long n_docs,
                                    FacetFilters F, const uint32_t* __restrict__ del, uint32_t del_words,
                                    uint32_t* __restrict__ out) {
  const unsigned long long d = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  bool excluded = false;
  if (d < n_docs) {
    const uint8_t* rec = records + d * record_size;
    for (uint32_t i = 0; i < F.n && !excluded; i++) excluded = !facet_pass(rec, F.f[i]);
  }
  const unsigned long long b = __ballot(excluded);
  const uint32_t lane = threadIdx.x & 63u;
  if ((lane & 31u) == 0) {
    const unsigned long long w = d >> 5;
    if (w < (n_docs + 31) / 32) {
      uint32_t bits = (uint32_t)(b >> (lane & 32u));
      if (w < del_words) bits |= del[w];
      out[w] = bits;
    }
  }
}

int ssi_facet_build(ss_shard* s, uint32_t n_filters, const ss_facet_filter* filters, hipStream_t st) {
  if (!s->d_facets) return SS_ESTATE;
  if (n_filters == 0 || n_filters > SS_MAX_FACET_FILTERS || !filters) return SS_EINVAL;
  FacetFilters F;
  F.n = n_filters;
  uint64_t set_words = 0, set_begin[SS_MAX_FACET_FILTERS] = {0}, set_bits[SS_MAX_FACET_FILTERS] = {0};
  for (uint32_t i = 0; i < n_filters; i++) {
    const ss_facet_filter& f = filters[i];
    const int rcf = ssi_filter_prepare(f, s->facet_record_size, &F.f[i]);  // (filter_rows.h: the checks, a Point filter's Morton corners)
    if (rcf != SS_OK) return rcf;
    if (ssi_filter_is_extern(f)) {  // lo = host array of hi ids -> a bitmap over [0, largest id]
      const uint32_t* ids = (const uint32_t*)(uintptr_t)f.lo;
      uint64_t bits = 0;
      for (uint64_t j = 0; j < f.hi; j++) bits = std::max<uint64_t>(bits, (uint64_t)ids[j] + 1);
      if (f.type == SS_FACET_STRING16) bits = std::min<uint64_t>(bits, 65536);  // ids beyond the facet's width match nothing
      if (bits > (1ull << 30)) return SS_EINVAL;
      set_begin[i] = set_words;
      set_bits[i] = bits;
      set_words += (bits + 31) / 32;
    }
  }
  const uint64_t words = (s->facet_docs + 31) / 32;
  if (words + set_words > s->filter_words_cap) {
    if (s->d_filter_bits) (void)hipFree(s->d_filter_bits);
    s->d_filter_bits = nullptr;
    s->filter_words_cap = 0;
    SS_HIP(hipMalloc(&s->d_filter_bits, (words + set_words) * sizeof(uint32_t)));
    s->filter_words_cap = words + set_words;
  }
  if (set_words) {  // the id sets as bitmaps behind the exclusion bitmap
    // staging that outlives the call (the copy is asynchronous on st; calls that share a shard are stream-ordered)
    static thread_local std::vector<uint32_t> stage;
    stage.assign(set_words, 0u);
    for (uint32_t i = 0; i < n_filters; i++) {
      const ss_facet_filter& f = filters[i];
      if (!((f.type == SS_FACET_STRING16 || f.type == SS_FACET_STRING32) && f.n_values == SS_FACET_IDS_EXTERN)) continue;
      const uint32_t* ids = (const uint32_t*)(uintptr_t)f.lo;
      for (uint64_t j = 0; j < f.hi; j++)
        if (ids[j] < set_bits[i]) stage[set_begin[i] + (ids[j] >> 5)] |= 1u << (ids[j] & 31u);
      F.f[i].lo = (uint64_t)(uintptr_t)(s->d_filter_bits + words + set_begin[i]);
      F.f[i].hi = set_bits[i];
    }
    SS_HIP(hipMemcpyAsync(s->d_filter_bits + words, stage.data(), set_words * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  }
  facet_filter_kernel<<<(unsigned)((s->facet_docs + 255) / 256), 256, 0, st>>>(
      s->d_facets, s->facet_record_size, (unsigned long long)s->facet_docs, F, s->n_deleted ? s->d_deleted : nullptr,
      (uint32_t)s->deleted_words, s->d_filter_bits);
  SS_HIP(hipGetLastError());
  return SS_OK;
}

// ---- Exclusion ROWS: a batch whose queries each carry their own filter set (ss_bm25_search_each; filter_rows.h groups byte-equal sets
// into rows).  ONE pass over the records writes all n_rows <= 64 rows: a block of 256 threads stages the sets -- [row_begin: n_rows + 1
// u32, padded to 16 bytes][the filters, 64 bytes each]; 64 sets of 8 filters are 32 KB, beyond any kernarg -- and its 256 records in LDS
// (one coalesced read of 256 * record_size bytes, whatever n_rows is; records of more than 64 bytes are read in place instead), then
// every thread tests its doc against row after row with facet_pass as it stands, one ballot per row, and the lanes 0 and 32 of a wave
// write the row's word | the tombstones' word.  The grid covers the whole row -- row_words * 32 docs, the lexical image's sub-blocks --
// and a doc at or beyond n_docs is excluded, so every word of every row is written: no clearing, no atomics.
constexpr uint32_t FR_THREADS = 256, FR_RECORD_LDS = 16384;
static inline uint32_t filter_rows_head(uint32_t n_rows) { return ((n_rows + 1u) * 4u + 15u) & ~15u; }
__global__ __launch_bounds__(FR_THREADS) void facet_filter_rows_kernel(const uint8_t* __restrict__ records, uint32_t record_size, unsigned long long n_docs,
                                                                       const uint32_t* __restrict__ sets, uint32_t n_rows, uint32_t n_filters, uint32_t stage_records,
                                                                       const uint32_t* __restrict__ del, uint32_t del_words, uint32_t* __restrict__ out,
                                                                       uint32_t row_words) {
  extern __shared__ __align__(16) uint8_t fr_lds[];
  const uint32_t tid = threadIdx.x, head = ((n_rows + 1u) * 4u + 15u) & ~15u, set_words = (head + n_filters * (uint32_t)sizeof(ss_facet_filter)) / 4u;
  const uint32_t* s_begin = (const uint32_t*)fr_lds;
  const ss_facet_filter* s_f = (const ss_facet_filter*)(fr_lds + head);
  uint8_t* s_rec = fr_lds + (size_t)set_words * 4u;
  for (uint32_t i = tid; i < set_words; i += FR_THREADS) ((uint32_t*)fr_lds)[i] = sets[i];
  const unsigned long long d0 = (unsigned long long)blockIdx.x * FR_THREADS, d = d0 + tid;
  const uint8_t* rec = records + d * record_size;  // (dereferenced for d < n_docs only)
  if (stage_records && d0 < n_docs) {
    const uint32_t bytes = (uint32_t)min((unsigned long long)FR_THREADS, n_docs - d0) * record_size, words = bytes / 4u;
    const uint8_t* src = records + d0 * record_size;  // (d0 is a multiple of 256: word-aligned whatever the record size)
    for (uint32_t i = tid; i < words; i += FR_THREADS) ((uint32_t*)s_rec)[i] = ((const uint32_t*)src)[i];
    for (uint32_t i = words * 4u + tid; i < bytes; i += FR_THREADS) s_rec[i] = src[i];
    rec = s_rec + tid * record_size;
  }
  __syncthreads();
  const bool live = d < n_docs;
  const uint32_t lane = tid & 63u;
  const unsigned long long w = d >> 5;
  const bool writer = (lane & 31u) == 0u && w < row_words;
  const uint32_t tomb = (writer && del && w < del_words) ? del[w] : 0u;
  for (uint32_t r = 0; r < n_rows; r++) {
    bool excluded = !live;
    if (live)
      for (uint32_t j = s_begin[r]; j < s_begin[r + 1] && !excluded; j++) excluded = !facet_pass(rec, s_f[j]);
    const unsigned long long b = __ballot(excluded);
    if (writer) out[(size_t)r * row_words + w] = (uint32_t)(b >> (lane & 32u)) | tomb;
  }
}

size_t ssi_filter_rows_bytes(const ss_filter_rows& rows) { return filter_rows_head(rows.n_rows) + rows.prepared.size() * sizeof(ss_facet_filter); }

int ssi_facet_build_rows(ss_shard* s, const ss_filter_rows& rows, void* d_sets, std::vector<uint8_t>* h_stage, uint32_t* d_rows, uint32_t row_words,
                         hipStream_t st) {
  if (!s->d_facets || s->facet_docs < s->bm_n_docs) return SS_ESTATE;
  if (rows.n_rows == 0) return SS_OK;
  if (rows.n_rows > 64 || rows.row_begin.size() != rows.n_rows + 1u || (uint64_t)row_words * 32u < s->bm_n_docs) return SS_EINVAL;
  const uint32_t head = filter_rows_head(rows.n_rows), n_filters = (uint32_t)rows.prepared.size();
  h_stage->assign(ssi_filter_rows_bytes(rows), 0);
  memcpy(h_stage->data(), rows.row_begin.data(), rows.row_begin.size() * 4);
  if (n_filters) memcpy(h_stage->data() + head, rows.prepared.data(), (size_t)n_filters * sizeof(ss_facet_filter));
  SS_HIP(hipMemcpyAsync(d_sets, h_stage->data(), h_stage->size(), hipMemcpyHostToDevice, st));
  const uint32_t stage_records = (uint64_t)FR_THREADS * s->facet_record_size <= FR_RECORD_LDS ? 1u : 0u;
  const size_t lds = h_stage->size() + (stage_records ? (size_t)FR_THREADS * s->facet_record_size : 0);
  const unsigned grid = (unsigned)(((uint64_t)row_words * 32u + FR_THREADS - 1) / FR_THREADS);
  facet_filter_rows_kernel<<<grid, FR_THREADS, lds, st>>>(s->d_facets, s->facet_record_size, (unsigned long long)s->bm_n_docs, (const uint32_t*)d_sets,
                                                          rows.n_rows, n_filters, stage_records, s->n_deleted ? s->d_deleted : nullptr,
                                                          (uint32_t)s->deleted_words, d_rows, row_words);
  SS_HIP(hipGetLastError());
  return SS_OK;
}

// E[i] &= ~X[row_of[i]]: match sets built under the tombstones alone meet their queries' filters here; d_total[i] = what is left.
// Xq (may be null): query i's row copied out as ITS exclusion bitmap, the one-per-query layout a batched search reads.
__global__ __launch_bounds__(256) void match_exclude_rows_kernel(unsigned long long* __restrict__ E, const unsigned long long* __restrict__ X,
                                                                 const uint32_t* __restrict__ row_of, unsigned long long groups,
                                                                 unsigned long long* __restrict__ total, unsigned long long* __restrict__ Xq) {
  const uint32_t i = blockIdx.y;
  const unsigned long long* x = X + (size_t)row_of[i] * groups;
  unsigned long long* e = E + (size_t)i * groups;
  uint32_t n = 0;
  for (unsigned long long g = (unsigned long long)blockIdx.x * 256u + threadIdx.x; g < groups; g += (unsigned long long)gridDim.x * 256u) {
    const unsigned long long xg = x[g], v = e[g] & ~xg;
    e[g] = v;
    if (Xq) Xq[(size_t)i * groups + g] = xg;
    n += (uint32_t)__popcll(v);
  }
  for (int off = 32; off; off >>= 1) n += __shfl_down(n, off);
  if ((threadIdx.x & 63u) == 0u && n) atomicAdd(&total[i], (unsigned long long)n);
}
int ssi_match_exclude_rows(ss_shard* s, uint32_t nq, unsigned long long* d_E, const unsigned long long* d_X, const uint32_t* d_row_of, uint64_t groups,
                           unsigned long long* d_total, unsigned long long* d_Xq, hipStream_t st) {
  (void)s;
  if (nq == 0 || nq > 64) return SS_EINVAL;
  SS_HIP(hipMemsetAsync(d_total, 0, (size_t)nq * 8, st));
  const unsigned gx = (unsigned)std::min<uint64_t>((groups + 1023) / 1024, 64u);  // (a block walks >= 4 words per thread)
  match_exclude_rows_kernel<<<dim3(std::max(gx, 1u), nq), 256, 0, st>>>(d_E, d_X, d_row_of, groups, d_total, d_Xq);
  SS_HIP(hipGetLastError());
  return SS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Facet counting (facet_count, add_result.rs:484-640): every counted doc adds one to the bucket of its facet value -- a
// string facet's id, or for a numeric facet the range whose lower bound is the last one <= the value (ranges sorted by
// lower bound, binary_search_by_key ... map_or_else(|idx| idx - 1, |idx| idx)).  The counted docs are the query's match
// set after NOT terms, tombstones and the facet filter: the bitmap bm25_union_count_kernel writes from the bit records.
// One thread per 64-doc group walks its set bits; the histogram lives in global memory (64-bit atomics).
__device__ __forceinline__ bool facet_le(uint32_t type, unsigned long long bound, unsigned long long v) {  // bound <= v
  switch (type) {
    case SS_FACET_I8: case SS_FACET_I16: case SS_FACET_I32: case SS_FACET_I64: return (long long)bound <= (long long)v;
    case SS_FACET_F32: return __uint_as_float((uint32_t)bound) <= __uint_as_float((uint32_t)v);
    case SS_FACET_F64: return __longlong_as_double((long long)bound) <= __longlong_as_double((long long)v);
    default: return bound <= v;
  }
}
__global__ void facet_count_kernel(const unsigned long long* __restrict__ bits, unsigned long long n_docs,
                                   const uint8_t* __restrict__ records, uint32_t record_size, uint32_t offset, uint32_t type,
                                   uint32_t n_buckets, const unsigned long long* __restrict__ bounds,
                                   unsigned long long* __restrict__ counts, uint32_t stored_type, FacetPoint pt) {
  const unsigned long long g = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g * 64ull >= n_docs) return;
  unsigned long long m = bits[g];
  static const uint32_t width[] = {1, 2, 4, 8, 1, 2, 4, 8, 4, 8, 2, 4, 8};
  while (m) {
    const unsigned long long d = g * 64ull + (unsigned long long)__builtin_ctzll(m);
    m &= m - 1;
    if (d >= n_docs) break;
    type = stored_type;
    unsigned long long v = facet_load(records + d * record_size + offset, width[stored_type], type, pt);
    if (type == SS_FACET_I8) v = (unsigned long long)(long long)(int8_t)v;      // sign-extend for the comparisons
    else if (type == SS_FACET_I16) v = (unsigned long long)(long long)(int16_t)v;
    else if (type == SS_FACET_I32) v = (unsigned long long)(long long)(int32_t)v;
    uint32_t b;
    if (type == SS_FACET_STRING16 || type == SS_FACET_STRING32) {
      b = v < n_buckets ? (uint32_t)v : n_buckets;
    } else {
      uint32_t lo = 0, hi = n_buckets;  // number of bounds <= v
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (facet_le(type, bounds[mid], v)) lo = mid + 1; else hi = mid;
      }
      b = lo ? lo - 1 : n_buckets;  // below the first bound: the reference's index underflows; reported as "other"
    }
    atomicAdd(&counts[b], 1ull);
  }
}

int ssi_facet_count(ss_shard* s, const unsigned long long* d_bits, uint64_t n_docs, uint32_t offset, uint32_t type, uint32_t n_buckets,
                    const uint64_t* d_bounds, unsigned long long* d_counts, const ss_facet_point* point, hipStream_t st) {
  FacetPoint pt{0, 0, 0};
  if (type == SS_FACET_POINT && facet_point_of(point, &pt) != SS_OK) return SS_EINVAL;
  const uint64_t groups = (n_docs + 63) / 64;
  facet_count_kernel<<<(unsigned)((groups + 255) / 256), 256, 0, st>>>(d_bits, (unsigned long long)n_docs, s->d_facets,
                                                                      s->facet_record_size, offset, type, n_buckets,
                                                                      (const unsigned long long*)d_bounds, d_counts, type, pt);
  SS_HIP(hipGetLastError());
  return SS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Result sort (search.rs ResultSort, min_heap.rs:574-1050 result_ordering_shard): results ordered by facet values -- each
// field ascending or descending, the score last -- instead of by score alone.  The top-k under such an order is found from
// its PIVOT: the k-th best value of the first sort field among the query's matches (a byte-wise radix select over the match
// set: one histogram pass per byte of the field), after which "strictly better than the pivot" and "equal to the pivot" are
// ordinary facet filters on ordinary searches (the hosts compose them: seekstorm_amd/search.py search_lexical_sorted).
// key: the stored value mapped to an unsigned integer that orders like the value (sign bit flipped for integers, the usual
// transform for floats), complemented for an ascending sort, so that a larger key is always the better one.  -0.0 is read as
// +0.0 first: the reference compares floats with partial_cmp (min_heap.rs:807-830), which ties them, so they share one key.
__host__ __device__ inline unsigned long long facet_order_key(unsigned long long v, uint32_t type, uint32_t bits, bool descending) {
  const unsigned long long mask = bits == 64 ? ~0ull : ((1ull << bits) - 1ull), top = 1ull << (bits - 1);
  unsigned long long k = v & mask;
  if (type >= SS_FACET_I8 && type <= SS_FACET_I64) k ^= top;
  else if (type == SS_FACET_F32 || type == SS_FACET_F64) {
    if (k == top) k = 0;  // -0.0 -> +0.0
    k = (k & top) ? (~k & mask) : (k | top);
  }
  return descending ? k : (~k & mask);
}
// the inverse of facet_order_key: the key the two zeros share comes back as +0.0
__host__ inline unsigned long long facet_order_value(unsigned long long k, uint32_t type, uint32_t bits, bool descending) {
  const unsigned long long mask = bits == 64 ? ~0ull : ((1ull << bits) - 1ull), top = 1ull << (bits - 1);
  if (!descending) k = ~k & mask;
  if (type >= SS_FACET_I8 && type <= SS_FACET_I64) k ^= top;
  else if (type == SS_FACET_F32 || type == SS_FACET_F64) k = (k & top) ? (k & ~top) : (~k & mask);
  return k;
}
// histogram of byte `byte_index` (0 = most significant) of the keys that share `prefix` in the bytes above it
__global__ void facet_radix_kernel(const unsigned long long* __restrict__ bits, unsigned long long n_docs,
                                   const uint8_t* __restrict__ records, uint32_t record_size, uint32_t offset, uint32_t type,
                                   uint32_t key_bits, uint32_t descending, unsigned long long prefix, uint32_t byte_index,
                                   unsigned long long* __restrict__ hist, FacetPoint pt) {
  __shared__ unsigned int h[256];
  h[threadIdx.x & 255u] = 0u;
  __syncthreads();
  const unsigned long long g = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g * 64ull < n_docs) {
    unsigned long long m = bits[g];
    const uint32_t shift = key_bits - 8u * (byte_index + 1u);
    while (m) {
      const unsigned long long d = g * 64ull + (unsigned long long)__builtin_ctzll(m);
      m &= m - 1;
      if (d >= n_docs) break;
      uint32_t ty = type;
      const unsigned long long v = facet_load(records + d * record_size + offset, key_bits / 8u, ty, pt);
      const unsigned long long k = facet_order_key(v, ty, key_bits, descending != 0u);
      if (byte_index == 0u || (k >> (shift + 8u)) == prefix) atomicAdd(&h[(k >> shift) & 255u], 1u);
    }
  }
  __syncthreads();
  if (h[threadIdx.x & 255u]) atomicAdd(&hist[threadIdx.x & 255u], (unsigned long long)h[threadIdx.x & 255u]);
}

// k-th best key of the match set `d_bits` (k >= 1; with fewer than k matches: the worst match).  *n_better = matches
// strictly better than it, *n_equal = matches equal to it.  d_hist: 256 counters of workspace.
int ssi_facet_kth(ss_shard* s, const unsigned long long* d_bits, uint64_t n_docs, uint64_t n_matches, uint32_t offset, uint32_t type,
                  bool descending, uint64_t k, unsigned long long* d_hist, uint64_t* value_bits, uint64_t* n_better, uint64_t* n_equal,
                  const ss_facet_point* point, hipStream_t st) {
  if (type == SS_FACET_STRING16 || type == SS_FACET_STRING32) return SS_ENOTSUP;  // they sort by their strings, which live in the host's facet.json
  FacetPoint pt{0, 0, 0};
  if (type == SS_FACET_POINT && facet_point_of(point, &pt) != SS_OK) return SS_EINVAL;  // the key is the f64 distance
  *n_better = 0; *n_equal = 0; *value_bits = 0;
  if (n_matches == 0) return SS_OK;
  const uint32_t key_bits = 8u * ssi_facet_width(type);
  uint64_t want = std::min<uint64_t>(k, n_matches);  // rank (1-based) still to be found inside the current prefix
  unsigned long long prefix = 0;
  const uint64_t groups = (n_docs + 63) / 64;
  unsigned long long hist[256];
  uint64_t equal = 0;
  for (uint32_t b = 0; b < key_bits / 8u; b++) {
    SS_HIP(hipMemsetAsync(d_hist, 0, sizeof(hist), st));
    facet_radix_kernel<<<(unsigned)((groups + 255) / 256), 256, 0, st>>>(d_bits, (unsigned long long)n_docs, s->d_facets, s->facet_record_size,
                                                                        offset, type, key_bits, descending ? 1u : 0u, prefix, b, d_hist, pt);
    SS_HIP(hipGetLastError());
    SS_HIP(hipMemcpyAsync(hist, d_hist, sizeof(hist), hipMemcpyDeviceToHost, st));
    SS_HIP(hipStreamSynchronize(st));
    int v = 255;
    for (; v > 0; v--) {  // from the best byte value down to the bucket that holds the wanted rank
      if (hist[v] >= want) break;
      want -= hist[v];
      *n_better += hist[v];
    }
    prefix = (prefix << 8) | (unsigned long long)v;
    equal = hist[v];
  }
  *n_equal = equal;
  *value_bits = facet_order_value(prefix, type == SS_FACET_POINT ? (uint32_t)SS_FACET_F64 : type, key_bits, descending);
  return SS_OK;
}

__global__ void facet_values_kernel(const uint8_t* __restrict__ records, uint32_t record_size, uint32_t offset, uint32_t bytes,
                                    const uint32_t* __restrict__ docs, uint32_t n, unsigned long long n_docs, unsigned long long* __restrict__ out,
                                    uint32_t type, FacetPoint pt) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = docs[i] < n_docs ? facet_load(records + (size_t)docs[i] * record_size + offset, bytes, type, pt) : 0ull;
}
// point == nullptr: the stored bits (a Point facet's Morton code); with a point: the f64 distance to it
int ssi_facet_values(ss_shard* s, const uint32_t* d_docs, uint32_t n, uint32_t offset, uint32_t type, unsigned long long* d_out,
                     const ss_facet_point* point, hipStream_t st) {
  FacetPoint pt{0, 0, 0};
  uint32_t load_as = type;
  if (type == SS_FACET_POINT) {
    if (!point) load_as = SS_FACET_U64;
    else if (facet_point_of(point, &pt) != SS_OK) return SS_EINVAL;
  }
  if (n) facet_values_kernel<<<(n + 255) / 256, 256, 0, st>>>(s->d_facets, s->facet_record_size, offset, ssi_facet_width(type), d_docs, n,
                                                               (unsigned long long)s->facet_docs, d_out, load_as, pt);
  SS_HIP(hipGetLastError());
  return SS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Result sort for a BATCH, pivots on the device (ss_bm25_search_sorted).  The composition above -- pivot of the first field, a search
// filtered to "better", a search filtered to "equal" that recurses on the next field -- cost a host round trip per radix byte and per
// search.  Here the whole chain stays on the device, per query:
//   E = the match set (bits), B = {} ; per sort field: radix select over E for the k_left-th best key (histogram pass + a one-block
//   decide kernel per byte, the prefix kept in device memory), then a classify pass: docs of E strictly better than the pivot move to
//   B, worse ones leave E; k_left -= |moved|.  After the last field B holds the (< k) docs that are in the answer for sure, E the tie
//   group of the last pivot, of which the best by SCORE fill the rest.  Two ordinary searches under exclusion bitmaps ~B and ~E (the
//   bitmap the kernels honour for tombstones / facet filters) give both lists with their scores; a compose kernel orders B's docs by
//   (field 1, ..., field m, score, doc) -- a bitonic sort of <= 1024 tuples in LDS -- and appends the first k - |B| of E's.
struct SortState { unsigned long long prefix, want, n_better, n_equal, count_e, k_left, better_total, pad; };
struct SortFieldsDev {
  uint32_t n;
  uint32_t offset[SS_MAX_SORT_FIELDS], type[SS_MAX_SORT_FIELDS], bytes[SS_MAX_SORT_FIELDS], desc[SS_MAX_SORT_FIELDS];
  const uint8_t* base[SS_MAX_SORT_FIELDS];  // where the field's keys live: the facet records, or a string facet's rank column
  uint32_t stride[SS_MAX_SORT_FIELDS];
  FacetPoint pt[SS_MAX_SORT_FIELDS];
};
// where every sort field's key is read (facet_commit.h ss_sort_sources)
int ssi_sort_resolve(const ss_shard* s, uint32_t n_sorts, const ss_result_sort* sorts, ss_sort_sources* out) {
  memset(out, 0, sizeof(*out));
  if (n_sorts > SS_MAX_SORT_FIELDS) return SS_EINVAL;
  for (uint32_t f = 0; f < n_sorts; f++) {
    if (sorts[f].facet_type == SS_FACET_STRING16 || sorts[f].facet_type == SS_FACET_STRING32) {
      const uint32_t* col = ssi_facet_rank_column(s, sorts[f].facet_offset, sorts[f].facet_type);
      if (!col) return SS_ENOTSUP;  // no table: the strings live in the host's facet.json
      out->base[f] = (const uint8_t*)col; out->stride[f] = 4u; out->offset[f] = 0u; out->type[f] = SS_FACET_U32;
    } else {
      out->base[f] = s->d_facets; out->stride[f] = s->facet_record_size; out->offset[f] = sorts[f].facet_offset; out->type[f] = sorts[f].facet_type;
    }
  }
  return SS_OK;
}

// (every kernel below: blockIdx.y / blockIdx.x of the one-block kernels = the query of the batch; bit sets [nq][groups], states [nq],
// histograms [nq][256])
__global__ void sort_begin_kernel(SortState* st, const unsigned long long* total, unsigned long long k) {
  st += blockIdx.x;
  if (threadIdx.x == 0) { st->count_e = total[blockIdx.x]; st->k_left = k; st->better_total = 0ull; }
}
// (keep_hist: the histogram already holds the level's byte 0 -- facet_sort_first_kernel counted it)
__global__ void sort_level_begin_kernel(SortState* st, unsigned long long* hist, uint32_t keep_hist) {
  st += blockIdx.x;
  if (!keep_hist) hist[(size_t)blockIdx.x * 256u + (threadIdx.x & 255u)] = 0ull;
  if (threadIdx.x == 0) { st->want = st->k_left < st->count_e ? st->k_left : st->count_e; st->prefix = 0ull; st->n_better = 0ull; st->n_equal = 0ull; }
}
// One byte of the select: the histogram of byte `byte_index` over the docs of E that share the prefix decided so far -- and, on the way,
// the classification by that prefix: a doc above it moves to B, a doc below it leaves E.  E thus shrinks 256-fold per byte, and only
// the first two passes of a field touch every match (each doc's record is a scattered read: they are what a sort by a wide field costs).
__global__ void sort_radix_kernel(unsigned long long* __restrict__ bits, unsigned long long* __restrict__ B, unsigned long long n_docs,
                                  unsigned long long groups, const uint8_t* __restrict__ records, uint32_t record_size, uint32_t offset,
                                  uint32_t type, uint32_t key_bits, uint32_t descending, const SortState* __restrict__ st, uint32_t byte_index,
                                  unsigned long long* __restrict__ hist, FacetPoint pt) {
  __shared__ unsigned int h[256];
  st += blockIdx.y;
  if (st->want == 0ull) return;
  bits += (size_t)blockIdx.y * groups;
  B += (size_t)blockIdx.y * groups;
  hist += (size_t)blockIdx.y * 256u;
  const unsigned long long prefix = st->prefix;
  h[threadIdx.x & 255u] = 0u;
  __syncthreads();
  const unsigned long long g = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g * 64ull < n_docs) {
    const unsigned long long m0 = bits[g];
    unsigned long long m = m0, keep = m0, better = 0ull;
    const uint32_t shift = key_bits - 8u * (byte_index + 1u);
    while (m) {
      const int b = __builtin_ctzll(m);
      const unsigned long long d = g * 64ull + (unsigned long long)b;
      m &= m - 1;
      if (d >= n_docs) break;
      uint32_t ty = type;
      const unsigned long long v = facet_load(records + d * record_size + offset, key_bits / 8u, ty, pt);
      const unsigned long long k = facet_order_key(v, ty, key_bits, descending != 0u);
      if (byte_index == 0u) {
        atomicAdd(&h[(k >> shift) & 255u], 1u);
      } else {
        const unsigned long long kp = k >> (shift + 8u);
        if (kp == prefix) atomicAdd(&h[(k >> shift) & 255u], 1u);
        else { keep &= ~(1ull << b); if (kp > prefix) better |= 1ull << b; }
      }
    }
    if (keep != m0) bits[g] = keep;
    if (better) B[g] |= better;
  }
  __syncthreads();
  if (h[threadIdx.x & 255u]) atomicAdd(&hist[threadIdx.x & 255u], (unsigned long long)h[threadIdx.x & 255u]);
}
// one byte decided: from the best byte value down to the bucket that holds the wanted rank (ssi_facet_kth's host loop)
__global__ void sort_decide_kernel(SortState* st, unsigned long long* hist) {
  st += blockIdx.x;
  hist += (size_t)blockIdx.x * 256u;
  if (threadIdx.x == 0) {
    unsigned long long want = st->want, nb = st->n_better;
    int v = 255;
    if (want != 0ull)
      for (; v > 0; v--) {
        if (hist[v] >= want) break;
        want -= hist[v];
        nb += hist[v];
      }
    st->prefix = (st->prefix << 8) | (unsigned long long)v;
    st->n_equal = st->want != 0ull ? hist[v] : 0ull;
    st->want = want;
    st->n_better = nb;
  }
  __syncthreads();
  hist[threadIdx.x & 255u] = 0ull;
}
// E: docs equal to the pivot stay; strictly better ones move to B; worse ones leave
__global__ void sort_classify_kernel(unsigned long long* __restrict__ E, unsigned long long* __restrict__ B, unsigned long long n_docs,
                                     unsigned long long groups, const uint8_t* __restrict__ records, uint32_t record_size, uint32_t offset,
                                     uint32_t type, uint32_t key_bits, uint32_t descending, const SortState* __restrict__ st, FacetPoint pt) {
  const unsigned long long g = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g * 64ull >= n_docs) return;
  st += blockIdx.y;
  E += (size_t)blockIdx.y * groups;
  B += (size_t)blockIdx.y * groups;
  const unsigned long long pivot = st->prefix;
  unsigned long long m = E[g], keep = 0ull, better = 0ull;
  while (m) {
    const int b = __builtin_ctzll(m);
    const unsigned long long d = g * 64ull + (unsigned long long)b;
    m &= m - 1;
    if (d >= n_docs) break;
    uint32_t ty = type;
    const unsigned long long v = facet_load(records + d * record_size + offset, key_bits / 8u, ty, pt);
    const unsigned long long k = facet_order_key(v, ty, key_bits, descending != 0u);
    if (k > pivot) better |= 1ull << b;
    else if (k == pivot) keep |= 1ull << b;
  }
  E[g] = keep;
  if (better) B[g] |= better;
}
__global__ void sort_level_end_kernel(SortState* st) {
  st += blockIdx.x;
  if (threadIdx.x == 0) { st->k_left -= st->n_better; st->count_e = st->n_equal; st->better_total += st->n_better; }
}
__global__ void sort_excl_kernel(const unsigned long long* __restrict__ E, const unsigned long long* __restrict__ B,
                                 unsigned long long* __restrict__ ex_b, unsigned long long* __restrict__ ex_e, unsigned long long groups) {
  const unsigned long long g = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t o = (size_t)blockIdx.y * groups + g;
  if (g < groups) { ex_b[o] = ~B[o]; ex_e[o] = ~E[o]; }
}
// the answer of one query (blockIdx.x): list A (the docs of B with their scores, any order) ordered by (sort keys, score desc, doc asc),
// then the first k - |A| of list C (the tie group of the last pivot, by score).
// BROWSE (the empty query, ss_docs_search: min_heap.rs:535-536, 1043-1044): nobody has a score -- a_score, c_score and out_score are not
// read or written -- and the order after the sort keys is the doc id alone, 1 = the larger id first (the crate's default), 2 = the smaller.
template <int BROWSE>
__global__ void __launch_bounds__(1024) sort_compose_kernel(const uint32_t* __restrict__ a_doc, const float* __restrict__ a_score,
                                                            const uint32_t* __restrict__ a_cnt, const uint32_t* __restrict__ c_doc,
                                                            const float* __restrict__ c_score, const uint32_t* __restrict__ c_cnt,
                                                            const unsigned long long* __restrict__ total, unsigned long long n_facet_docs,
                                                            SortFieldsDev F, uint32_t k,
                                                            uint32_t* __restrict__ out_doc, float* __restrict__ out_score,
                                                            uint32_t* __restrict__ out_count, unsigned long long* __restrict__ out_total) {
  __shared__ unsigned long long key[SS_MAX_SORT_FIELDS][1024];
  __shared__ float sc[1024];
  __shared__ uint32_t dc[1024];
  __shared__ uint16_t perm[1024];
  const uint32_t i = threadIdx.x, q = blockIdx.x;
  a_doc += (size_t)q * k; c_doc += (size_t)q * k; out_doc += (size_t)q * k;
  if (!BROWSE) { a_score += (size_t)q * k; c_score += (size_t)q * k; out_score += (size_t)q * k; }
  const uint32_t na = min(a_cnt[q] == 0xFFFFFFFFu ? 0u : a_cnt[q], k);
  const uint32_t nc = min(c_cnt[q] == 0xFFFFFFFFu ? 0u : c_cnt[q], k - na);
  perm[i] = (uint16_t)i;
  dc[i] = i < na ? a_doc[i] : 0xFFFFFFFFu;
  sc[i] = BROWSE ? 0.f : (i < na ? a_score[i] : -INFINITY);
  for (uint32_t f = 0; f < (uint32_t)SS_MAX_SORT_FIELDS; f++) {
    unsigned long long kk = 0ull;
    if (i < na && f < F.n && dc[i] < n_facet_docs) {
      uint32_t ty = F.type[f];
      const unsigned long long v = facet_load(F.base[f] + (size_t)dc[i] * F.stride[f] + F.offset[f], F.bytes[f], ty, F.pt[f]);
      kk = facet_order_key(v, ty, 8u * F.bytes[f], F.desc[f] != 0u);
    }
    key[f][i] = kk;
  }
  __syncthreads();
  auto before = [&](uint32_t a, uint32_t b) -> bool {  // a stands before b in the answer
    const bool la = a < na, lb = b < na;
    if (la != lb) return la;
    if (!la) return a < b;
    for (uint32_t f = 0; f < F.n; f++)
      if (key[f][a] != key[f][b]) return key[f][a] > key[f][b];
    if (!BROWSE && sc[a] != sc[b]) return sc[a] > sc[b];
    return BROWSE == 1 ? dc[a] > dc[b] : dc[a] < dc[b];
  };
  for (uint32_t size = 2; size <= 1024u; size <<= 1)
    for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
      const uint32_t j = i ^ stride;
      if (j > i) {
        const uint32_t a = perm[i], b = perm[j];
        const bool up = (i & size) == 0u;  // ascending block: the better one first
        if (up ? before(b, a) : before(a, b)) { perm[i] = (uint16_t)b; perm[j] = (uint16_t)a; }
      }
      __syncthreads();
    }
  if (i < na) { out_doc[i] = dc[perm[i]]; if (!BROWSE) out_score[i] = sc[perm[i]]; }
  else if (i < na + nc) { out_doc[i] = c_doc[i - na]; if (!BROWSE) out_score[i] = c_score[i - na]; }
  else if (i < k) { out_doc[i] = 0xFFFFFFFFu; if (!BROWSE) out_score[i] = 0.f; }
  if (i == 0) { out_count[q] = na + nc; out_total[q] = total[q]; }
}

// the device chain of nq queries up to the exclusion bitmaps (the caller then runs the two searches and ssi_sort_compose);
// bit sets [nq][groups], d_total / d_state [nq], d_hist [nq][256].  d_ex_b = nullptr: no exclusion bitmaps (ss_docs_search reads B and E)
int ssi_sort_select(ss_shard* s, uint32_t nq, unsigned long long* d_E, unsigned long long* d_B, unsigned long long* d_ex_b, unsigned long long* d_ex_e,
                    const unsigned long long* d_total, unsigned long long* d_hist, void* d_state, uint32_t n_sorts, const ss_result_sort* sorts,
                    const ss_sort_sources& src, uint32_t k, hipStream_t st, bool byte0_counted) {
  const unsigned long long n_docs = s->bm_n_docs, groups = (unsigned long long)s->bm_n_sub * (BM_SUB / 64);
  const dim3 grid((unsigned)((groups + 255) / 256), nq);
  SortState* state = (SortState*)d_state;
  SS_HIP(hipMemsetAsync(d_B, 0, (size_t)nq * groups * 8, st));
  sort_begin_kernel<<<nq, 64, 0, st>>>(state, d_total, (unsigned long long)k);
  for (uint32_t f = 0; f < n_sorts; f++) {
    const uint32_t type = src.type[f];
    FacetPoint pt{0, 0, 0};
    if (type == SS_FACET_POINT) {
      const ss_facet_point base{sorts[f].base_lat, sorts[f].base_lon, SS_POINT_SORTKEY, 0};
      if (facet_point_of(&base, &pt) != SS_OK) return SS_EINVAL;
    }
    const uint32_t key_bits = 8u * ssi_facet_width(type);
    const bool counted = byte0_counted && f == 0;  // pass 0 only counts (it never modifies E): the histogram is all it leaves
    sort_level_begin_kernel<<<nq, 256, 0, st>>>(state, d_hist, counted ? 1u : 0u);
    for (uint32_t b = 0; b < key_bits / 8u; b++) {
      if (!(counted && b == 0))
        sort_radix_kernel<<<grid, 256, 0, st>>>(d_E, d_B, n_docs, groups, src.base[f], src.stride[f], src.offset[f], type, key_bits,
                                                sorts[f].descending ? 1u : 0u, state, b, d_hist, pt);
      sort_decide_kernel<<<nq, 256, 0, st>>>(state, d_hist);
    }
    sort_classify_kernel<<<grid, 256, 0, st>>>(d_E, d_B, n_docs, groups, src.base[f], src.stride[f], src.offset[f], type, key_bits,
                                               sorts[f].descending ? 1u : 0u, state, pt);
    sort_level_end_kernel<<<nq, 64, 0, st>>>(state);
  }
  if (d_ex_b) sort_excl_kernel<<<grid, 256, 0, st>>>(d_E, d_B, d_ex_b, d_ex_e, groups);
  SS_HIP(hipGetLastError());
  return SS_OK;
}
static int sort_fields_dev(uint32_t n_sorts, const ss_result_sort* sorts, const ss_sort_sources& src, SortFieldsDev* out) {
  SortFieldsDev& F = *out;
  memset(&F, 0, sizeof(F));
  F.n = n_sorts;
  for (uint32_t f = 0; f < n_sorts; f++) {
    F.base[f] = src.base[f]; F.stride[f] = src.stride[f];
    F.offset[f] = src.offset[f]; F.type[f] = src.type[f]; F.bytes[f] = ssi_facet_width(src.type[f]); F.desc[f] = sorts[f].descending ? 1u : 0u;
    if (sorts[f].facet_type == SS_FACET_POINT) {
      const ss_facet_point base{sorts[f].base_lat, sorts[f].base_lon, SS_POINT_SORTKEY, 0};
      if (facet_point_of(&base, &F.pt[f]) != SS_OK) return SS_EINVAL;
    }
  }
  return SS_OK;
}
// the browse order of ONE answer (ss_docs_search): list A by (sort keys, doc id), then the first k - |A| of list C; no scores
int ssi_sort_compose_browse(ss_shard* s, const uint32_t* a_doc, const uint32_t* a_cnt, const uint32_t* c_doc, const uint32_t* c_cnt,
                            const unsigned long long* d_total, uint32_t n_sorts, const ss_result_sort* sorts, const ss_sort_sources& src, uint32_t k,
                            bool doc_ascending, uint32_t* out_doc, uint32_t* out_count, unsigned long long* out_total, hipStream_t st) {
  if (k == 0 || k > 1024u) return SS_EINVAL;  // (one tuple per thread)
  SortFieldsDev F;
  if (sort_fields_dev(n_sorts, sorts, src, &F) != SS_OK) return SS_EINVAL;
  if (doc_ascending)
    sort_compose_kernel<2><<<1, 1024, 0, st>>>(a_doc, nullptr, a_cnt, c_doc, nullptr, c_cnt, d_total, (unsigned long long)s->facet_docs, F, k,
                                                out_doc, nullptr, out_count, out_total);
  else
    sort_compose_kernel<1><<<1, 1024, 0, st>>>(a_doc, nullptr, a_cnt, c_doc, nullptr, c_cnt, d_total, (unsigned long long)s->facet_docs, F, k,
                                                out_doc, nullptr, out_count, out_total);
  SS_HIP(hipGetLastError());
  return SS_OK;
}
// lists [nq][k], counts / totals / outputs per query
int ssi_sort_compose(ss_shard* s, uint32_t nq, const uint32_t* a_doc, const float* a_score, const uint32_t* a_cnt, const uint32_t* c_doc,
                     const float* c_score, const uint32_t* c_cnt, const unsigned long long* d_total, uint32_t n_sorts, const ss_result_sort* sorts,
                     const ss_sort_sources& src, uint32_t k, uint32_t* out_doc, float* out_score, uint32_t* out_count, unsigned long long* out_total,
                     hipStream_t st) {
  SortFieldsDev F;
  if (sort_fields_dev(n_sorts, sorts, src, &F) != SS_OK) return SS_EINVAL;
  sort_compose_kernel<0><<<nq, 1024, 0, st>>>(a_doc, a_score, a_cnt, c_doc, c_score, c_cnt, d_total, (unsigned long long)s->facet_docs, F, k,
                                           out_doc, out_score, out_count, out_total);
  SS_HIP(hipGetLastError());
  return SS_OK;
}

// the signatures ss_common.h declares: the sort's sources resolved here
int ssi_sort_select(ss_shard* s, uint32_t nq, unsigned long long* d_E, unsigned long long* d_B, unsigned long long* d_ex_b, unsigned long long* d_ex_e,
                    const unsigned long long* d_total, unsigned long long* d_hist, void* d_state, uint32_t n_sorts, const ss_result_sort* sorts,
                    uint32_t k, hipStream_t st) {
  ss_sort_sources src;
  const int rc = ssi_sort_resolve(s, n_sorts, sorts, &src);
  return rc != SS_OK ? rc : ssi_sort_select(s, nq, d_E, d_B, d_ex_b, d_ex_e, d_total, d_hist, d_state, n_sorts, sorts, src, k, st);
}
int ssi_sort_compose(ss_shard* s, uint32_t nq, const uint32_t* a_doc, const float* a_score, const uint32_t* a_cnt, const uint32_t* c_doc,
                     const float* c_score, const uint32_t* c_cnt, const unsigned long long* d_total, uint32_t n_sorts, const ss_result_sort* sorts,
                     uint32_t k, uint32_t* out_doc, float* out_score, uint32_t* out_count, unsigned long long* out_total, hipStream_t st) {
  ss_sort_sources src;
  const int rc = ssi_sort_resolve(s, n_sorts, sorts, &src);
  return rc != SS_OK ? rc : ssi_sort_compose(s, nq, a_doc, a_score, a_cnt, c_doc, c_score, c_cnt, d_total, n_sorts, sorts, src, k, out_doc, out_score,
                                             out_count, out_total, st);
}
// ... no base point
int ssi_facet_kth(ss_shard* s, const unsigned long long* d_bits, uint64_t n_docs, uint64_t n_matches, uint32_t offset, uint32_t type,
                  bool descending, uint64_t k, unsigned long long* d_hist, uint64_t* value_bits, uint64_t* n_better, uint64_t* n_equal,
                  hipStream_t st) {
  return ssi_facet_kth(s, d_bits, n_docs, n_matches, offset, type, descending, k, d_hist, value_bits, n_better, n_equal, nullptr, st);
}
int ssi_facet_values(ss_shard* s, const uint32_t* d_docs, uint32_t n, uint32_t offset, uint32_t type, unsigned long long* d_out, hipStream_t st) {
  return ssi_facet_values(s, d_docs, n, offset, type, d_out, nullptr, st);
}
int ssi_facet_count(ss_shard* s, const unsigned long long* d_bits, uint64_t n_docs, uint32_t offset, uint32_t type, uint32_t n_buckets,
                    const uint64_t* d_bounds, unsigned long long* d_counts, hipStream_t st) {
  return ssi_facet_count(s, d_bits, n_docs, offset, type, n_buckets, d_bounds, d_counts, nullptr, st);
}

// ---------------------------------------------------------------------------------------------------------------
// Facet counts of a BATCH: every requested facet of every query in ONE launch (ss_bm25_search_facets; query_facets of a search,
// add_result.rs:487-643 bumps every facet for every counted doc).  blockIdx.y = the query, blockIdx.x = a slice of 256 * wpt words of
// its match bitmap.  The slice's matches are COMPACTED onto the lanes: a popcount prefix over the slice's words (in LDS), then match i
// of the slice is found by a binary search over the prefix and a rank select inside the word -- a 1 % match set keeps every lane
// busy where one thread per 64-doc group would leave 99 % idle.  A matched doc's record is visited once for all its facets.
// Counters are 32-bit LDS histograms (FM_LDS_COUNTERS words shared by the facets that fit, in facet order), flushed once per
// workgroup with one 64-bit global atomic per non-zero counter; a facet of <= FM_AGGREGATE buckets adds lane-aggregated (one add per
// distinct bucket of the wave).  A facet whose counters do not fit (string facets of many ids) counts straight into global memory:
// its ids spread over many lines.  Bounds of the range facets are staged in LDS (the first FM_LDS_BOUNDS of them).
// LDS: 4 KiB words + 2 KiB prefix + 8 KiB counters + 4 KiB bounds = 18 KiB: eight workgroups (32 waves) per CU.
constexpr uint32_t FM_THREADS = 256, FM_MAX_WPT = 2, FM_LDS_COUNTERS = 2048, FM_LDS_BOUNDS = 512, FM_AGGREGATE = 16, FM_NO_LDS = 0xFFFFFFFFu;
struct FacetMultiDesc {
  uint32_t offset, type, n_buckets;
  uint32_t bounds_begin;  // of its lower bounds inside the batch's bounds (range facets)
  uint32_t cnt_begin;     // of its n_buckets + 1 counters inside a query's row
  uint32_t lds_begin;     // of its LDS counters, FM_NO_LDS: counts in global memory
  FacetPoint pt;
};
struct FacetMulti {
  uint32_t n, lds_used, n_bounds, pad;
  unsigned long long stride;  // counters per query
  FacetMultiDesc f[SS_MAX_QUERY_FACETS];
};

// the bucket of one doc's value: facet_count_kernel's rule, word for word
__device__ __forceinline__ uint32_t facet_bucket(const uint8_t* p, uint32_t stored_type, uint32_t n_buckets, const unsigned long long* bounds,
                                                 const FacetPoint& pt) {
  static const uint32_t width[] = {1, 2, 4, 8, 1, 2, 4, 8, 4, 8, 2, 4, 8};
  uint32_t type = stored_type;
  unsigned long long v = facet_load(p, width[stored_type], type, pt);
  if (type == SS_FACET_I8) v = (unsigned long long)(long long)(int8_t)v;      // sign-extend for the comparisons
  else if (type == SS_FACET_I16) v = (unsigned long long)(long long)(int16_t)v;
  else if (type == SS_FACET_I32) v = (unsigned long long)(long long)(int32_t)v;
  if (type == SS_FACET_STRING16 || type == SS_FACET_STRING32) return v < n_buckets ? (uint32_t)v : n_buckets;
  uint32_t lo = 0, hi = n_buckets;  // number of bounds <= v
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (facet_le(type, bounds[mid], v)) lo = mid + 1; else hi = mid;
  }
  return lo ? lo - 1 : n_buckets;  // below the first bound (or NaN): "other"
}
// The sort field whose first radix byte facet_sort_first_kernel counts beside the facets (ss_sort_sources' entry 0 of the call)
struct FacetSortKey {
  const uint8_t* base;  // the facet records, or a string facet's rank column
  uint32_t stride, offset, type, key_bits, descending;
  FacetPoint pt;
};
// The body both kernels share.  SORT: every matched doc's key of sort field 0 is loaded too (facet_load + facet_order_key, as
// sort_radix_kernel does) and its TOP byte counted into a 256-counter LDS histogram of its own (1 KiB beside the 18 KiB above: eight
// workgroups per CU still fit), flushed into hist [nq][256] -- what sort_radix_kernel's pass 0 of field 0 would count, without its
// second visit of every match (ssi_sort_select, byte0_counted).
template <bool SORT>
__device__ __forceinline__ void facet_multi_body(const unsigned long long* __restrict__ bits, unsigned long long groups,
                                                 unsigned long long n_docs, const uint8_t* __restrict__ records,
                                                 uint32_t record_size, uint32_t wpt, const unsigned long long* __restrict__ bounds,
                                                 unsigned long long* __restrict__ counts, const FacetMulti& F, const FacetSortKey& K,
                                                 unsigned long long* __restrict__ hist) {
  __shared__ uint32_t s_radix[SORT ? 256 : 1];
  __shared__ unsigned long long s_word[FM_THREADS * FM_MAX_WPT];
  __shared__ uint32_t s_pre[FM_THREADS * FM_MAX_WPT + 1];
  __shared__ uint32_t s_wave[FM_THREADS / 64];
  __shared__ uint32_t s_cnt[FM_LDS_COUNTERS];
  __shared__ unsigned long long s_bounds[FM_LDS_BOUNDS];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t W = FM_THREADS * wpt;  // words of this slice (wpt <= FM_MAX_WPT)
  const unsigned long long w0 = (unsigned long long)blockIdx.x * W;
  bits += (size_t)blockIdx.y * groups;
  counts += (size_t)blockIdx.y * F.stride;
  unsigned long long mw[FM_MAX_WPT];
  uint32_t c = 0;
  for (uint32_t j = 0; j < FM_MAX_WPT; j++) {
    mw[j] = 0ull;
    if (j < wpt) {
      const unsigned long long g = w0 + (unsigned long long)tid * wpt + j;
      unsigned long long m = g < groups ? bits[g] : 0ull;
      if (m && g * 64ull + 64ull > n_docs) m = g * 64ull >= n_docs ? 0ull : (m & ((1ull << (n_docs - g * 64ull)) - 1ull));  // no doc behind the last
      mw[j] = m;
      s_word[tid * wpt + j] = m;
      c += (uint32_t)__popcll(m);
    }
  }
  uint32_t inc = c;  // inclusive scan of the threads' match counts: inside the wave, then over the waves
  for (uint32_t o = 1; o < 64u; o <<= 1) {
    const uint32_t y = __shfl_up(inc, o);
    if (lane >= o) inc += y;
  }
  if (lane == 63u) s_wave[wave] = inc;
  __syncthreads();
  uint32_t base = 0, T = 0;
  for (uint32_t w = 0; w < FM_THREADS / 64; w++) { if (w < wave) base += s_wave[w]; T += s_wave[w]; }
  if (T == 0) return;  // (the whole workgroup: nothing matched in this slice)
  uint32_t e = base + inc - c;
  for (uint32_t j = 0; j < FM_MAX_WPT; j++)
    if (j < wpt) { s_pre[tid * wpt + j] = e; e += (uint32_t)__popcll(mw[j]); }
  if (tid == 0) s_pre[W] = T;
  for (uint32_t i = tid; i < F.lds_used; i += FM_THREADS) s_cnt[i] = 0u;
  if (SORT) s_radix[tid & 255u] = 0u;
  const uint32_t nb_lds = F.n_bounds < FM_LDS_BOUNDS ? F.n_bounds : FM_LDS_BOUNDS;
  for (uint32_t i = tid; i < nb_lds; i += FM_THREADS) s_bounds[i] = bounds[i];
  __syncthreads();
  for (uint32_t i = tid; i < T; i += FM_THREADS) {
    uint32_t lo = 0, hi = W;  // s_pre[lo] <= i < s_pre[hi]: the word that holds match i
    while (hi - lo > 1u) {
      const uint32_t mid = (lo + hi) >> 1;
      if (s_pre[mid] <= i) lo = mid; else hi = mid;
    }
    const unsigned long long d = (w0 + lo) * 64ull + facet_select64(s_word[lo], i - s_pre[lo]);  // < n_docs: the words were masked
    const uint8_t* rec = records + d * record_size;
    if (SORT) {
      uint32_t ty = K.type;
      const unsigned long long v = facet_load(K.base + d * K.stride + K.offset, K.key_bits / 8u, ty, K.pt);
      const uint32_t top = (uint32_t)(facet_order_key(v, ty, K.key_bits, K.descending != 0u) >> (K.key_bits - 8u)) & 255u;
      const unsigned long long active = __ballot(1);  // keys of one wave mostly share their top byte: then one add for all of them
      const uint32_t first = (uint32_t)__shfl((int)top, __builtin_ctzll(active));
      if (__ballot(top == first) == active) { if ((int)lane == __builtin_ctzll(active)) atomicAdd(&s_radix[first], (uint32_t)__popcll(active)); }
      else atomicAdd(&s_radix[top], 1u);
    }
    for (uint32_t f = 0; f < F.n; f++) {
      const FacetMultiDesc& D = F.f[f];
      const unsigned long long* bnd = D.bounds_begin + D.n_buckets <= nb_lds ? s_bounds + D.bounds_begin : bounds + D.bounds_begin;
      const uint32_t b = facet_bucket(rec + D.offset, D.type, D.n_buckets, bnd, D.pt);
      if (D.n_buckets <= FM_AGGREGATE) {  // few buckets: one add per distinct bucket of the wave
        unsigned long long todo = __ballot(1);
        while (todo) {
          const int leader = __builtin_ctzll(todo);
          const uint32_t lb = (uint32_t)__shfl((int)b, leader);
          const unsigned long long same = __ballot(b == lb) & todo;
          if ((int)lane == leader) {
            if (D.lds_begin != FM_NO_LDS) atomicAdd(&s_cnt[D.lds_begin + lb], (uint32_t)__popcll(same));
            else atomicAdd(&counts[D.cnt_begin + lb], (unsigned long long)__popcll(same));
          }
          todo &= ~same;
        }
      } else if (D.lds_begin != FM_NO_LDS) {
        atomicAdd(&s_cnt[D.lds_begin + b], 1u);
      } else {
        atomicAdd(&counts[D.cnt_begin + b], 1ull);
      }
    }
  }
  __syncthreads();
  for (uint32_t f = 0; f < F.n; f++) {
    const FacetMultiDesc& D = F.f[f];
    if (D.lds_begin == FM_NO_LDS) continue;
    for (uint32_t i = tid; i <= D.n_buckets; i += FM_THREADS) {
      const uint32_t v = s_cnt[D.lds_begin + i];
      if (v) atomicAdd(&counts[D.cnt_begin + i], (unsigned long long)v);
    }
  }
  if (SORT && tid < 256u && s_radix[tid]) atomicAdd(&hist[(size_t)blockIdx.y * 256u + tid], (unsigned long long)s_radix[tid]);
}
__global__ void __launch_bounds__(FM_THREADS) facet_multi_kernel(const unsigned long long* __restrict__ bits, unsigned long long groups,
                                                                 unsigned long long n_docs, const uint8_t* __restrict__ records,
                                                                 uint32_t record_size, uint32_t wpt, const unsigned long long* __restrict__ bounds,
                                                                 unsigned long long* __restrict__ counts, FacetMulti F) {
  facet_multi_body<false>(bits, groups, n_docs, records, record_size, wpt, bounds, counts, F, FacetSortKey{}, nullptr);
}
// facet_multi_kernel + the histogram of the top byte of sort field 0's keys: the first pass of a sorted search that counts facets too
// (ss_bm25_search_sorted_facets).  hist [nq][256], zeroed by the caller.
__global__ void __launch_bounds__(FM_THREADS) facet_sort_first_kernel(const unsigned long long* __restrict__ bits, unsigned long long groups,
                                                                      unsigned long long n_docs, const uint8_t* __restrict__ records,
                                                                      uint32_t record_size, uint32_t wpt,
                                                                      const unsigned long long* __restrict__ bounds,
                                                                      unsigned long long* __restrict__ counts, FacetMulti F, FacetSortKey K,
                                                                      unsigned long long* __restrict__ hist) {
  facet_multi_body<true>(bits, groups, n_docs, records, record_size, wpt, bounds, counts, F, K, hist);
}

// d_bits [nq][groups] match sets, d_bounds: the range facets' lower bounds back to back in facet order, d_counts [nq][sum_f (n_buckets[f] + 1)]
// (zeroed by the caller).  The arguments were validated by the caller (types, bases, offsets inside the record).
static int facet_multi_desc(uint32_t nq, uint32_t n_facets, const uint32_t* offset, const uint32_t* type, const uint32_t* n_buckets,
                            const ss_facet_point* bases, FacetMulti* out) {
  if (nq == 0 || nq > 65535u || n_facets == 0 || n_facets > SS_MAX_QUERY_FACETS) return SS_EINVAL;
  FacetMulti& F = *out;
  memset(&F, 0, sizeof(F));
  F.n = n_facets;
  for (uint32_t f = 0; f < n_facets; f++) {
    FacetMultiDesc& D = F.f[f];
    D.offset = offset[f]; D.type = type[f]; D.n_buckets = n_buckets[f];
    D.pt = FacetPoint{0, 0, 0};
    if (type[f] == SS_FACET_POINT && facet_point_of(bases ? bases + f : nullptr, &D.pt) != SS_OK) return SS_EINVAL;
    const bool strings = type[f] == SS_FACET_STRING16 || type[f] == SS_FACET_STRING32;
    D.bounds_begin = F.n_bounds;
    if (!strings) F.n_bounds += n_buckets[f];
    D.cnt_begin = (uint32_t)F.stride;
    F.stride += (unsigned long long)n_buckets[f] + 1ull;
    D.lds_begin = FM_NO_LDS;
    if (n_buckets[f] + 1u <= FM_LDS_COUNTERS - F.lds_used) { D.lds_begin = F.lds_used; F.lds_used += n_buckets[f] + 1u; }
  }
  return SS_OK;
}
// two words per thread unless that leaves the chip short of workgroups
static uint32_t facet_multi_wpt(unsigned long long groups, uint32_t nq) {
  return ((groups + 2 * FM_THREADS - 1) / (2 * FM_THREADS)) * nq >= 2048u ? 2u : 1u;
}
int ssi_facet_count_multi(ss_shard* s, uint32_t nq, const unsigned long long* d_bits, uint32_t n_facets, const uint32_t* offset, const uint32_t* type,
                          const uint32_t* n_buckets, const ss_facet_point* bases, const uint64_t* d_bounds, unsigned long long* d_counts,
                          hipStream_t st) {
  FacetMulti F;
  if (const int rc = facet_multi_desc(nq, n_facets, offset, type, n_buckets, bases, &F)) return rc;
  const unsigned long long groups = (unsigned long long)s->bm_n_sub * (BM_SUB / 64);
  const uint32_t wpt = facet_multi_wpt(groups, nq);
  const dim3 grid((unsigned)((groups + (unsigned long long)FM_THREADS * wpt - 1) / ((unsigned long long)FM_THREADS * wpt)), nq);
  facet_multi_kernel<<<grid, FM_THREADS, 0, st>>>(d_bits, groups, (unsigned long long)s->bm_n_docs, s->d_facets, s->facet_record_size, wpt,
                                                  (const unsigned long long*)d_bounds, d_counts, F);
  SS_HIP(hipGetLastError());
  return SS_OK;
}
// ssi_facet_count_multi's counters AND, in the same launch, the histogram of the top byte of sort field 0's keys over every query's
// match set into d_hist [nq][256] (cleared here): what pass 0 of ssi_sort_select's first field counts -- hand it byte0_counted = true.
int ssi_facet_sort_first(ss_shard* s, uint32_t nq, const unsigned long long* d_bits, uint32_t n_facets, const uint32_t* offset, const uint32_t* type,
                         const uint32_t* n_buckets, const ss_facet_point* bases, const uint64_t* d_bounds, unsigned long long* d_counts,
                         const ss_result_sort* sorts, const ss_sort_sources& src, unsigned long long* d_hist, hipStream_t st) {
  FacetMulti F;
  if (const int rc = facet_multi_desc(nq, n_facets, offset, type, n_buckets, bases, &F)) return rc;
  FacetSortKey K{src.base[0], src.stride[0], src.offset[0], src.type[0], 8u * ssi_facet_width(src.type[0]), sorts[0].descending ? 1u : 0u,
                 FacetPoint{0, 0, 0}};
  if (K.type == SS_FACET_POINT) {
    const ss_facet_point base{sorts[0].base_lat, sorts[0].base_lon, SS_POINT_SORTKEY, 0};
    if (facet_point_of(&base, &K.pt) != SS_OK) return SS_EINVAL;
  }
  const unsigned long long groups = (unsigned long long)s->bm_n_sub * (BM_SUB / 64);
  const uint32_t wpt = facet_multi_wpt(groups, nq);
  const dim3 grid((unsigned)((groups + (unsigned long long)FM_THREADS * wpt - 1) / ((unsigned long long)FM_THREADS * wpt)), nq);
  SS_HIP(hipMemsetAsync(d_hist, 0, (size_t)nq * 256 * 8, st));
  facet_sort_first_kernel<<<grid, FM_THREADS, 0, st>>>(d_bits, groups, (unsigned long long)s->bm_n_docs, s->d_facets, s->facet_record_size, wpt,
                                                       (const unsigned long long*)d_bounds, d_counts, F, K, d_hist);
  SS_HIP(hipGetLastError());
  return SS_OK;
}
