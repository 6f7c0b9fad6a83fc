// Facet filters on the host: the checks and the completion of ONE filter that ssi_facet_build (facet.hip) and a batch with a filter set
// PER QUERY (ss_bm25_search_each, api_each.hip) share, and the grouping of such a batch's filter sets into exclusion ROWS -- one row
// per distinct set, row_of[query] says which (facet.hip facet_filter_rows_kernel writes them, match_exclude_rows_kernel applies them).
// Header-only and free of HIP types: tests/filter_rows_check.cpp compiles it with a plain C++ compiler.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/seekstorm_hip.h"

// bytes a facet of `type` (<= SS_FACET_POINT, checked by the caller) takes in the record; a Point is its 8-byte Morton code.  (The
// sorts never read a string's id: a string sort field resolves to its u32 rank column, facet_commit.h, or is refused.)  The kernels keep their own device-side tables.
inline uint32_t ssi_facet_width(uint32_t type) {
  static const uint8_t width[] = {1, 2, 4, 8, 1, 2, 4, 8, 4, 8, 2, 4, 8};
  return width[type];
}

// ---- Point facets, the host's half (facet.hip has the distances): the Morton code of (lat, lon) x 1e7 as i32 (geo_search.rs:27-41)
static constexpr double kDeg2Rad = 0.017453292519943295, kEarthKm = 6371.0087714, kEarthMi = 3958.761315801475;
inline unsigned long long morton_spread(uint32_t v) {
  unsigned long long x = v;
  x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
  x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
  x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
  x = (x | (x << 2)) & 0x3333333333333333ull;
  x = (x | (x << 1)) & 0x5555555555555555ull;
  return x;
}
inline uint32_t morton_coord(double degrees) {  // (v * 1e7) as i32 as u32: Rust's cast truncates, saturates, NaN -> 0
  const double v = degrees * 10000000.0;
  int32_t i;
  if (v != v) i = 0;
  else if (v >= 2147483647.0) i = INT32_MAX;
  else if (v <= -2147483648.0) i = INT32_MIN;
  else i = (int32_t)v;
  return (uint32_t)i;
}
inline unsigned long long morton_encode(double lat, double lon) { return (morton_spread(morton_coord(lon)) << 1) | morton_spread(morton_coord(lat)); }

inline bool ssi_filter_is_extern(const ss_facet_filter& f) {
  return (f.type == SS_FACET_STRING16 || f.type == SS_FACET_STRING32) && f.n_values == SS_FACET_IDS_EXTERN;
}

// ONE filter against a record of record_size bytes, as every entry checks it (SS_EINVAL: a type beyond SS_FACET_POINT, a field beyond
// the record, more than 8 inline string ids, an id array that is missing, a Point unit beyond SS_POINT_MILES), and *out = the filter as
// the device reads it: a Point distance filter with the Morton corners of its box in values[4..7].  The ids of an SS_FACET_IDS_EXTERN
// filter stay where they are: its caller turns them into a bitmap on the device.
inline int ssi_filter_prepare(const ss_facet_filter& f, uint32_t record_size, ss_facet_filter* out) {
  if (f.type > SS_FACET_POINT || f.offset + ssi_facet_width(f.type) > record_size) return SS_EINVAL;
  const bool strings = f.type == SS_FACET_STRING16 || f.type == SS_FACET_STRING32;
  if (strings && f.n_values > 8 && f.n_values != SS_FACET_IDS_EXTERN) return SS_EINVAL;
  if (strings && f.n_values == SS_FACET_IDS_EXTERN && f.hi && !(const uint32_t*)(uintptr_t)f.lo) return SS_EINVAL;
  *out = f;
  if (f.type == SS_FACET_POINT) {
    if (f.n_values > SS_POINT_MILES) return SS_EINVAL;
    if (f.n_values != SS_POINT_SORTKEY) {
      // point_distance_to_morton_range(base, distance_range.end, unit), search.rs:2712-2722 / geo_search.rs:128-144: the
      // codes of the two corners of the box around the base -- a range of the Z-ORDER, as the reference compares it
      double lat, lon, end;
      unsigned long long w0 = (unsigned long long)f.values[0] | ((unsigned long long)f.values[1] << 32),
                         w1 = (unsigned long long)f.values[2] | ((unsigned long long)f.values[3] << 32);
      memcpy(&lat, &w0, 8); memcpy(&lon, &w1, 8); memcpy(&end, &f.hi, 8);
      const double radius = f.n_values == SS_POINT_KM ? kEarthKm : kEarthMi;
      const double lat_delta = end / (kDeg2Rad * radius), lon_delta = end / (kDeg2Rad * radius * cos(kDeg2Rad * lat));
      const unsigned long long m0 = morton_encode(lat - lat_delta, lon - lon_delta), m1 = morton_encode(lat + lat_delta, lon + lon_delta);
      out->values[4] = (uint32_t)m0; out->values[5] = (uint32_t)(m0 >> 32);
      out->values[6] = (uint32_t)m1; out->values[7] = (uint32_t)(m1 >> 32);
    }
  }
  return SS_OK;
}

// The filter sets of nq queries -- query i's filters are filters[filter_begin[i] .. filter_begin[i + 1]) -- grouped into rows.
//   row_of[i]   the row of query i; byte-equal sets share one, rows are numbered in the order their first query comes; SS_ROW_SLOW for
//               a query whose set holds an SS_FACET_IDS_EXTERN filter: it has no row and runs alone through the single-filter entry
//   row_begin   [n_rows + 1]: row r's filters are prepared[row_begin[r] .. row_begin[r + 1]) (ssi_filter_prepare's form); an empty set
//               is a row without filters -- the tombstones alone
// SS_EINVAL: filter_begin missing or not ascending, filters missing where a set is not empty, a set of more than SS_MAX_FACET_FILTERS,
// a filter ssi_filter_prepare refuses (those of the slow queries too).
#define SS_ROW_SLOW 0xFFFFFFFFu
struct ss_filter_rows {
  uint32_t n_rows = 0, n_slow = 0;
  std::vector<uint32_t> row_of, row_begin;
  std::vector<ss_facet_filter> prepared;
};
inline int ssi_filter_rows(uint32_t nq, const uint32_t* filter_begin, const ss_facet_filter* filters, uint32_t record_size, ss_filter_rows* out) {
  *out = ss_filter_rows();
  if (!filter_begin) return SS_EINVAL;
  for (uint32_t i = 0; i < nq; i++) {
    if (filter_begin[i + 1] < filter_begin[i] || filter_begin[i + 1] - filter_begin[i] > SS_MAX_FACET_FILTERS) return SS_EINVAL;
    if (filter_begin[i + 1] > filter_begin[i] && !filters) return SS_EINVAL;
  }
  out->row_of.assign(nq, SS_ROW_SLOW);
  out->row_begin.push_back(0);
  std::vector<uint32_t> first;  // the first query of every row
  for (uint32_t i = 0; i < nq; i++) {
    const uint32_t n = filter_begin[i + 1] - filter_begin[i];
    const ss_facet_filter* fi = n ? filters + filter_begin[i] : nullptr;
    bool slow = false;
    ss_facet_filter done[SS_MAX_FACET_FILTERS];
    for (uint32_t j = 0; j < n; j++) {
      const int rc = ssi_filter_prepare(fi[j], record_size, &done[j]);
      if (rc != SS_OK) return rc;
      slow |= ssi_filter_is_extern(fi[j]);
    }
    if (slow) { out->n_slow++; continue; }
    uint32_t r = 0;
    for (; r < out->n_rows; r++) {
      const uint32_t o = first[r];
      if (filter_begin[o + 1] - filter_begin[o] == n && (n == 0 || memcmp(filters + filter_begin[o], fi, (size_t)n * sizeof(ss_facet_filter)) == 0)) break;
    }
    if (r == out->n_rows) {
      first.push_back(i);
      out->prepared.insert(out->prepared.end(), done, done + n);
      out->row_begin.push_back((uint32_t)out->prepared.size());
      out->n_rows++;
    }
    out->row_of[i] = r;
  }
  return SS_OK;
}
