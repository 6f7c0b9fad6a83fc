// Stand-alone check of seekstorm_amd/csrc/filter_rows.h (tests/test_filter_rows_cpu.py builds it with -fsanitize=address,undefined and
// runs it): the grouping of a batch's per-query filter sets into exclusion rows, the filter_begin edges, the refusals a filter meets in
// every entry, the Morton corners of a Point filter, and the marks of the queries that run alone.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../seekstorm_amd/csrc/filter_rows.h"

#define CHECK(x)                                                        \
  do {                                                                  \
    if (!(x)) {                                                         \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); \
      exit(1);                                                          \
    }                                                                   \
  } while (0)

// records of 24 bytes: u32 @0, i16 @4, string16 @6, f32 @8, point @16
static const uint32_t REC = 24;

static ss_facet_filter range(uint32_t off, uint32_t type, uint64_t lo, uint64_t hi) {
  ss_facet_filter f;
  memset(&f, 0, sizeof f);
  f.offset = off; f.type = type; f.lo = lo; f.hi = hi;
  return f;
}
static ss_facet_filter strings(uint32_t off, uint32_t n, uint32_t first) {
  ss_facet_filter f;
  memset(&f, 0, sizeof f);
  f.offset = off; f.type = SS_FACET_STRING16; f.n_values = n;
  for (uint32_t i = 0; i < n && i < 8; i++) f.values[i] = first + i;
  return f;
}
static ss_facet_filter point(uint32_t off, double lat, double lon, double lo, double hi, uint32_t unit) {
  ss_facet_filter f;
  memset(&f, 0, sizeof f);
  f.offset = off; f.type = SS_FACET_POINT; f.n_values = unit;
  uint64_t w;
  memcpy(&w, &lat, 8); f.values[0] = (uint32_t)w; f.values[1] = (uint32_t)(w >> 32);
  memcpy(&w, &lon, 8); f.values[2] = (uint32_t)w; f.values[3] = (uint32_t)(w >> 32);
  memcpy(&f.lo, &lo, 8); memcpy(&f.hi, &hi, 8);
  return f;
}

int main() {
  CHECK(sizeof(ss_facet_filter) == 64);  // (byte-equal sets are compared with memcmp: no padding may hide in the struct)
  ss_filter_rows R;

  // ---- grouping: sets 0 and 3 byte-equal (two filters), 1 its own, 2 and 5 empty, 4 = set 0 with the filters swapped: another row
  {
    const ss_facet_filter a = range(0, SS_FACET_U32, 10, 20), b = range(4, SS_FACET_I16, (uint64_t)-5, 7), c = strings(6, 8, 3);
    const std::vector<ss_facet_filter> f = {a, b, c, a, b, b, a};
    const uint32_t begin[] = {0, 2, 3, 3, 5, 7, 7};
    CHECK(ssi_filter_rows(6, begin, f.data(), REC, &R) == SS_OK);
    CHECK(R.n_rows == 4 && R.n_slow == 0);
    const uint32_t want[] = {0, 1, 2, 0, 3, 2};
    for (int i = 0; i < 6; i++) CHECK(R.row_of[i] == want[i]);
    const uint32_t rb[] = {0, 2, 3, 3, 5};
    CHECK(R.row_begin.size() == 5);
    for (int i = 0; i < 5; i++) CHECK(R.row_begin[i] == rb[i]);
    CHECK(R.prepared.size() == 5 && memcmp(&R.prepared[0], &a, 64) == 0 && memcmp(&R.prepared[2], &c, 64) == 0 && memcmp(&R.prepared[3], &b, 64) == 0);
  }
  // ---- filter_begin edges: one query; all empty (filters may be NULL); the last set empty; more than 64 distinct sets
  {
    const ss_facet_filter a = range(0, SS_FACET_U32, 1, 2);
    const uint32_t one[] = {0, 1};
    CHECK(ssi_filter_rows(1, one, &a, REC, &R) == SS_OK && R.n_rows == 1 && R.row_of[0] == 0 && R.row_begin[1] == 1);
    const uint32_t none[] = {0, 0, 0, 0};
    CHECK(ssi_filter_rows(3, none, nullptr, REC, &R) == SS_OK && R.n_rows == 1 && R.prepared.empty());
    for (int i = 0; i < 3; i++) CHECK(R.row_of[i] == 0);
    const uint32_t last_empty[] = {0, 1, 1};
    CHECK(ssi_filter_rows(2, last_empty, &a, REC, &R) == SS_OK && R.n_rows == 2 && R.row_of[0] == 0 && R.row_of[1] == 1 && R.row_begin[2] == 1);
    CHECK(ssi_filter_rows(0, none, nullptr, REC, &R) == SS_OK && R.n_rows == 0 && R.row_of.empty());
    // a window into a longer array: the offsets are absolute
    const ss_facet_filter two[] = {range(0, SS_FACET_U32, 1, 2), range(0, SS_FACET_U32, 3, 4)};
    const uint32_t window[] = {1, 2, 2};
    CHECK(ssi_filter_rows(2, window, two, REC, &R) == SS_OK && R.n_rows == 2 && memcmp(&R.prepared[0], &two[1], 64) == 0);
  }
  // ---- refusals, all SS_EINVAL and all before a row is formed
  {
    const ss_facet_filter ok = range(0, SS_FACET_U32, 1, 2);
    const uint32_t one[] = {0, 1};
    CHECK(ssi_filter_rows(1, nullptr, &ok, REC, &R) == SS_EINVAL);
    const uint32_t down[] = {0, 2, 1};
    const ss_facet_filter three[] = {ok, ok, ok};
    CHECK(ssi_filter_rows(2, down, three, REC, &R) == SS_EINVAL);  // not ascending
    CHECK(ssi_filter_rows(1, one, nullptr, REC, &R) == SS_EINVAL);   // a set without an array
    std::vector<ss_facet_filter> nine(9, ok);
    const uint32_t nine_b[] = {0, 9};
    CHECK(ssi_filter_rows(1, nine_b, nine.data(), REC, &R) == SS_EINVAL);  // more than SS_MAX_FACET_FILTERS in a set
    ss_facet_filter f = range(21, SS_FACET_U32, 0, 1);  // a field beyond the record: 21 + 4 > 24
    CHECK(ssi_filter_rows(1, one, &f, REC, &R) == SS_EINVAL);
    f = range(20, SS_FACET_U32, 0, 1);
    CHECK(ssi_filter_rows(1, one, &f, REC, &R) == SS_OK);
    f = range(17, SS_FACET_POINT, 0, 1);
    CHECK(ssi_filter_rows(1, one, &f, REC, &R) == SS_EINVAL);
    f = range(0, SS_FACET_POINT + 1, 0, 1);
    CHECK(ssi_filter_rows(1, one, &f, REC, &R) == SS_EINVAL);
    f = strings(6, 9, 0);  // nine inline ids
    CHECK(ssi_filter_rows(1, one, &f, REC, &R) == SS_EINVAL);
    f = strings(6, 8, 0);
    CHECK(ssi_filter_rows(1, one, &f, REC, &R) == SS_OK);
    f = point(16, 48.0, 11.0, 0.0, 50.0, SS_POINT_MILES + 1);  // a bad unit
    CHECK(ssi_filter_rows(1, one, &f, REC, &R) == SS_EINVAL);
    f = strings(6, SS_FACET_IDS_EXTERN, 0);  // an id array that is missing
    f.lo = 0; f.hi = 3;
    CHECK(ssi_filter_rows(1, one, &f, REC, &R) == SS_EINVAL);
    // ssi_filter_prepare alone: what ssi_facet_build calls
    ss_facet_filter out;
    CHECK(ssi_filter_prepare(range(23, SS_FACET_U8, 0, 1), REC, &out) == SS_OK && ssi_filter_prepare(range(24, SS_FACET_U8, 0, 1), REC, &out) == SS_EINVAL);
  }
  // ---- a Point filter: the Morton corners of the box around the base in values[4..7], the caller's part untouched; the sort key has none
  {
    const ss_facet_filter p = point(16, 48.137, 11.575, 0.0, 25.0, SS_POINT_KM);
    const uint32_t one[] = {0, 1};
    CHECK(ssi_filter_rows(1, one, &p, REC, &R) == SS_OK && R.n_rows == 1);
    const ss_facet_filter& d = R.prepared[0];
    CHECK(memcmp(&d, &p, offsetof(ss_facet_filter, values) + 16) == 0 && d.reserved == p.reserved);
    const double lat_delta = 25.0 / (kDeg2Rad * kEarthKm), lon_delta = 25.0 / (kDeg2Rad * kEarthKm * cos(kDeg2Rad * 48.137));
    const unsigned long long m0 = morton_encode(48.137 - lat_delta, 11.575 - lon_delta), m1 = morton_encode(48.137 + lat_delta, 11.575 + lon_delta);
    CHECK(d.values[4] == (uint32_t)m0 && d.values[5] == (uint32_t)(m0 >> 32) && d.values[6] == (uint32_t)m1 && d.values[7] == (uint32_t)(m1 >> 32));
    CHECK(m0 < m1 && m0 != 0);
    // lat in the even bits, lon in the odd ones; saturation and NaN as Rust's `as i32`
    CHECK(morton_encode(0.0000001, 0.0) == 1ull && morton_encode(0.0, 0.0000001) == 2ull);
    CHECK(morton_coord(1e9) == 0x7FFFFFFFu && morton_coord(-1e9) == 0x80000000u && morton_coord(NAN) == 0u);
    const ss_facet_filter k = point(16, 48.137, 11.575, 0.0, 25.0, SS_POINT_SORTKEY);
    ss_facet_filter out;
    CHECK(ssi_filter_prepare(k, REC, &out) == SS_OK && memcmp(&out, &k, 64) == 0);
    // byte-equal Point sets share a row
    const ss_facet_filter pp[] = {p, p};
    const uint32_t two[] = {0, 1, 2};
    CHECK(ssi_filter_rows(2, two, pp, REC, &R) == SS_OK && R.n_rows == 1 && R.row_of[1] == 0);
  }
  // ---- the slow-path marks: a set with an SS_FACET_IDS_EXTERN filter (any number of ids) has no row; its neighbours keep theirs
  {
    uint32_t ids[30];
    for (uint32_t i = 0; i < 30; i++) ids[i] = i * 2;
    ss_facet_filter e = strings(6, SS_FACET_IDS_EXTERN, 0);
    e.lo = (uint64_t)(uintptr_t)ids; e.hi = 30;
    const ss_facet_filter a = range(0, SS_FACET_U32, 1, 2);
    const ss_facet_filter f[] = {a, e, a, a, e};
    const uint32_t begin[] = {0, 1, 2, 3, 5};  // {a} {e} {a} {a, e}
    CHECK(ssi_filter_rows(4, begin, f, REC, &R) == SS_OK);
    CHECK(R.n_rows == 1 && R.n_slow == 2 && R.row_of[0] == 0 && R.row_of[1] == SS_ROW_SLOW && R.row_of[2] == 0 && R.row_of[3] == SS_ROW_SLOW);
    CHECK(R.prepared.size() == 1 && ssi_filter_is_extern(e) && !ssi_filter_is_extern(a));
    e.hi = 0; e.lo = 0;  // an empty id set: legal, still the slow path
    const uint32_t one[] = {0, 1};
    CHECK(ssi_filter_rows(1, one, &e, REC, &R) == SS_OK && R.n_slow == 1 && R.n_rows == 0);
    // a bad filter beside an extern one is still refused
    const ss_facet_filter bad[] = {e, range(30, SS_FACET_U8, 0, 1)};
    const uint32_t two[] = {0, 2};
    CHECK(ssi_filter_rows(1, two, bad, REC, &R) == SS_EINVAL);
  }
  // ---- 64 distinct sets and 7 more queries that repeat them: 64 rows
  {
    std::vector<ss_facet_filter> f;
    std::vector<uint32_t> begin = {0};
    for (uint32_t i = 0; i < 71; i++) { f.push_back(range(0, SS_FACET_U32, i % 64, 100)); begin.push_back((uint32_t)f.size()); }
    CHECK(ssi_filter_rows(71, begin.data(), f.data(), REC, &R) == SS_OK && R.n_rows == 64 && R.row_of[70] == 6 && R.row_of[63] == 63);
  }
  printf("filter_rows ok\n");
  return 0;
}
