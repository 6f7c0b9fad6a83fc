// Stand-alone check of the host pass over one committed level of a multi-field SPARSE TIER (seekstorm_amd/csrc/mf_sparse_level.h), built
// with -fsanitize=address,undefined by tests/test_mf_sparse_level_cpu.py.  Every input is a heap block of exactly the size the caller
// owns, so a read past an end is the sanitizer's to report; every output is compared with a slow reference written from the header's
// comment.
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <vector>

#include "../seekstorm_amd/csrc/mf_sparse_level.h"

static uint32_t rnd_state = 88172645u;
static uint32_t rnd() { return rnd_state = rnd_state * 1664525u + 1013904223u; }

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

struct Level {
  uint32_t level = 0, n_docs = 0, n_fields = 0, n_lists = 0;
  uint64_t off0 = 0;  // offs need not start at 0: the arrays carry that many unused entries in front
  std::vector<uint64_t> offs;
  std::vector<uint32_t> docs;
  std::vector<uint8_t> fields;
  std::vector<uint16_t> tfs, npos, positions;
  bool use_npos = false;
  int run(mf_sparse_level_host* out, bool with_pos = true) const {
    static const uint16_t none = 0;  // (an empty pool is still "with positions": the pointer says which)
    return mf_sparse_level_prepare(level, n_docs, n_fields, n_lists, offs.data(), docs.data(), fields.data(), tfs.data(),
                                   use_npos ? npos.data() : nullptr, with_pos ? (positions.empty() ? &none : positions.data()) : nullptr,
                                   positions.size(), out);
  }
};

// per_list[i] = docs of the list (sorted, distinct, relative to the level).  which: 0 = the doc's own field d % n_fields and now and then
// another, 1 = every field, 2 = field 1 only, 3 = all fields on even docs and one field on odd ones
static Level make(uint32_t level, uint32_t n_docs, uint32_t n_fields, const std::vector<std::vector<uint32_t>>& per_list, int which, bool use_npos,
                  uint64_t off0, bool no_positions = false) {
  Level L;
  L.level = level; L.n_docs = n_docs; L.n_fields = n_fields; L.n_lists = (uint32_t)per_list.size(); L.off0 = off0; L.use_npos = use_npos;
  L.docs.assign(off0, 0xFFFFFFFFu); L.fields.assign(off0, 0xFF); L.tfs.assign(off0, 0); L.npos.assign(off0, 0xFFFF);
  L.offs.push_back(off0);
  for (const auto& dd : per_list) {
    for (uint32_t d : dd)
      for (uint32_t f = 0; f < n_fields; f++) {
        const bool in = which == 1 || (which == 2 && f == 1) || (which == 0 && (f == d % n_fields || rnd() % 3u == 0u)) ||
                        (which == 3 && ((d & 1u) == 0u || f == d % n_fields));
        if (!in) continue;
        const uint16_t tf = (uint16_t)(1u + rnd() % 5u);
        const uint16_t np = no_positions ? 0 : use_npos ? (uint16_t)(rnd() % 4u) : tf;  // (an n-gram key's component may carry 0 positions)
        L.docs.push_back(level * 65536u + d); L.fields.push_back((uint8_t)f); L.tfs.push_back(tf); L.npos.push_back(np);
        uint16_t p = (uint16_t)(rnd() % 100u);
        for (uint16_t x = 0; x < np; x++) { L.positions.push_back(p); p = (uint16_t)(p + 1u + rnd() % 50u); }
      }
    L.offs.push_back(L.docs.size());
  }
  return L;
}

static void verify(const Level& L, bool with_pos) {
  mf_sparse_level_host H;
  CHECK(L.run(&H, with_pos) == MF_OK);
  const size_t F = L.n_fields;
  CHECK(H.n_lists == L.n_lists && H.n_fields == L.n_fields && H.with_pos == with_pos);
  CHECK(H.moff.size() == (size_t)L.n_lists + 1 && H.moff[0] == 0 && H.mtf.size() == H.mdoc.size() * F && H.moff.back() == H.mdoc.size());
  if (failures) return;
  uint64_t pos_at = 0;
  for (uint32_t i = 0; i < L.n_lists; i++) {
    std::map<uint32_t, std::vector<uint64_t>> by_doc;  // the naive construction: the list's entries grouped by doc
    for (uint64_t j = L.offs[i]; j < L.offs[i + 1]; j++) by_doc[L.docs[j]].push_back(j);
    const uint64_t ma = H.moff[i], mb = H.moff[i + 1];
    CHECK(mb - ma == by_doc.size());
    if (with_pos) CHECK(H.lpos[i] == pos_at);
    uint64_t m = ma, rel = 0;
    for (const auto& kv : by_doc) {
      if (m >= mb) break;
      CHECK(H.mdoc[m] == kv.first && (m == ma || H.mdoc[m] > H.mdoc[m - 1]));
      std::vector<uint16_t> want(F, 0);
      uint32_t cnt = 0;
      for (uint64_t j : kv.second) { want[L.fields[j]] = L.tfs[j]; cnt += L.use_npos ? L.npos[j] : L.tfs[j]; }
      for (size_t f = 0; f < F; f++) CHECK(H.mtf[m * F + f] == want[f]);
      if (with_pos) {
        CHECK(H.mnpos[m] == cnt && H.mpend[m] == rel + cnt);
        uint64_t x = 0;
        for (uint64_t j : kv.second)
          for (uint32_t k = 0; k < (L.use_npos ? L.npos[j] : L.tfs[j]); k++, x++)
            CHECK(H.pos[pos_at + rel + x] == (((uint32_t)L.fields[j] << MF_POS_FIELD_SHIFT) | L.positions[pos_at + rel + x]));
        rel += cnt;
      }
      m++;
    }
    pos_at += rel;
  }
  if (with_pos) CHECK(H.lpos.size() == (size_t)L.n_lists + 1 && H.lpos[L.n_lists] == L.positions.size() && H.pos.size() == L.positions.size());
  else CHECK(H.pos.empty() && H.lpos.empty() && H.mnpos.empty() && H.mpend.empty());
}

static std::vector<uint32_t> some_docs(uint32_t n_docs, uint32_t one_in) {
  std::vector<uint32_t> d;
  for (uint32_t i = 0; i < n_docs; i++)
    if (rnd() % one_in == 0u) d.push_back(i);
  return d;
}

// the first entry with two positions or more (not the last entry), and where its positions start
static bool entry_with_two(const Level& L, uint64_t* j_out, uint64_t* at_out) {
  uint64_t at = 0;
  for (uint64_t j = L.off0; j + 1 < L.docs.size(); j++) {
    const uint32_t c = L.use_npos ? L.npos[j] : L.tfs[j];
    if (c >= 2) { *j_out = j; *at_out = at; return true; }
    at += c;
  }
  return false;
}

int main() {
  mf_sparse_level_host H;
  // shapes: an empty list among full ones, a list of one entry, docs in all fields and in one only, the first and the last doc of the
  // level; npos given and NULL; with and without positions; offs from 0 and not
  for (int use_npos = 0; use_npos < 2; use_npos++)
    for (int which = 0; which < 4; which++)
      for (uint64_t off0 : {(uint64_t)0, (uint64_t)5}) {
        verify(make(3, 5000, 3, {some_docs(5000, 50), {}, some_docs(5000, 400), {0, 4095, 4096, 4999}, {}, {17}}, which, use_npos != 0, off0), true);
        verify(make(0, 5000, 8, {some_docs(5000, 90), {}, {4999}}, which, use_npos != 0, off0), false);
        verify(make(1, 1, 2, {{0}, {}, {0}}, which, use_npos != 0, off0), true);
        verify(make(65535, 1, 2, {{0}}, which, use_npos != 0, off0), true);
      }
  verify(make(2, 65536, 3, {some_docs(65536, 300), {0, 65535}, {}, {65535}, {0}}, 3, false, 0), true);
  verify(make(2, 65536, 3, {some_docs(65536, 200)}, 1, true, 3), true);
  verify(make(1, 3000, 3, {{5}}, 2, false, 0), true);  // a list with ONE entry (field 1 only)
  {  // an empty positions pool: every entry brings 0 positions (npos), the level still carries positions
    const Level e = make(1, 3000, 3, {some_docs(3000, 100), {}, {2999}}, 1, true, 0, /*no_positions=*/true);
    CHECK(e.positions.empty());
    verify(e, true);
  }
  {  // a level without a single entry: null arrays are fine, with and without positions
    const uint64_t offs[3] = {0, 0, 0};
    const uint16_t none = 0;
    CHECK(mf_sparse_level_prepare(0, 10, 3, 2, offs, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &H) == MF_OK && H.mdoc.empty() && !H.with_pos);
    CHECK(mf_sparse_level_prepare(0, 10, 3, 2, offs, nullptr, nullptr, nullptr, nullptr, &none, 0, &H) == MF_OK && H.with_pos && H.lpos.size() == 3);
  }
  // every refusal of the validation
  const Level good = make(1, 3000, 3, {some_docs(3000, 40), some_docs(3000, 90)}, 1, false, 0);
  CHECK(good.run(&H) == MF_OK && good.docs.size() > 12);
  { Level b = good; b.n_lists = 0; CHECK(b.run(&H) == MF_EINVAL); }
  { Level b = good; b.n_docs = 0; CHECK(b.run(&H) == MF_EINVAL); }
  { Level b = good; b.n_docs = 65537; CHECK(b.run(&H) == MF_EINVAL); }
  { Level b = good; b.n_fields = 1; CHECK(b.run(&H) == MF_EINVAL); }
  { Level b = good; b.n_fields = 9; CHECK(b.run(&H) == MF_EINVAL); }
  CHECK(mf_sparse_level_prepare(1, 3000, 3, 2, nullptr, good.docs.data(), good.fields.data(), good.tfs.data(), nullptr, nullptr, 0, &H) == MF_EINVAL);
  CHECK(mf_sparse_level_prepare(1, 3000, 3, 2, good.offs.data(), good.docs.data(), good.fields.data(), good.tfs.data(), nullptr, nullptr, 0, nullptr) == MF_EINVAL);
  CHECK(mf_sparse_level_prepare(1, 3000, 3, 2, good.offs.data(), nullptr, good.fields.data(), good.tfs.data(), nullptr, nullptr, 0, &H) == MF_EINVAL);
  { Level b = good; std::swap(b.offs[1], b.offs[2]); CHECK(b.run(&H) == MF_EINVAL); }                          // offs decreasing
  { Level b = good; b.docs[4] = 65536u - 1u; CHECK(b.run(&H) == MF_EINVAL); }                                   // a doc of the level before
  { Level b = good; b.docs.back() = 65536u + 3000u; CHECK(b.run(&H) == MF_EINVAL); }                            // ... of the docs behind the level
  { Level b = good; b.tfs[7] = 0; CHECK(b.run(&H) == MF_EINVAL); }                                              // tf 0
  { Level b = good; b.fields[2] = 3; CHECK(b.run(&H) == MF_EINVAL); }                                           // field >= n_fields
  { Level b = good; std::swap(b.fields[0], b.fields[1]); CHECK(b.run(&H) == MF_EINVAL); }                       // field not ascending inside a doc
  { Level b = good; b.fields[1] = b.fields[0]; CHECK(b.run(&H) == MF_EINVAL); }                                 // (doc, field) twice
  { Level b = good; std::swap(b.docs[0], b.docs[3]); CHECK(b.run(&H) == MF_EINVAL); }                           // docs not ascending
  { Level b = good; b.positions.pop_back(); CHECK(b.run(&H) == MF_EINVAL); }                                    // position total != n_positions: one too few
  { Level b = good; b.positions.push_back(1); CHECK(b.run(&H) == MF_EINVAL); }                                  // ... one too many
  for (int use_npos = 0; use_npos < 2; use_npos++) {  // positions of an entry not ascending: equal, descending; counts from tf and from npos
    const Level g = use_npos ? make(1, 3000, 3, {some_docs(3000, 40), some_docs(3000, 90)}, 1, true, 0) : good;
    uint64_t j = 0, at = 0;
    CHECK(entry_with_two(g, &j, &at) && j + 1 < g.docs.size() && g.run(&H) == MF_OK);
    if (failures) break;
    const uint32_t c = use_npos ? g.npos[j] : g.tfs[j];
    CHECK(at + c < g.positions.size());
    if (failures) break;
    { Level b = g; b.positions[at + 1] = b.positions[at]; CHECK(b.run(&H) == MF_EINVAL); }
    { Level b = g; std::swap(b.positions[at + c - 2], b.positions[at + c - 1]); CHECK(b.run(&H) == MF_EINVAL); }
    { Level b = g; b.positions[at + c] = 0; CHECK(b.run(&H) == MF_OK); }  // (the next entry starts over: only an entry's own positions ascend)
  }
  {  // 2^32 positions of one list in one level (counted from npos alone: refused before a position is read)
    Level b = make(0, 65536, 2, {some_docs(65536, 1)}, 1, true, 0);
    for (auto& c : b.npos) c = 0xFFFF;
    b.positions.assign(1, 0);
    CHECK((uint64_t)b.npos.size() * 0xFFFFull >= (1ull << 32) && b.run(&H) == MF_ENOTSUP);
  }
  if (failures) { printf("%d checks failed\n", failures); return 1; }
  printf("mf_sparse_level ok\n");
  return 0;
}
