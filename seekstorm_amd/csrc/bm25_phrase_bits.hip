// Match sets of PHRASE queries, as bitmaps on the device: what facet counts, the sort pivot and result sorts walk (bm25_match.h).
// A phrase is an intersection whose survivors pass the position check (add_result.rs:3586-3684; bm25_phrase.hip, bm25_sparse.hip).
// The intersection of its unique terms is a match set the library already builds -- ssi_bm25_match_bits[_tiered], both tiers, NOT terms
// applied, under the exclusion bitmap in force (ssi_bm25_phrase_stage writes the query's intersection form).  phrase_refine_kernel takes
// that bitmap and clears every doc whose positions do not carry the phrase; it reads only candidates, ranks nothing and needs no
// per-term-count instances.
//
// One wave per (query, 64 groups of 64 docs = one sub-block).  The lanes load the 64 candidate words; a wave whose words are all zero
// ends there (ballot).  The candidates are dealt to the lanes one each, 64 per step, by their rank among the wave's set bits (prefix
// counts + rank select: a first version gave every non-zero word a step of its own with lane l on doc 64 g + l, and at one or two
// candidates per word ran 64 steps of one busy lane each -- 360 us of a 650 us call).  A lane finds its doc's posting in every unique
// term a place of the phrase names
// -- a dense term in its only / merged list (dense_find), a sparse term in its list (sp_find) --, keeps where the posting's positions
// lie (pointer + count per term, in LDS: a register array indexed by the running word would live in scratch) and runs the phrase check
// the ranking kernels run: a start offered by the first word's positions, word i by binary search at start + i, SS_PHRASE_SKIP places
// passed over; PT = uint32_t (several indexed fields, merged lists): the start's field tag tested against the query's field filter.
// (One of five copies of the check; tests/test_gpu_phrase_positions.py drives all five over one world of position edges.)
// A failed doc's bit is cleared in the wave's LDS copy of the words.  Global writes: the refined word (a plain store by the lane that
// loaded it) and one atomic add per wave, which takes the cleared docs off the query's count.  Queries of the batch that are no phrases are not touched.
#include <algorithm>

#include "bm25_match.h"
#include "bm25_find.h"
#include "bit_select.h"

namespace {

constexpr int PB_WAVES = 4;
constexpr uint32_t PB_NT = SS_MAX_PHRASE;  // the unique terms a place can name (ssi_bm25_phrase_check refuses a later one)
constexpr uint32_t PB_SKIP = 15u;          // 4-bit code of a place without an entry

struct PbParams {
  const ss_bm25_query* q;  // the batch as the caller gave it (phrase_seq, phrase_len, field filter)
  const uint32_t* post;
  const unsigned long long* term_base;
  const uint32_t* sub_off;
  const uint32_t* pos_off;
  const unsigned long long* pos_base;
  const unsigned long long* sp_base;
  const unsigned long long* sp_post;
  const unsigned long long* sp_pos_end;
  unsigned long long* bits;   // [nq][n_groups]
  unsigned long long* total;  // [nq]
  uint32_t n_sub, n_dense, n_lists, n_groups;
};

template <typename PT>
__global__ void __launch_bounds__(PB_WAVES * 64) phrase_refine_kernel(PbParams P, const PT* __restrict__ pos, const PT* __restrict__ sp_pos) {
  constexpr bool MF = sizeof(PT) == 4;  // several indexed fields: positions carry their field
  __shared__ const PT* s_ptr[PB_WAVES][PB_NT][64];  // the owned doc's positions of every unique term, [term][lane]: each lane its own column
  __shared__ uint32_t s_n[PB_WAVES][PB_NT][64];
  __shared__ unsigned long long s_word[PB_WAVES][64], s_ref[PB_WAVES][64];  // the candidate words as loaded / as refined
  __shared__ uint32_t s_pre[PB_WAVES][64];                                  // candidates before each word
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint32_t qi = blockIdx.y, g0 = (blockIdx.x * PB_WAVES + (uint32_t)w) * 64u;
  const ss_bm25_query* __restrict__ Q = P.q + qi;
  if (bm_q_op(Q->op) != SS_OP_PHRASE || g0 >= P.n_groups) return;
  const uint32_t g = g0 + (uint32_t)lane;
  unsigned long long* __restrict__ bits = P.bits + (size_t)qi * P.n_groups;
  const unsigned long long word = g < P.n_groups ? bits[g] : 0ull;
  if (__ballot(word != 0ull) == 0ull) return;
  const uint32_t nt = min(Q->n_terms, PB_NT), plen = min(Q->phrase_len, (uint32_t)SS_MAX_PHRASE);
  const uint32_t filt = MF ? bm_q_field_filter(Q->op) : 0u, fmask = filt ? filt : 0xFFFFFFFFu;
  // place i of the phrase -> unique term, 4 bits each (uniform per wave); `named`: the terms some place names -- an n-gram key's other
  // component terms are in the intersection but offer no positions to the check
  unsigned long long wpack = 0ull;
  uint32_t named = 0u;
#pragma unroll
  for (int i = 0; i < SS_MAX_PHRASE; i++) {
    const uint32_t sq = Q->phrase_seq[i];
    const uint32_t sl = ((uint32_t)i < plen && sq < nt) ? sq : PB_SKIP;
    wpack |= (unsigned long long)sl << (4 * i);
    if (sl != PB_SKIP) named |= 1u << sl;
  }
  auto wslot = [&](uint32_t i) -> uint32_t { return (uint32_t)(wpack >> (4u * i)) & 15u; };
  const uint32_t w0 = wslot(0u);

  // the wave's candidates, dealt one per lane: match i of the 64 words lies in the word whose exclusive prefix count holds i
  // (binary search over s_pre), at the (i - prefix)-th set bit of it -- a word with one candidate does not cost a step of its own
  const uint32_t cnt = (uint32_t)__popcll(word);
  uint32_t run = cnt;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t v = __shfl_up(run, o);
    if (lane >= o) run += v;
  }
  const uint32_t total = __shfl(run, 63);
  s_pre[w][lane] = run - cnt;
  s_word[w][lane] = word;
  s_ref[w][lane] = word;
  __builtin_amdgcn_wave_barrier();
  for (uint32_t i = (uint32_t)lane; i < total; i += 64u) {
    uint32_t wl = 0u, wh = 64u;  // s_pre[wl] <= i < s_pre[wh] (past the last word: total)
    while (wh - wl > 1u) {
      const uint32_t mid = (wl + wh) >> 1;
      if (s_pre[w][mid] <= i) wl = mid; else wh = mid;
    }
    const uint32_t bit = facet_select64(s_word[w][wl], i - s_pre[w][wl]);
    const uint32_t doc = (g0 + wl) * 64u + bit;
    bool match = false;
    for (uint32_t t = 0; t < nt; t++) {
      const PT* p = pos;
      uint32_t n = 0u;
      if ((named >> t) & 1u) {
        const uint32_t term = Q->term[t];
        if (term >= P.n_dense) {
          const uint32_t j = term - P.n_dense;
          const unsigned long long b1 = P.sp_base[j + 1], x = sp_find(P.sp_post, P.sp_base[j], b1, doc);
          if (x < b1 && (uint32_t)P.sp_post[x] == doc) {
            const unsigned long long st = x ? P.sp_pos_end[x - 1] : 0ull;  // (posting 0 of the tier starts at 0)
            p = sp_pos + st;
            n = (uint32_t)(P.sp_pos_end[x] - st);
          }
        } else {
          const uint32_t row = term * P.n_lists + (P.n_lists - 1u);
          uint32_t slot = 0u;
          if (dense_find(P.post, P.term_base, P.sub_off, P.n_sub, row, doc, &slot)) {
            const uint32_t* po = P.pos_off + P.term_base[row] * 4ull;
            const uint32_t st = slot ? po[slot - 1u] : 0u;
            p = pos + P.pos_base[row] + st;
            n = po[slot] - st;
          }
        }
      }
      s_ptr[w][t][lane] = p;
      s_n[w][t][lane] = n;
    }
    // the phrase: start = a position of word 0, word i must sit at start + i
    if (w0 != PB_SKIP) {
      const PT* b0p = s_ptr[w][w0][lane];
      const uint32_t n0 = s_n[w][w0][lane];
      for (uint32_t j = 0; j < n0 && !match; j++) {
        const uint32_t start = b0p[j];
        bool ok = !MF || ((fmask >> (start >> BM_POS_FIELD_SHIFT)) & 1u);  // the field the phrase would stand in is listed
        for (uint32_t pl = 1; pl < plen && ok; pl++) {
          const uint32_t sl = wslot(pl);
          if (sl == PB_SKIP) continue;  // a place inside an n-gram key: no entry of its own
          const PT* bp = s_ptr[w][sl][lane];
          const uint32_t n = s_n[w][sl][lane], target = start + pl;
          uint32_t lo = 0u, hi = n;
          while (lo < hi) {  // first position >= target (the list is ascending)
            const uint32_t mid = (lo + hi) >> 1;
            if ((uint32_t)bp[mid] < target) lo = mid + 1u; else hi = mid;
          }
          ok = lo < n && (uint32_t)bp[lo] == target;
        }
        match = ok;
      }
    }
    if (!match) atomicAnd(&s_ref[w][wl], ~(1ull << bit));
  }
  __builtin_amdgcn_wave_barrier();
  const unsigned long long refined = s_ref[w][lane];
  if (refined != word) bits[g] = refined;
  uint32_t cleared = (uint32_t)__popcll(word) - (uint32_t)__popcll(refined);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cleared += __shfl_xor(cleared, o);
  if (lane == 0 && cleared) atomicAdd(P.total + qi, 0ull - (unsigned long long)cleared);
}

}  // namespace

int ssi_bm25_phrase_check(const ss_shard* s, const ss_bm25_query& q) {
  const uint32_t L = std::max<uint32_t>(s->bm_n_fields, 1u), n_dense = s->bm_n_terms / L, np = q.n_terms;
  if (np == 0 || np + bm_q_nnot(q.op) > (uint32_t)SS_MAX_QUERY_TERMS) return SS_EINVAL;
  if (q.phrase_len < 2 || q.phrase_len > SS_MAX_PHRASE || q.phrase_seq[0] >= np) return SS_EINVAL;
  for (uint32_t j = 1; j < q.phrase_len; j++)
    if (q.phrase_seq[j] >= np && q.phrase_seq[j] != SS_PHRASE_SKIP) return SS_EINVAL;
  for (uint32_t j = 0; j < q.phrase_len; j++)  // (the search refuses it too: bm25_shape_of)
    if (q.phrase_seq[j] >= SS_MAX_PHRASE && q.phrase_seq[j] != SS_PHRASE_SKIP) return SS_ENOTSUP;
  if (L > 1 && !s->bm_merged) return SS_ENOTSUP;  // phrases of several indexed fields read the merged lists' field-tagged positions
  bool sparse = false, dense = false;
  for (uint32_t t = 0; t < np + bm_q_nnot(q.op); t++) {
    if (q.term[t] >= n_dense + s->sp_n) return SS_EINVAL;
    if (t < np) (q.term[t] >= n_dense ? sparse : dense) = true;
  }
  if (dense && (L > 1 ? !s->d_pos32 : !s->d_pos)) return SS_ENOTSUP;  // the image holds no positions
  if (sparse && (!s->d_sp_pos_end || s->sp_pos_elem != (L > 1 ? 4u : 2u))) return SS_ENOTSUP;  // ... nor does the tier
  if (sparse && np > 6) return SS_ENOTSUP;  // (the sparse phrase kernel's limit: the search refuses it too)
  return SS_OK;
}

void ssi_bm25_phrase_stage(const ss_bm25_query& q, ss_bm25_query* out) {
  *out = q;
  out->op = (uint32_t)SS_OP_INTERSECTION | SS_OP_NOT_TERMS(bm_q_nnot(q.op));  // no field-filter bits: a phrase's filter is a test on positions
  out->phrase_len = 0;
  for (uint32_t i = 0; i < (uint32_t)SS_MAX_PHRASE; i++) out->phrase_seq[i] = 0;
}

int ssi_bm25_phrase_refine(ss_shard* s, const ss_bm25_query* d_q, unsigned long long* d_bits, unsigned long long* d_total, hipStream_t st, uint32_t nq) {
  if (!s->d_post) return SS_ESTATE;
  if (nq == 0 || nq > 64) return SS_EINVAL;
  const bool mf = s->bm_n_fields > 1;
  PbParams P{};
  P.q = d_q;
  P.post = s->d_post;
  P.term_base = (const unsigned long long*)s->d_term_base;
  P.sub_off = s->d_sub_off;
  P.pos_off = s->d_pos_off;
  P.pos_base = (const unsigned long long*)s->d_pos_base;
  P.sp_base = (const unsigned long long*)s->d_sp_base;
  P.sp_post = (const unsigned long long*)s->d_sp_post;
  P.sp_pos_end = (const unsigned long long*)s->d_sp_pos_end;
  P.bits = d_bits;
  P.total = d_total;
  P.n_sub = s->bm_n_sub;
  P.n_dense = s->bm_n_terms / s->bm_n_fields;
  P.n_lists = s->bm_n_fields;
  P.n_groups = s->bm_n_sub * (BM_SUB / 64);
  const dim3 grid((s->bm_n_sub + PB_WAVES - 1) / PB_WAVES, nq);  // one wave per (query, sub-block)
  if (mf) phrase_refine_kernel<uint32_t><<<grid, PB_WAVES * 64, 0, st>>>(P, (const uint32_t*)s->d_pos32, (const uint32_t*)s->d_sp_pos);
  else phrase_refine_kernel<uint16_t><<<grid, PB_WAVES * 64, 0, st>>>(P, (const uint16_t*)s->d_pos, (const uint16_t*)s->d_sp_pos);
  SS_HIP(hipGetLastError());
  return SS_OK;
}
