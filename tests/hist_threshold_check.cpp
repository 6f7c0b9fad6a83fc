// Stand-alone check of the score histogram's bucket rule (seekstorm_amd/csrc/bm25_hist.h) on the CPU: plain host build, own main.
// For a range of (lo, hi) pairs: bucket() is monotone in the score, edge(bucket(s)) <= s at every bucket edge +- 1 ulp and at random
// scores, scores >= hi land in no bucket below hi's own (the last one once clamped), scores < lo are not counted, and shift is the smallest one that fits.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../seekstorm_amd/csrc/bm25_hist.h"

static uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float float_of(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static long check_pair(float lo, float hi) {
  const uint32_t lo_bits = bits_of(lo), hi_bits = bits_of(hi);
  const uint32_t shift = bm_hist_shift(lo_bits, hi_bits);
  long n = 0;
  CHECK(((hi_bits - lo_bits) >> shift) < BM_HIST_B, "lo %g hi %g shift %u", lo, hi, shift);
  CHECK(shift == 0u || ((hi_bits - lo_bits) >> (shift - 1u)) >= BM_HIST_B, "lo %g hi %g: shift %u is not the smallest", lo, hi, shift);
  auto one = [&](uint32_t s) {
    n++;
    const uint32_t b = bm_hist_bucket(s, lo_bits, shift);
    if (s < lo_bits) { CHECK(b == BM_HIST_NONE, "score below lo counted: lo %g s %g bucket %u", lo, float_of(s), b); return; }
    CHECK(b < BM_HIST_B, "lo %g hi %g s %g bucket %u", lo, hi, float_of(s), b);
    if (b >= BM_HIST_B) return;
    const uint32_t e = bm_hist_edge(b, lo_bits, shift);
    CHECK(e <= s && float_of(e) <= float_of(s), "edge above the score: lo %g hi %g s %g (%08x) bucket %u edge %08x", lo, hi, float_of(s), s, b, e);
    CHECK(e >= lo_bits, "edge below lo: lo %g bucket %u", lo, b);
    if (s >= hi_bits) CHECK(b >= ((hi_bits - lo_bits) >> shift), "a score >= hi below hi's bucket: lo %g hi %g s %g bucket %u", lo, hi, float_of(s), b);
    if (b + 1u < BM_HIST_B) CHECK(s < bm_hist_edge(b + 1u, lo_bits, shift), "score past the next edge: s %08x bucket %u", s, b);
  };
  // every bucket edge +- 1 ulp, and lo / hi themselves +- 1 ulp
  for (uint32_t b = 0; b < BM_HIST_B; b++) {
    const uint64_t e = (uint64_t)lo_bits + ((uint64_t)b << shift);
    if (e + 1u >= 0x7F800000ull) break;  // (past the finite floats: no score is there)
    for (int d = -1; d <= 1; d++) one((uint32_t)((int64_t)e + d));
  }
  for (int d = -1; d <= 1; d++) { one((uint32_t)((int64_t)hi_bits + d)); one((uint32_t)((int64_t)lo_bits + d)); }
  // monotone: a sweep of ascending scores from below lo to above hi never steps down (uncounted scores come first)
  const uint32_t a0 = lo_bits > 1000u ? lo_bits - 1000u : 1u;
  const uint64_t a1w = (uint64_t)hi_bits + (hi_bits - lo_bits) / 4u + 1000u;
  const uint32_t a1 = a1w < 0x7F7FFFFFull ? (uint32_t)a1w : 0x7F7FFFFFu;  // (finite positive floats only: no score is anything else)
  const uint32_t step = (a1 - a0) / 4096u + 1u;
  int64_t prev = -1;
  for (uint64_t s = a0; s <= a1 && s < 0x7F800000ull; s += step) {
    one((uint32_t)s);
    const uint32_t b = bm_hist_bucket((uint32_t)s, lo_bits, shift);
    const int64_t cur = b == BM_HIST_NONE ? -1 : (int64_t)b;
    CHECK(cur >= prev, "bucket not monotone: lo %g hi %g s %08x bucket %lld after %lld", lo, hi, (uint32_t)s, (long long)cur, (long long)prev);
    prev = cur;
  }
  // scores at and above hi: the last bucket a score of this query can be in -- and B - 1 once the clamp is reached
  CHECK(bm_hist_bucket(0x7F7FFFFFu, lo_bits, shift) == BM_HIST_B - 1u, "FLT_MAX: lo %g hi %g", lo, hi);
  CHECK(bm_hist_bucket(hi_bits, lo_bits, shift) == ((hi_bits - lo_bits) >> shift), "hi itself: lo %g hi %g", lo, hi);
  if (((uint64_t)(BM_HIST_B - 1u) << shift) + lo_bits < 0x7F800000ull)
    CHECK(bm_hist_bucket(lo_bits + ((BM_HIST_B - 1u) << shift), lo_bits, shift) == BM_HIST_B - 1u, "the last edge: lo %g hi %g", lo, hi);
  // random scores across and around the range
  for (int i = 0; i < 4000; i++) {
    const uint32_t span = a1 - a0 + 1u;
    one(a0 + (uint32_t)(rnd() % span));
  }
  for (int i = 0; i < 200; i++) one((uint32_t)(rnd() % 0x7F800000ull));  // any positive finite float
  return n;
}

int main() {
  long n = 0, pairs = 0;
  auto pair = [&](float lo, float hi) { n += check_pair(lo, hi); pairs++; };
  const float his[] = {0.37f, 1.0f, 7.25f, 19.999f, 31.5f, 1.0e-3f, 3.0e4f};
  for (float hi : his) {
    pair(hi, hi);                                  // lo = hi
    pair(float_of(bits_of(hi) - 1u), hi);          // lo one ulp below hi
    pair(float_of(bits_of(hi) - 63u), hi);         // the widest range with shift 0
    pair(float_of(bits_of(hi) - 64u), hi);         // the narrowest with shift 1
    pair(hi * BM_HIST_SEEDLESS_LO, hi);            // a seedless range
    pair(hi * 0.6f, hi);                           // lo in the binade below hi's (or in hi's own)
    pair(hi * 0.93f, hi);
    pair(hi * 0.51f, hi * 1.02f);                  // hi in the next binade
    pair(hi * 1.0e-3f, hi);                        // ten binades
  }
  pair(float_of(0x3F7FFFFFu), 1.0f);               // lo and hi on either side of a binade's edge
  pair(1.17549435e-38f, 3.0e38f);                  // the whole range of normal floats
  for (int i = 0; i < 200; i++) {                  // random pairs
    const uint32_t a = 0x30000000u + (uint32_t)(rnd() % 0x20000000u), d = (uint32_t)(rnd() % (1u << (rnd() % 27u)));
    pair(float_of(a), float_of(a + d));
  }
  if (fails) { printf("hist_threshold FAILED: %d checks\n", fails); return 1; }
  printf("hist_threshold ok: %ld pairs, %ld scores\n", pairs, n);
  return 0;
}
