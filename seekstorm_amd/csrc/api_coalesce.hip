// C ABI, the coalescer: concurrent callers' searches merged into batches (futex group commit), its SS_CO_TRACE report and its stats.
#include <linux/futex.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <cstring>

#include "api_internal.h"

// SS_CO_TRACE: where a coalesced lexical batch spends its time (sums in us; printed when the shard is destroyed)
struct CoTrace { std::atomic<uint64_t> n{0}, stage{0}, enqueue{0}, wait{0}, scatter{0}, linger{0}, wake{0}, members{0}; };
static CoTrace g_co_trace;
// ... and of the VECTOR coalescer, batch by batch (SS_CO_TRACE: what a pass waited for and whom it left behind)
struct CoVecBatch { uint32_t members, left_queued, linger_us, batch_us; uint64_t t_formed_us; };
static std::vector<CoVecBatch> g_co_vec_trace;
static std::vector<uint32_t> g_co_vec_wake_us, g_co_vec_run_us;  // per vector batch: the leader's wake loop, and the batch itself (stage .. answers scattered)
static std::mutex g_co_vec_trace_mu;
static const bool g_co_trace_on = getenv("SS_CO_TRACE") != nullptr;

bool ssi_co_trace_on() { return g_co_trace_on; }
void ssi_co_trace_lane(uint64_t enqueue_ns, uint64_t wait_ns) { g_co_trace.enqueue += enqueue_ns; g_co_trace.linger += wait_ns; }
void ssi_co_trace_report() {
  if (g_co_trace_on && g_co_trace.n.load()) {
    const double n = (double)g_co_trace.n.load() * 1000.0;  // ns -> us per batch
    fprintf(stderr, "[co] %llu lexical batches: stage %.1f us, search call %.1f us (enqueue %.1f + device wait %.1f), scatter %.1f us, waking %.1f members %.1f us per batch\n",
            (unsigned long long)g_co_trace.n.load(), g_co_trace.stage.load() / n, g_co_trace.wait.load() / n, g_co_trace.enqueue.load() / n,
            g_co_trace.linger.load() / n, g_co_trace.scatter.load() / n, g_co_trace.members.load() / (double)g_co_trace.n.load(), g_co_trace.wake.load() / n);
  }
  if (g_co_trace_on && !g_co_vec_trace.empty()) {
    std::lock_guard<std::mutex> gt(g_co_vec_trace_mu);
    std::vector<uint32_t> m, l, q;
    std::vector<uint64_t> gap;
    for (size_t i = 0; i < g_co_vec_trace.size(); i++) {
      m.push_back(g_co_vec_trace[i].members); l.push_back(g_co_vec_trace[i].linger_us); q.push_back(g_co_vec_trace[i].left_queued);
      if (i) gap.push_back(g_co_vec_trace[i].t_formed_us - g_co_vec_trace[i - 1].t_formed_us);
    }
    auto pc = [](std::vector<uint32_t> v, double p) { std::sort(v.begin(), v.end()); return v[(size_t)(p * (v.size() - 1))]; };
    auto pc64 = [](std::vector<uint64_t> v, double p) { if (v.empty()) return (uint64_t)0; std::sort(v.begin(), v.end()); return v[(size_t)(p * (v.size() - 1))]; };
    fprintf(stderr, "[co-vec] %zu batches: members p1 %u p10 %u p50 %u; linger us p50 %u p90 %u p99 %u; left queued p50 %u p90 %u p99 %u; formed-to-formed us p50 %llu p90 %llu p99 %llu\n",
            m.size(), pc(m, 0.01), pc(m, 0.10), pc(m, 0.50), pc(l, 0.50), pc(l, 0.90), pc(l, 0.99), pc(q, 0.50), pc(q, 0.90), pc(q, 0.99),
            (unsigned long long)pc64(gap, 0.50), (unsigned long long)pc64(gap, 0.90), (unsigned long long)pc64(gap, 0.99));
    if (!g_co_vec_wake_us.empty())
      fprintf(stderr, "[co-vec] wake loop us p50 %u p90 %u p99 %u max %u; batch (formed .. scattered) us p50 %u p99 %u max %u\n", pc(g_co_vec_wake_us, 0.5), pc(g_co_vec_wake_us, 0.9),
              pc(g_co_vec_wake_us, 0.99), pc(g_co_vec_wake_us, 1.0), pc(g_co_vec_run_us, 0.5), pc(g_co_vec_run_us, 0.99), pc(g_co_vec_run_us, 1.0));
    // the batches that make a tail: fewer members than usual, a long pass, or a long gap to the batch before -- with their neighbours
    if (g_co_vec_run_us.size() == g_co_vec_trace.size() && g_co_vec_wake_us.size() == g_co_vec_trace.size() && gap.size() > 8) {
      const uint32_t m50 = pc(m, 0.5), r50 = pc(g_co_vec_run_us, 0.5);
      const uint64_t g50 = pc64(gap, 0.5);
      int shown = 0;
      for (size_t i = 1; i < g_co_vec_trace.size() && shown < 24; i++) {
        const uint64_t g = g_co_vec_trace[i].t_formed_us - g_co_vec_trace[i - 1].t_formed_us;
        if (g_co_vec_trace[i].members * 4u >= m50 * 3u && g_co_vec_run_us[i] * 4u <= r50 * 5u && g * 10u <= g50 * 13u) continue;
        shown++;
        for (size_t j = i - 1; j <= std::min(i + 1, g_co_vec_trace.size() - 1); j++)
          fprintf(stderr, "[co-vec]   %s batch %zu: members %u, left queued %u, linger %u us, formed-to-scattered %u us, wake loop %u us, since the batch before %llu us\n",
                  j == i ? "*" : " ", j, g_co_vec_trace[j].members, g_co_vec_trace[j].left_queued, g_co_vec_trace[j].linger_us, g_co_vec_run_us[j], g_co_vec_wake_us[j],
                  (unsigned long long)(j ? g_co_vec_trace[j].t_formed_us - g_co_vec_trace[j - 1].t_formed_us : 0));
      }
    }
    g_co_vec_wake_us.clear(); g_co_vec_run_us.clear();
    g_co_vec_trace.clear();
  }
}

extern "C" {

// ------------------------------------------------------------------ coalescing of concurrent callers (group commit)
namespace {
inline void co_futex_wait(std::atomic<uint32_t>* a, uint32_t expect) { (void)syscall(SYS_futex, (uint32_t*)a, FUTEX_WAIT_PRIVATE, expect, nullptr, nullptr, 0); }
inline void co_futex_wake(std::atomic<uint32_t>* a) { (void)syscall(SYS_futex, (uint32_t*)a, FUTEX_WAKE_PRIVATE, 1, nullptr, nullptr, 0); }
// set a request's state (1 = done, 3 = lead) and wake its thread if it went to sleep
inline void co_signal(ss_co_req* r, uint32_t st) {
  const uint32_t old = r->state.exchange(st, std::memory_order_acq_rel);
  if (old & 4u) co_futex_wake(&r->state);
}
// wait until the state leaves "pending": a SHORT spin, then the futex.  (Spinning for about a batch's duration -- a sleeping
// follower costs its leader a system call, ~1.5 us each -- was measured and is wrong for a library: 64 spinning callers ran the
// process into its CPU quota, 185 K -> 47 K q/s with a p99 of 73 ms, the CFS throttling period; gpurun_out/conc_linger2.log)
inline void co_cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
  __builtin_ia32_pause();
#elif defined(__aarch64__)
  asm volatile("yield");
#endif
}
inline uint32_t co_wait(ss_co_req* r, uint32_t spin_us) {
  const auto until = std::chrono::steady_clock::now() + std::chrono::microseconds(spin_us);
  for (;;) {
    for (int i = 0; i < 64; i++) {
      const uint32_t v = r->state.load(std::memory_order_acquire);
      if (v != 0u) return v;
      co_cpu_relax();
    }
    if (std::chrono::steady_clock::now() >= until) break;
  }
  for (;;) {
    uint32_t v = 0u;
    if (r->state.compare_exchange_strong(v, 4u, std::memory_order_acq_rel)) v = 4u;
    if (v != 4u) return v;  // done / lead arrived before (or instead of) the sleep
    co_futex_wait(&r->state, 4u);
    v = r->state.load(std::memory_order_acquire);
    if (v != 4u) return v;
  }
}
// requests that can share a batch.  k may differ: the batch runs at the largest k and every member keeps its own prefix -- the
// result order is total (score descending, then doc id ascending), so the top-k' of a query is the head of its top-k.
// Only requests of one k CLASS merge (<= 64, <= 128, <= 256, more -- the kernels' top-k register budgets): a caller with a large k
// must not push the others off the pruned / 16-bit kernels, which serve k <= 128 / k <= 64.
inline uint32_t co_k_class(uint32_t k) { return k <= 64u ? 0u : k <= 128u ? 1u : k <= 256u ? 2u : 3u; }
inline bool co_compatible(const ss_co_req* a, const ss_co_req* b) {
  return (a->k == 0) == (b->k == 0) && co_k_class(a->k) == co_k_class(b->k) && a->rt == b->rt && a->elem == b->elem && a->thr == b->thr &&
         (a->qscale != nullptr) == (b->qscale != nullptr);
}

int co_run_lexical_one(ss_shard* s, ss_co_req* r) {
  return ssi_bm25_search_direct(s, r->nq, (const ss_bm25_query*)r->q, r->k, r->rt, 0, nullptr, r->out_doc, r->out_score, r->out_count, r->out_total);
}
int co_run_vector_one(ss_shard* s, ss_co_req* r) {
  return ssi_vec_search_host(s, r->nq, r->q, r->elem, r->qscale, r->k, r->thr, nullptr, r->out_doc, r->out_score, r->out_count, r->out_total, nullptr);
}

// ---- the FACETED kind (ss_shard_abi::co_fac, api_internal.h): requests of ss_bm25_search_filtered with filters, _facets, _sorted and _sorted_facets.  Two share a
// batch when their specs in ss_bm25_search_each's terms are equal byte for byte -- sorts, facets, bounds, bases of the Point facets, k
// (equal, not a class: the select's pivot is the k-th value) and result type; their FILTERS may differ, that is the point of the batch.
inline bool co_fac_compatible(const ss_co_fac_req* a, const ss_co_fac_req* b) {
  if (a->k != b->k || a->rt != b->rt || a->n_sorts != b->n_sorts || a->n_facets != b->n_facets || a->n_bounds != b->n_bounds) return false;
  if (a->n_sorts && memcmp(a->sorts, b->sorts, (size_t)a->n_sorts * sizeof(ss_result_sort)) != 0) return false;
  if (a->n_facets) {
    const size_t n = (size_t)a->n_facets * 4;
    if (memcmp(a->facet_offset, b->facet_offset, n) != 0 || memcmp(a->facet_type, b->facet_type, n) != 0 || memcmp(a->n_buckets, b->n_buckets, n) != 0) return false;
    if (a->n_bounds && memcmp(a->range_lower_bounds, b->range_lower_bounds, a->n_bounds * 8) != 0) return false;
    for (uint32_t f = 0; f < a->n_facets; f++)
      if (a->facet_type[f] == SS_FACET_POINT && memcmp(&a->bases[f], &b->bases[f], sizeof(ss_facet_point)) != 0) return false;
  }
  return true;
}
// this thread is the coalescer running ONE request through its caller's own entry: that entry must not hand it back
thread_local int t_co_fac_direct = 0;
int co_run_fac_one(ss_shard* s, ss_co_req* r_) {
  ss_co_fac_req* r = static_cast<ss_co_fac_req*>(r_);
  struct Guard { Guard() { t_co_fac_direct++; } ~Guard() { t_co_fac_direct--; } } guard;
  const ss_bm25_query* q = (const ss_bm25_query*)r->q;
  switch (r->kind) {
    case SS_CO_FILTERED:
      return ss_bm25_search_filtered(s, r->nq, q, r->k_own, r->rt_own, r->n_filters, r->filters, r->out_doc, r->out_score, r->out_count, r->out_total);
    case SS_CO_FACETS:
      return ss_bm25_search_facets(s, r->nq, q, r->k_own, r->rt_own, r->n_filters, r->filters, r->n_facets, r->facet_offset, r->facet_type, r->n_buckets,
                                   r->range_lower_bounds, r->bases, r->out_doc, r->out_score, r->out_count, r->out_total, r->out_facet_counts);
    case SS_CO_SORTED:
      return ss_bm25_search_sorted(s, r->nq, q, r->n_sorts, r->sorts, r->k_own, r->n_filters, r->filters, r->out_doc, r->out_score, r->out_count, r->out_total);
    case SS_CO_SORTED_FACETS:
      return ss_bm25_search_sorted_facets(s, r->nq, q, r->n_sorts, r->sorts, r->k_own, r->rt_own, r->n_filters, r->filters, r->n_facets, r->facet_offset,
                                          r->facet_type, r->n_buckets, r->range_lower_bounds, r->bases, r->out_doc, r->out_score, r->out_count, r->out_total,
                                          r->out_facet_counts);
    default: return SS_EINVAL;
  }
}
// one merged batch of <= 64 queries: the members' queries and filters back to back, ONE ss_bm25_search_each -- every query of a member
// under that member's filters --, every member's rows and counters copied to its own arrays
int co_run_fac_batch(ss_shard* s, const std::vector<ss_co_req*>& batch) {
  struct Guard { Guard() { t_co_fac_direct++; } ~Guard() { t_co_fac_direct--; } } guard;  // (nothing in here comes back as a request of its own)
  const ss_co_fac_req* f = static_cast<const ss_co_fac_req*>(batch[0]);
  uint32_t total = 0, total_f = 0;
  for (const ss_co_req* r : batch) { total += r->nq; total_f += r->nq * static_cast<const ss_co_fac_req*>(r)->n_filters; }
  const uint32_t k = f->k;
  std::vector<ss_bm25_query> q(total);
  std::vector<uint32_t> fb(total + 1, 0u), doc((size_t)total * k), cnt(total);
  std::vector<ss_facet_filter> ff;
  ff.reserve(total_f);
  std::vector<float> score((size_t)total * k);
  std::vector<uint64_t> tot(total), fc((size_t)total * f->stride);
  uint32_t at = 0;
  for (const ss_co_req* r_ : batch) {
    const ss_co_fac_req* r = static_cast<const ss_co_fac_req*>(r_);
    memcpy(q.data() + at, r->q, (size_t)r->nq * sizeof(ss_bm25_query));
    for (uint32_t i = 0; i < r->nq; i++) {  // (every query of a request runs under the request's filters)
      ff.insert(ff.end(), r->filters, r->filters + r->n_filters);
      fb[at + i + 1] = (uint32_t)ff.size();
    }
    at += r->nq;
  }
  const int rc = ss_bm25_search_each(s, total, q.data(), f->n_sorts, f->sorts, k, f->rt, fb.data(), ff.data(), f->n_facets, f->facet_offset, f->facet_type,
                                     f->n_buckets, f->range_lower_bounds, f->bases, doc.data(), score.data(), cnt.data(), tot.data(), fc.data());
  if (rc != SS_OK) return rc;
  at = 0;
  for (ss_co_req* r_ : batch) {
    ss_co_fac_req* r = static_cast<ss_co_fac_req*>(r_);
    if (k) {
      memcpy(r->out_doc, doc.data() + (size_t)at * k, (size_t)r->nq * k * sizeof(uint32_t));
      memcpy(r->out_score, score.data() + (size_t)at * k, (size_t)r->nq * k * sizeof(float));
    }
    memcpy(r->out_count, cnt.data() + at, (size_t)r->nq * sizeof(uint32_t));
    memcpy(r->out_total, tot.data() + at, (size_t)r->nq * sizeof(uint64_t));
    if (f->stride) memcpy(r->out_facet_counts, fc.data() + (size_t)at * f->stride, (size_t)r->nq * f->stride * sizeof(uint64_t));
    r->rc = SS_OK;
    at += r->nq;
  }
  return SS_OK;
}

// one merged batch: the members' queries back to back, one search, every member's rows copied to its own buffers
int co_run_batch(ss_shard* s, ss_coalescer& co, bool lexical, const std::vector<ss_co_req*>& batch, uint32_t lane_ix) {
  ss_co_req* f = batch[0];
  ss_coalescer::Lane& ln = co.lane[lane_ix];
  uint32_t total = 0, kk = 0;
  for (ss_co_req* r : batch) { total += r->nq; kk = std::max(kk, r->k); }
  const uint32_t kw = std::max<uint32_t>(kk, 1u);
  const size_t qbytes = lexical ? sizeof(ss_bm25_query) : (size_t)s->dim * f->elem;
  auto al = [](size_t x) { return (x + 63) & ~(size_t)63; };
  const size_t o_q = 0, o_qs = o_q + al((size_t)total * qbytes), o_doc = o_qs + al((size_t)total * 4), o_sc = o_doc + al((size_t)total * kw * 4),
               o_cnt = o_sc + al((size_t)total * kw * 4), o_tot = o_cnt + al((size_t)total * 4), need = o_tot + al((size_t)total * 8);
  SS_HIP(hipSetDevice(s->device));
  if (need > ln.h_pin_cap) {
    if (ln.h_pin) (void)hipHostFree(ln.h_pin);
    ln.h_pin = nullptr; ln.h_pin_cap = 0;
    const size_t cap = std::max<size_t>(need * 2, 1u << 20);
    SS_HIP(hipHostMalloc((void**)&ln.h_pin, cap, hipHostMallocDefault));
    ln.h_pin_cap = cap;
  }
  if (!ln.ev) SS_HIP(hipEventCreateWithFlags(&ln.ev, hipEventDisableTiming));
  char* h_q = ln.h_pin + o_q;
  float* h_qs = (float*)(ln.h_pin + o_qs);
  uint32_t* h_doc = (uint32_t*)(ln.h_pin + o_doc);
  float* h_sc = (float*)(ln.h_pin + o_sc);
  uint32_t* h_cnt = (uint32_t*)(ln.h_pin + o_cnt);
  uint64_t* h_tot = (uint64_t*)(ln.h_pin + o_tot);
  const uint64_t tr0 = g_co_trace_on ? co_now_us() : 0;
  uint32_t at = 0;
  for (ss_co_req* r : batch) {
    memcpy(h_q + (size_t)at * qbytes, r->q, (size_t)r->nq * qbytes);
    if (f->qscale) memcpy(h_qs + at, r->qscale, (size_t)r->nq * sizeof(float));
    at += r->nq;
  }
  const uint64_t tr1 = g_co_trace_on ? co_now_us() : 0;
  int rc;
  static thread_local std::vector<uint32_t> row_of;  // lexical: the row of the lane's buffers that holds query i's answer (ssi_bm25_search_direct_lane)
  if (lexical)
    rc = ssi_bm25_search_direct_lane(s, total, (const ss_bm25_query*)h_q, kk, f->rt, h_doc, h_sc, h_cnt, h_tot, ln.ev, 1u + lane_ix, row_of);
  else
    rc = ssi_vec_search_host_lane(s, total, h_q, f->elem, f->qscale ? h_qs : nullptr, kk, f->thr, h_doc, h_sc, h_cnt, h_tot);
  if (rc != SS_OK) return rc;
  const uint64_t tr2 = g_co_trace_on ? co_now_us() : 0;
  at = 0;
  for (ss_co_req* r : batch) {
    for (uint32_t i = 0; i < r->nq; i++) {
      const size_t row = lexical ? row_of[at + i] : at + i;
      if (r->k) {
        memcpy(r->out_doc + (size_t)i * r->k, h_doc + row * kk, (size_t)r->k * sizeof(uint32_t));
        memcpy(r->out_score + (size_t)i * r->k, h_sc + row * kk, (size_t)r->k * sizeof(float));
      }
      r->out_count[i] = std::min(h_cnt[row], r->k);
      r->out_total[i] = h_tot[row];
    }
    r->rc = SS_OK;
    at += r->nq;
  }
  if (g_co_trace_on && lexical) {
    g_co_trace.n++; g_co_trace.stage += tr1 - tr0; g_co_trace.wait += tr2 - tr1; g_co_trace.scatter += co_now_us() - tr2;
  }
  return SS_OK;
}
}  // namespace

// faceted: `co` is the shard's faceted coalescer and every request in its queue an ss_co_fac_req (lexical in every other respect: the
// linger's rule, a lone caller straight through its own path)
static int co_submit(ss_shard* s, ss_coalescer& co, bool lexical, ss_co_req* me, bool faceted) {
  bool lead;
  {
    std::lock_guard<std::mutex> g(co.mu);
    // a free lane: this thread leads a batch on it at once (nobody in flight: alone, straight away -- a lone caller pays nothing);
    // invariant: a non-empty queue always has a leader at work, or a successor already told to lead
    lead = co.leaders < ((co.n_lanes == 2u && (co.lanes_forced || co.callers_est >= co.lanes_from)) ? 2u : 1u);
    if (lead) {
      co.leaders++;
      me->lane = co.lane[0].busy ? 1u : 0u;
      co.lane[me->lane].busy = true;
    }
    co.queue.push_back(me);
    co.queued_nq.fetch_add(me->nq, std::memory_order_relaxed);
  }
  std::vector<ss_co_req*> batch;
  for (;;) {
    if (!lead) {
      // No spin before the sleep (round 6).  Rounds 3-5 spun 30 us first -- a request that arrives in the last 30 us of the batch in flight
      // saves a futex round trip -- and at T = 64 / 256 callers that was 12.7 / 16 cores busy (290 K .. 350 K calls a second x 30 us), the
      // whole CPU quota of the box at T = 256, throttled in 19 of 20 CFS periods.  Without it: T = 64 283 -> 297 K q/s on 4.2 cores,
      // T = 256 345 -> 393 K on 6.7 (p99 1.5 - 2.5 ms -> 0.85), T = 8 unchanged (profiles/r6_spin.log).
#ifndef CO_SPIN_US
#define CO_SPIN_US 0u
#endif
      const uint32_t v = co_wait(me, CO_SPIN_US);
      if (v == 1u) return me->rc;
      me->state.store(0u, std::memory_order_release);  // v == 3: this thread leads the next batch (its request is the queue's front)
      lead = true;
    }
    // Linger.  With T callers in a loop and one batch in flight, half of them ride in the batch and half wait: batches of T / 2
    // (vectors, T = 64: two 32-query passes of 7.5 ms where one 64-query pass takes 9 ms).  The callers a finished batch has just
    // released are back within microseconds, so the next leader waits for them -- until as many requests are queued as callers
    // seem to be around, at most an eighth of the last batch's duration (<= 1 ms), and only if that batch had company at all: a
    // lone caller is never delayed.  max_wait_us > 0 (ss_shard_set_coalescing) waits that long unconditionally.
    const uint64_t trace_t_lead_ns = g_co_trace_on && !lexical ? co_now_us() : 0;
    {
      uint32_t want, wait_us, hard_us;
      {
        std::lock_guard<std::mutex> g(co.mu);
        // (several lanes: the callers around are shared between the batches in flight)
        want = co.max_wait_us ? co.max_batch : std::min(co.callers_est / std::max(co.leaders, 1u), co.max_batch);
        // (round 5, with the spin still there: an eighth of the last batch's duration, <= 1 ms -- measured at 8 / 4 / 2 / 1 on the C2 image,
        // T = 64: 247 / 245 / 233 / 254 K q/s at batches of 39 / 48 / 62 / 64; profiles/r5_linger.log)
        // VECTOR passes: a quarter, <= 3 ms.  A pass costs the same 9 ms for 44 queries as for 64, so whoever misses it pays a whole pass
        // more -- and a hybrid caller comes back through its lexical half first, which at k = 100 takes 0.5 - 1.5 ms for 64 callers
        // (profiles/r6_co_vec_trace.log: with the 1 ms cap 6 % of the hybrid searches missed their pass, p99 = 2.3 x p50).
        // LEXICAL, round 6 (the followers' spin gone, CPU to spare): up to the WHOLE of the last batch's duration, at most 150 us -- a
        // one-launch batch of top-10 queries takes ~100 us, so the callers it released are all back (one futex wake each, ~1.2 us apiece)
        // and every batch is full: T = 32 195 -> 245 K q/s, T = 64 303 -> 320 - 346 K (p99 280 -> 240 - 255 us), T = 8 p99 160 -> 94 us
        // (profiles/r6_linger_div.log).  The cap keeps a hybrid caller's lexical half (k = 100: 0.4 - 0.8 ms a batch) from lingering its
        // callers past their vector pass (uncapped: hybrid T = 64 p99 21 ms in one of two runs, r6_linger_div_hybrid.log).
        const uint32_t div = lexical ? 1u : 4u, cap = lexical ? 150u : 3000u;
        wait_us = co.max_wait_us ? co.max_wait_us : (co.callers_est > 1 ? std::min<uint32_t>(cap, co.last_batch_us / div) : 0u);
        hard_us = std::max<uint32_t>(wait_us, std::min<uint32_t>(co.last_batch_us, 10000u));  // (last_batch_us is written under co.mu: read here)
      }
      if (wait_us) {
        const auto t_in = std::chrono::steady_clock::now(), until = t_in + std::chrono::microseconds(wait_us);
        const auto hard_until = t_in + std::chrono::microseconds(hard_us);
        // VECTOR passes also leave when the batch is NEARLY full and the arrivals have gone quiet: of 64 callers released together, 63 are
        // back within ~150 us; now and then one is not (the scheduler's doing) -- waiting out the cap for it costs the 63 a quarter of a
        // pass each (their p99: 12 - 14 ms against a p50 of 9.4, profiles/r6_tail_repeat.log), where going without it costs ONE caller a
        // second pass.  (A hybrid caller's lexical halves come back in two or three clumps half a millisecond apart: between clumps the
        // batch is half empty, and the rule does not fire.)
#ifndef CO_VEC_QUIET_US
#define CO_VEC_QUIET_US 700
#endif
        const uint32_t nearly = want - std::max(1u, want / 16u);
        uint32_t have_prev = 0;
        auto t_change = t_in;
        for (;;) {
          uint32_t have = 0;
          have = co.queued_nq.load(std::memory_order_relaxed);
          if (have >= want) break;
          const auto now = std::chrono::steady_clock::now();
          // members of the batch before that its leader has NOT EVEN WOKEN yet are certain to come: the wake loop is 64 system calls one
          // after the other, ~100 us as a rule -- and 6 ms now and then, when the leader loses its CPU in the middle (SS_CO_TRACE:
          // "wake loop us p50 103 p99 572 max 6318").  The three callers it had reached used to lead the next pass without the sixty it
          // had not (members p1 3): those paid a second pass, 19 ms.  Waited for beyond the cap, up to a pass's duration.
          const bool pending = co.waking.load(std::memory_order_relaxed) != 0u;
          if (now >= until && (!pending || now >= hard_until)) break;
          if (have != have_prev) { have_prev = have; t_change = now; }
          if (!lexical && !pending && want >= 16u && have >= nearly && now - t_change >= std::chrono::microseconds(CO_VEC_QUIET_US)) break;  // (longer than a lexical linger + batch: a hybrid caller's last clump)
          for (int i = 0; i < 32; i++) __builtin_ia32_pause();
        }
      }
    }
    const auto batch_t0 = std::chrono::steady_clock::now();
    const uint64_t trace_linger_ns = g_co_trace_on && !lexical ? co_now_us() : 0;
    batch.clear();
    {
      std::lock_guard<std::mutex> g(co.mu);
      uint32_t total = 0;
      // the leader's own request (told to lead as the queue's front, or just arrived -- then another lane's leader may have taken
      // requests ahead of it, never its own); with it every queued request that can share its batch
      ss_co_req* f = me;
      for (auto it = co.queue.begin(); it != co.queue.end(); ++it)
        if (*it == me) { co.queue.erase(it); co.queued_nq.fetch_sub(me->nq, std::memory_order_relaxed); break; }
      batch.push_back(me);  // first, whatever else fits
      total = me->nq;
      for (auto it = co.queue.begin(); it != co.queue.end();) {
        if ((*it)->lane == 0xFFFFFFFFu &&  // (a request that leads a lane itself is not a member of anybody's batch)
            (faceted ? co_fac_compatible(static_cast<const ss_co_fac_req*>(f), static_cast<const ss_co_fac_req*>(*it)) : co_compatible(f, *it)) &&
            total + (*it)->nq <= co.max_batch) {
          total += (*it)->nq;
          batch.push_back(*it);
          co.queued_nq.fetch_sub((*it)->nq, std::memory_order_relaxed);
          it = co.queue.erase(it);
        } else {
          ++it;
        }
      }
      co.batches++;
      co.queries += total;
      if (g_co_trace_on && !lexical) {
        uint32_t left = 0;
        for (ss_co_req* r : co.queue) left += r->nq;
        std::lock_guard<std::mutex> gt(g_co_vec_trace_mu);
        g_co_vec_trace.push_back(CoVecBatch{total, left, (uint32_t)((trace_linger_ns - trace_t_lead_ns) / 1000), 0u, trace_linger_ns / 1000});
      }
    }
    // (a lone VECTOR request takes the batch form too: the lane's pinned staging and the scan's own stream -- its pass must not hold the
    // shard mutex either)
    if (batch.size() == 1 && lexical) {
      batch[0]->rc = faceted ? co_run_fac_one(s, batch[0]) : co_run_lexical_one(s, batch[0]);
    } else if ((faceted ? co_run_fac_batch(s, batch) : co_run_batch(s, co, lexical, batch, me->lane)) != SS_OK) {
      // somebody's request is at fault (or the device is): every member is re-run alone and gets its own verdict
      for (ss_co_req* r : batch) r->rc = faceted ? co_run_fac_one(s, r) : lexical ? co_run_lexical_one(s, r) : co_run_vector_one(s, r);
    }
    ss_co_req* succ = nullptr;
    {
      std::lock_guard<std::mutex> g(co.mu);
      uint32_t members = 0, queued = 0;
      for (ss_co_req* r : batch) members += r->nq;
      for (ss_co_req* r : co.queue) queued += r->nq;
      // Callers around = the most seen at the end of any of the last FOUR batches, and never less than 15/16 of the estimate before.  Callers
      // seen at THIS moment miss those on their way back (a hybrid caller is in its lexical half just now), and one straggler's batch of ONE
      // used to zero the estimate: the next leader then did not linger at all, took the three callers that happened to be there, and sixty
      // paid a second pass (profiles/r6_quiet_ab.log: "members p1 3").  A lone caller is not delayed: after four batches of one the
      // estimate is zero.
      const uint32_t seen = members + queued, floor_ = co.callers_est - std::max(1u, co.callers_est / 16u);
      co.seen_ring[co.seen_at++ & 3u] = seen;
      const uint32_t recent = std::max(std::max(co.seen_ring[0], co.seen_ring[1]), std::max(co.seen_ring[2], co.seen_ring[3]));
      co.callers_est = recent > 1u ? std::max(recent, co.callers_est > 1u ? floor_ : 0u) : 0u;
      co.last_batch_us = (uint32_t)std::min<long long>(1000000, std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - batch_t0).count());
      // hand the lane to the queue's front unless another lane's leader already told it to lead
      for (ss_co_req* r : co.queue)
        if (r->lane == 0xFFFFFFFFu) { succ = r; break; }
      if (succ) succ->lane = me->lane;
      else { co.leaders--; co.lane[me->lane].busy = false; }
    }
    const uint64_t tw0 = g_co_trace_on ? co_now_us() : 0;
    if (succ) co_signal(succ, 3u);  // first: the next batch forms while this one's members are being woken
    // (one futex wake per sleeping member, 1.26 us each.  Waking them faster was built twice and is wrong on a CPU quota: one shared futex
    // with FUTEX_WAKE(all), round 5, and a tree -- the leader wakes every 8th member, who wakes its group --, round 6: the leader's part falls
    // 47 -> 4.4 us per batch, all members run, spin and re-submit at once, and the process is throttled: T = 256 344 K -> 75 K q/s with
    // p99 = 78 ms, the CFS period; T = 64 283 K -> 220 K.  The serial wake is the pacing.  profiles/r6_tree_wake_rejected.log)
    // (re-measured in round 6 WITHOUT the followers' spin, which had been what ran the process into its quota: the tree still loses --
    // T = 64 299 -> 277 K q/s, T = 256 394 -> 100-140 K with 18 - 30 s of SYSTEM time per 2 s: members woken together re-submit together
    // and fight over the queue's mutex.  The serial wake paces that too.  profiles/r6_spin_tree.log)
    bool mine = false;
    co.waking.fetch_add((uint32_t)batch.size(), std::memory_order_relaxed);
    for (ss_co_req* r : batch) {
      if (r == me) mine = true;
      else co_signal(r, 1u);
      co.waking.fetch_sub(1u, std::memory_order_relaxed);
    }
    if (g_co_trace_on && lexical && !faceted && batch.size() > 1) { g_co_trace.wake += co_now_us() - tw0; g_co_trace.members += batch.size() - 1; }
    if (g_co_trace_on && !lexical) {
      std::lock_guard<std::mutex> gt(g_co_vec_trace_mu);
      g_co_vec_wake_us.push_back((uint32_t)((co_now_us() - tw0) / 1000));
      g_co_vec_run_us.push_back((uint32_t)((tw0 - trace_linger_ns) / 1000));
    }
    if (mine) return me->rc;
    lead = false;  // (cannot happen while the leader's request is the front of its own batch; kept for safety)
  }
}

extern "C++" int ssi_co_submit(ss_shard* s, ss_coalescer& co, bool lexical, ss_co_req* me) { return co_submit(s, co, lexical, me, false); }

extern "C++" int ssi_co_fac_try(ss_shard* s, uint32_t kind, uint32_t nq, const ss_bm25_query* queries, uint32_t n_sorts, const ss_result_sort* sorts, uint32_t k,
                                uint32_t rt, uint32_t n_filters, const ss_facet_filter* filters, uint32_t n_facets, const uint32_t* facet_offset,
                                const uint32_t* facet_type, const uint32_t* n_buckets, const uint64_t* range_lower_bounds, const ss_facet_point* bases,
                                uint32_t* out_doc, float* out_score, uint32_t* out_count, uint64_t* out_total, uint64_t* out_facet_counts, bool* submitted) {
  *submitted = false;
  if (!s || t_co_fac_direct || nq == 0 || nq > SS_CO_FACETED_MAX_REQUEST) return SS_OK;
  ss_coalescer* co = &ssi_co_fac(s);
  if (!co->max_batch) return SS_OK;
  // only what a batch can carry as it stands; everything else is its own entry's to answer or refuse
  if (!queries || !out_count || !out_total || rt > SS_RT_TOPKCOUNT || n_sorts > SS_MAX_SORT_FIELDS || (n_sorts && !sorts) || n_filters > SS_MAX_FACET_FILTERS ||
      (n_filters && !filters) || n_facets > SS_MAX_QUERY_FACETS)
    return SS_OK;
  if (rt != SS_RT_COUNT && (k == 0 || k > SS_MAX_K || !out_doc || !out_score)) return SS_OK;
  if (n_facets && (!facet_offset || !facet_type || !n_buckets || !out_facet_counts)) return SS_OK;
  for (uint32_t j = 0; j < n_filters; j++)
    if (filters[j].n_values == SS_FACET_IDS_EXTERN && (filters[j].type == SS_FACET_STRING16 || filters[j].type == SS_FACET_STRING32)) return SS_OK;
  ss_co_fac_req r;
  r.kind = kind; r.k_own = k; r.rt_own = rt;
  r.q = queries; r.nq = nq; r.k = rt == SS_RT_COUNT ? 0u : k; r.rt = rt;
  r.n_sorts = n_sorts; r.sorts = sorts;
  r.n_filters = n_filters; r.filters = filters;
  r.n_facets = n_facets; r.facet_offset = facet_offset; r.facet_type = facet_type; r.n_buckets = n_buckets; r.range_lower_bounds = range_lower_bounds; r.bases = bases;
  for (uint32_t f = 0; f < n_facets; f++) {
    if (facet_type[f] > SS_FACET_POINT || n_buckets[f] == 0 || n_buckets[f] > (1u << 24) || (facet_type[f] == SS_FACET_POINT && !bases)) return SS_OK;
    if (facet_type[f] != SS_FACET_STRING16 && facet_type[f] != SS_FACET_STRING32) r.n_bounds += n_buckets[f];
    r.stride += (size_t)n_buckets[f] + 1;
  }
  if (r.n_bounds && !range_lower_bounds) return SS_OK;
  if (rt == SS_RT_COUNT && n_sorts) return SS_OK;  // (no select, but its sort fields are still checked: by its own entry)
  r.out_doc = out_doc; r.out_score = out_score; r.out_count = out_count; r.out_total = out_total; r.out_facet_counts = out_facet_counts;
  *submitted = true;
  return co_submit(s, *co, true, &r, true);
}

int ss_shard_set_coalescing_faceted(ss_shard* s, uint32_t max_batch, uint32_t max_wait_us) {
  if (!s || max_batch > 64u) return SS_EINVAL;
  ss_coalescer* co = &ssi_co_fac(s);
  std::lock_guard<std::mutex> g(co->mu);
  co->max_batch = max_batch;
  co->max_wait_us = max_wait_us;
  return SS_OK;
}
int ss_shard_coalescing_stats_faceted(ss_shard* s, uint64_t* batches, uint64_t* queries) {
  if (!s) return SS_EINVAL;
  ss_coalescer* co = &ssi_co_fac(s);
  std::lock_guard<std::mutex> g(co->mu);
  if (batches) *batches = co->batches;
  if (queries) *queries = co->queries;
  return SS_OK;
}
int ss_shard_set_coalescing(ss_shard* s, uint32_t max_lexical_batch, uint32_t max_vector_batch, uint32_t max_wait_us) {
  if (!s || max_vector_batch > SS_VEC_BATCH) return SS_EINVAL;
  { std::lock_guard<std::mutex> g(s->co_lex.mu); s->co_lex.max_batch = max_lexical_batch; s->co_lex.max_wait_us = max_wait_us; }
  { std::lock_guard<std::mutex> g(s->co_vec.mu); s->co_vec.max_batch = max_vector_batch; s->co_vec.max_wait_us = max_wait_us; }
  return SS_OK;
}
int ss_bm25_path_stats(ss_shard* s, uint64_t* one_launch_batches) {
  if (!s || !one_launch_batches) return SS_EINVAL;
  ShardLock g(s);
  *one_launch_batches = s->small_launches;
  return SS_OK;
}
int ss_bm25_shape_stats(ss_shard* s, uint64_t* generic_batches) {
  if (!s || !generic_batches) return SS_EINVAL;
  ShardLock g(s);
  *generic_batches = s->gallop_batches;
  return SS_OK;
}
int ss_shard_coalescing_stats(ss_shard* s, uint64_t* lexical_batches, uint64_t* lexical_queries, uint64_t* vector_batches, uint64_t* vector_queries) {
  if (!s) return SS_EINVAL;
  { std::lock_guard<std::mutex> g(s->co_lex.mu); if (lexical_batches) *lexical_batches = s->co_lex.batches; if (lexical_queries) *lexical_queries = s->co_lex.queries; }
  { std::lock_guard<std::mutex> g(s->co_vec.mu); if (vector_batches) *vector_batches = s->co_vec.batches; if (vector_queries) *vector_queries = s->co_vec.queries; }
  return SS_OK;
}

}  // extern "C"
