// C ABI, the vector side: the f32 and i8 images (uploads, level appends, side data, clusters), their host- and device-pointer search
// entries and the coalesced lane's pass.  The kernels live in vec_scan.hip / vec8_scan.hip / vec_ann.hip.
#include <cstring>

#include "api_internal.h"

extern "C" {

// RAII: a search on a stream other than the shard's own runs on that stream's set of scan buffers (swapped into the shard's
// fields while the launches are enqueued -- under s->mu -- and back afterwards; buffers are allocated lazily by the scan code)
struct VecWsBind {
  ss_shard* s;
  ss_vec_ws* w = nullptr;
  VecWsBind(ss_shard* s_, hipStream_t st) : s(s_) {
    if (st == s->stream) return;
    w = &s->vec_ws[st];
    swap();
  }
  ~VecWsBind() { if (w) swap(); }
  void swap() {
    std::swap(s->d_Qf, w->d_Qf);
    std::swap(s->d_vstate, w->d_vstate);
    std::swap(s->d_cand, w->d_cand);
    std::swap(s->d_qaux, w->d_qaux);
  }
};

// The ANN selection state (medoid scores, per-query cluster bitmaps, the tile list, the live counts) is ONE set of buffers per
// shard: a search with an ss_ann_mode queued on another stream than the previous one first waits for that one to finish.
// Caller holds s->mu.  (Searches without a mode touch none of it and stay concurrent across streams.)
struct AnnStateGuard {
  ss_shard* s;
  hipStream_t st;
  bool on;
  AnnStateGuard(ss_shard* s_, hipStream_t st_, const ss_ann_mode* mode) : s(s_), st(st_), on(mode != nullptr) {
    if (on && s->ann_ev_set && s->ann_ev_stream != st) (void)hipStreamWaitEvent(st, s->ann_ev, 0);
  }
  ~AnnStateGuard() {
    if (!on) return;
    if (!s->ann_ev && hipEventCreateWithFlags(&s->ann_ev, hipEventDisableTiming) != hipSuccess) { s->ann_ev = nullptr; s->ann_ev_set = false; return; }
    s->ann_ev_set = hipEventRecord(s->ann_ev, st) == hipSuccess;
    s->ann_ev_stream = st;
  }
};

extern "C++" void ssi_vec_free(ss_shard* s) {
  if (s->vstream) (void)hipStreamSynchronize(s->vstream);  // a coalesced scan still running reads the arrays released below
  for (auto& kv : s->vec_ws) {
    void* wp[] = {kv.second.d_Qf, kv.second.d_vstate, kv.second.d_cand, kv.second.d_qaux};
    for (void* p : wp) if (p) (void)hipFree(p);
  }
  s->vec_ws.clear();
  void* ptrs[] = {s->d_X, s->d_X8, s->d_row_scale, s->d_row_doc, s->d_Qf, s->d_vstate, s->d_cand, s->d_row_field, s->d_row_norm, s->d_row_sq, s->d_qaux, s->d_vec_r2};
  for (void* p : ptrs) if (p) (void)hipFree(p);
  s->d_X = nullptr; s->d_X8 = nullptr; s->d_row_scale = nullptr; s->d_row_doc = nullptr; s->d_Qf = nullptr;
  s->d_row_norm = nullptr; s->d_row_sq = nullptr; s->d_qaux = nullptr; s->d_vec_r2 = nullptr;
  s->d_vstate = nullptr; s->d_cand = nullptr; s->d_row_field = nullptr;
  s->n_rows = s->n_rows_pad = 0; s->dim = s->dim_pad = s->dim_pad8 = 0; s->vec_multi_record = false; s->vec_rows_cap = 0;
  ssi_vec_free_clusters(s);
  if (s->ann_ev) (void)hipEventDestroy(s->ann_ev);
  s->ann_ev = nullptr; s->ann_ev_set = false; s->ann_ev_stream = nullptr;
}

// ------------------------------------------------------------------ vectors
// end of every vector-image build: the Euclidean side data (f32: the two augmented columns; i8: the records' sums of
// squares), then the per-batch workspace
static int vec_finish(ss_shard* s) {
  if (s->vec_similarity == SS_SIM_EUCLIDEAN) {
    int rc = s->d_X ? ssi_vec_augment(s, s->stream) : ssi_vec8_row_sq(s, s->stream);
    if (rc) return rc;
    SS_HIP(hipStreamSynchronize(s->stream));
  }
  return ssi_vec_alloc_ws(s);
}

static int vec_alloc(ss_shard* s, uint64_t n_rows, uint32_t dim) {
  ssi_vec_free(s);
  s->n_rows = n_rows;
  s->dim = dim;
  // Euclidean: the scan computes -|q - x|^2 as the dot product of [x, |x|^2, 1] with [2 q, -1, -|q|^2] -- two more columns
  const uint32_t dim_img = dim + (s->vec_similarity == SS_SIM_EUCLIDEAN ? 2u : 0u);
  s->dim_pad = (dim_img + VS_KC - 1) / VS_KC * VS_KC;
  s->n_rows_pad = (n_rows + VS_TR - 1) / VS_TR * VS_TR;
  const size_t bytes = (size_t)s->n_rows_pad * s->dim_pad * sizeof(float);
  SS_HIP(hipMalloc(&s->d_X, bytes));
  if (s->dim_pad != dim) SS_HIP(hipMemsetAsync(s->d_X, 0, bytes, s->stream));
  else if (s->n_rows_pad != n_rows)
    SS_HIP(hipMemsetAsync(s->d_X + (size_t)n_rows * s->dim_pad, 0, (size_t)(s->n_rows_pad - n_rows) * s->dim_pad * sizeof(float),
                          s->stream));
  return SS_OK;
}

// the row_doc_ids of an upload or a level (n of them; none: a row is its own doc).  *multi: several records per doc (one per field x
// chunk, vector.rs:561-576) -> dedup in the refine kernel.  SS_NO_DOC is no doc id.
static int row_doc_ids_ok(const uint32_t* row_doc_ids, uint64_t n, bool* multi) {
  if (!row_doc_ids) return SS_OK;
  std::vector<uint32_t> tmp(row_doc_ids, row_doc_ids + n);
  std::sort(tmp.begin(), tmp.end());
  *multi = std::adjacent_find(tmp.begin(), tmp.end()) != tmp.end();
  return !tmp.empty() && tmp.back() == SS_NO_DOC ? SS_EINVAL : SS_OK;
}

int ss_vec_upload(ss_shard* s, uint64_t n_rows, uint32_t dim, const float* rows, const uint32_t* row_doc_ids) {
  if (!s || !rows || n_rows == 0 || dim == 0) return SS_EINVAL;
  if (n_rows > 0xFFFFFFFEull) return SS_ENOTSUP;
  bool multi = false;
  SS_TRY(row_doc_ids_ok(row_doc_ids, n_rows, &multi));
  ShardLock g(s);
  SS_HIP(hipSetDevice(s->device));
  SS_HIP(hipStreamSynchronize(s->stream));
  int rc = vec_alloc(s, n_rows, dim);
  if (rc) { ssi_vec_free(s); return rc; }
  SS_HIP(hipMemcpy2DAsync(s->d_X, (size_t)s->dim_pad * sizeof(float), rows, (size_t)dim * sizeof(float),
                          (size_t)dim * sizeof(float), n_rows, hipMemcpyHostToDevice, s->stream));
  s->vec_multi_record = multi;
  if (row_doc_ids) {
    SS_HIP(hipMalloc(&s->d_row_doc, n_rows * sizeof(uint32_t)));
    SS_HIP(hipMemcpyAsync(s->d_row_doc, row_doc_ids, n_rows * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
  }
  SS_HIP(hipStreamSynchronize(s->stream));
  return vec_finish(s);
}

// the i8 image's rows ("i8 (quantised) vectors" below)
static int vec8_alloc(ss_shard* s, uint64_t n_rows, uint32_t dim) {
  ssi_vec_free(s);
  s->n_rows = n_rows;
  s->dim = dim;
  s->dim_pad8 = (dim + 127u) / 128u * 128u;
  if (s->dim_pad8 > 2560u) { ssi_vec_free(s); return SS_ENOTSUP; }  // the 64 queries stay in LDS: 64 x dim_pad8 <= 160 KB
  s->n_rows_pad = (n_rows + VS_TR - 1) / VS_TR * VS_TR;
  const size_t bytes = (size_t)s->n_rows_pad * s->dim_pad8;
  SS_HIP(hipMalloc(&s->d_X8, bytes));
  if (s->dim_pad8 != dim || s->n_rows_pad != n_rows) SS_HIP(hipMemsetAsync(s->d_X8, 0, bytes, s->stream));  // padding is interleaved
  return SS_OK;
}

// vector.bin (writer vector.rs:1066-1094, reader 1279-1298): per level u32 cluster_count, cluster_count x u32 child_count,
// then the records cluster after cluster, each a packed 24-byte VectorHeader (u16 doc_id first, vector.rs:62-73) + dim x f32.
// Shard-local doc id of a record = (level << 16) | doc_id (vector.rs:1448).  The payloads go to HBM straight from the
// file bytes with a strided copy per level; the cluster structure is kept for the ANN modes (vec_ann.hip).
// i8 = Precision::I8 records (dim x i8 after the header); use_scale keeps VectorHeader.scale (f32 at byte 10) per record
// for dot_i8_quantized (ScalarQuantizationI8 with Dot / Euclidean; Cosine scores are the raw integer dot, vector.rs:1331-1333)
static int vec_bin_upload(ss_shard* s, const uint8_t* bytes, uint64_t len, uint32_t dim, bool i8, bool use_scale) {
  if (!s || !bytes || dim == 0) return SS_EINVAL;
  const uint64_t rec = 24u + (uint64_t)dim * (i8 ? 1u : 4u);
  struct Lvl { uint64_t first, n; };
  std::vector<Lvl> levels;
  std::vector<uint32_t> ids, level_clusters, child_counts;
  std::vector<uint16_t> fields;  // VectorHeader.field_id (u32 at byte 2); the reference compares it as u16 (vector.rs:1398)
  std::vector<float> scales, norms;
  uint64_t pos = 0;
  while (pos < len) {
    if (pos + 4 > len) return SS_EINVAL;
    uint32_t clusters;
    memcpy(&clusters, bytes + pos, 4);
    pos += 4;
    if (pos + (uint64_t)clusters * 4u > len) return SS_EINVAL;
    uint64_t n = 0;
    for (uint32_t c = 0; c < clusters; c++) {
      uint32_t child;
      memcpy(&child, bytes + pos + 4ull * c, 4);
      n += child;
      child_counts.push_back(child);
    }
    level_clusters.push_back(clusters);
    pos += (uint64_t)clusters * 4u;
    if (n > (len - pos) / rec || levels.size() >= 65536u) return SS_EINVAL;
    for (uint64_t r = 0; r < n; r++) {
      uint16_t d;
      memcpy(&d, bytes + pos + r * rec, 2);
      ids.push_back((uint32_t)(levels.size() << 16) | d);
      uint32_t fid;
      memcpy(&fid, bytes + pos + r * rec + 2, 4);
      fields.push_back((uint16_t)fid);
      if (use_scale) {
        float sc;
        memcpy(&sc, bytes + pos + r * rec + 10, 4);
        scales.push_back(sc);
        memcpy(&sc, bytes + pos + r * rec + 14, 4);  // VectorHeader.norm: euclidean_i8_quantized
        norms.push_back(sc);
      }
    }
    levels.push_back({pos, n});
    pos += n * rec;
  }
  const uint64_t n_rows = ids.size();
  if (n_rows == 0) return SS_EINVAL;
  if (n_rows > 0xFFFFFFFEull) return SS_ENOTSUP;
  std::vector<uint32_t> tmp(ids);
  std::sort(tmp.begin(), tmp.end());
  const bool multi = std::adjacent_find(tmp.begin(), tmp.end()) != tmp.end();
  ShardLock g(s);
  SS_HIP(hipSetDevice(s->device));
  SS_HIP(hipStreamSynchronize(s->stream));
  int rc = i8 ? vec8_alloc(s, n_rows, dim) : vec_alloc(s, n_rows, dim);
  if (rc) { ssi_vec_free(s); return rc; }
  int8_t* stage = nullptr;  // i8: row-major staging on the device, permuted into fragment order afterwards
  if (i8 && hipMalloc(&stage, (size_t)n_rows * dim) != hipSuccess) { ssi_vec_free(s); return SS_ENOMEM; }
  uint64_t row = 0;
  for (const Lvl& l : levels) {
    if (l.n == 0) continue;
    hipError_t e = i8 ? hipMemcpy2DAsync(stage + row * dim, (size_t)dim, bytes + l.first + 24u, rec, (size_t)dim, l.n,
                                         hipMemcpyHostToDevice, s->stream)
                      : hipMemcpy2DAsync(s->d_X + row * s->dim_pad, (size_t)s->dim_pad * sizeof(float), bytes + l.first + 24u, rec,
                                         (size_t)dim * sizeof(float), l.n, hipMemcpyHostToDevice, s->stream);
    if (e != hipSuccess) { if (stage) (void)hipFree(stage); ssi_vec_free(s); return SS_EDEVICE; }
    row += l.n;
  }
  if (i8) {
    rc = ssi_vec8_permute(s, stage, s->stream);
    (void)hipStreamSynchronize(s->stream);
    (void)hipFree(stage);
    if (rc) { ssi_vec_free(s); return rc; }
    if (use_scale) {
      SS_HIP(hipMalloc(&s->d_row_scale, n_rows * sizeof(float)));
      SS_HIP(hipMemcpyAsync(s->d_row_scale, scales.data(), n_rows * sizeof(float), hipMemcpyHostToDevice, s->stream));
      SS_HIP(hipMalloc(&s->d_row_norm, n_rows * sizeof(float)));
      SS_HIP(hipMemcpyAsync(s->d_row_norm, norms.data(), n_rows * sizeof(float), hipMemcpyHostToDevice, s->stream));
    }
  }
  s->vec_multi_record = multi;
  SS_HIP(hipMalloc(&s->d_row_doc, n_rows * sizeof(uint32_t)));
  SS_HIP(hipMemcpyAsync(s->d_row_doc, ids.data(), n_rows * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
  SS_HIP(hipMalloc(&s->d_row_field, n_rows * sizeof(uint16_t)));
  SS_HIP(hipMemcpyAsync(s->d_row_field, fields.data(), n_rows * sizeof(uint16_t), hipMemcpyHostToDevice, s->stream));
  SS_HIP(hipStreamSynchronize(s->stream));
  rc = ssi_vec_set_clusters(s, (uint32_t)level_clusters.size(), level_clusters.data(), child_counts.data());
  if (rc != SS_OK && rc != SS_ENOTSUP) { ssi_vec_free(s); return rc; }  // ENOTSUP (an empty cluster): AnnMode::All only
  return vec_finish(s);
}

int ss_vec_upload_vector_bin(ss_shard* s, const uint8_t* bytes, uint64_t len, uint32_t dim) {
  return vec_bin_upload(s, bytes, len, dim, false, false);
}

int ss_vec_upload_vector_bin_i8(ss_shard* s, const uint8_t* bytes, uint64_t len, uint32_t dim, int use_record_scale) {
  return vec_bin_upload(s, bytes, len, dim, true, use_record_scale != 0);
}

int ss_vec_synth(ss_shard* s, uint64_t seed, uint64_t n_rows, uint32_t dim) {
  if (!s || n_rows == 0 || dim == 0) return SS_EINVAL;
  if (n_rows > 0xFFFFFFFEull) return SS_ENOTSUP;
  ShardLock g(s);
  SS_HIP(hipSetDevice(s->device));
  SS_HIP(hipStreamSynchronize(s->stream));
  int rc = vec_alloc(s, n_rows, dim);
  if (rc) { ssi_vec_free(s); return rc; }
  SS_TRY(ssi_vec_synth(s, seed, s->stream));
  SS_HIP(hipStreamSynchronize(s->stream));
  return vec_finish(s);
}

int ss_vec_info(ss_shard* s, uint64_t* n_rows, uint32_t* dim) {
  if (!s) return SS_EINVAL;
  if (!s->d_X && !s->d_X8) return SS_ESTATE;
  if (n_rows) *n_rows = s->n_rows;
  if (dim) *dim = s->dim;
  return SS_OK;
}

int ss_vec_read_rows(ss_shard* s, uint64_t r0, uint64_t n, float* out) {
  if (!s || !out) return SS_EINVAL;
  if (!s->d_X) return SS_ESTATE;
  if (r0 + n > s->n_rows) return SS_EINVAL;
  ShardLock g(s);
  SS_HIP(hipSetDevice(s->device));
  SS_HIP(hipStreamSynchronize(s->stream));
  SS_HIP(hipMemcpy2D(out, (size_t)s->dim * sizeof(float), s->d_X + r0 * s->dim_pad, (size_t)s->dim_pad * sizeof(float),
                     (size_t)s->dim * sizeof(float), n, hipMemcpyDeviceToHost));
  return SS_OK;
}

// the search up to the device lists (s->d_out_* on s->stream, counts checked on the host: an overflowed batch is re-run in
// safe mode); caller holds s->mu.  h_count: nq words of host scratch.
extern "C++" int ssi_vec_search_host_lists(ss_shard* s, uint32_t nq, const void* queries, size_t elem, const float* query_scale, uint32_t k,
                                 float thr, const ss_ann_mode* mode, uint32_t* h_count, uint32_t** d_ncl_out,
                                 const float* query_norm, bool want_clusters, size_t out_slot) {
  SS_HIP(hipSetDevice(s->device));
  SS_TRY(ensure_out(s, out_slot + nq, k));  // out_slot: the lists go behind those of `out_slot` earlier queries (hybrid)
  uint32_t* const o_doc = s->d_out_doc + out_slot * k;
  float* const o_score = s->d_out_score + out_slot * k;
  uint32_t* const o_count = s->d_out_count + out_slot;
  uint64_t* const o_total = s->d_out_total + out_slot;
  const size_t qbytes = ((size_t)nq * s->dim * elem + 15) & ~(size_t)15;
  const size_t sbytes = query_scale ? (size_t)nq * sizeof(float) : 0;
  const size_t nbytes = query_norm ? (size_t)nq * sizeof(float) : 0;
  SS_TRY(ensure_qstage(s, qbytes + sbytes + nbytes + (want_clusters ? (size_t)nq * 3 * sizeof(uint32_t) : 0)));  // (three words with SS_ANN_REPORT_OBSERVED)
  float* d_qs = query_scale ? (float*)((char*)s->d_qstage + qbytes) : nullptr;
  float* d_qn = query_norm ? (float*)((char*)s->d_qstage + qbytes + sbytes) : nullptr;
  uint32_t* d_ncl = want_clusters ? (uint32_t*)((char*)s->d_qstage + qbytes + sbytes + nbytes) : nullptr;
  if (d_ncl_out) *d_ncl_out = d_ncl;
  int rc = SS_OK;
  AnnStateGuard ann_guard(s, s->stream, mode);
  for (int attempt = 0; attempt < 2; attempt++) {
    if (hipMemcpyAsync(s->d_qstage, queries, (size_t)nq * s->dim * elem, hipMemcpyHostToDevice, s->stream) != hipSuccess) { rc = SS_EDEVICE; break; }
    if (d_qs && hipMemcpyAsync(d_qs, query_scale, sbytes, hipMemcpyHostToDevice, s->stream) != hipSuccess) { rc = SS_EDEVICE; break; }
    if (d_qn && hipMemcpyAsync(d_qn, query_norm, nbytes, hipMemcpyHostToDevice, s->stream) != hipSuccess) { rc = SS_EDEVICE; break; }
    rc = ssi_vec_search(s, nq, s->d_qstage, d_qs, k, thr, o_doc, o_score, o_count, o_total, s->stream,
                        attempt == 1, mode, d_ncl, d_qn);
    if (rc) break;
    if (hipMemcpyAsync(h_count, o_count, (size_t)nq * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream) != hipSuccess ||
        hipStreamSynchronize(s->stream) != hipSuccess) { rc = SS_EDEVICE; break; }
    bool ovf = false;
    for (uint32_t i = 0; i < nq; i++) ovf |= h_count[i] == 0xFFFFFFFFu;
    if (!ovf) break;
    if (attempt == 1) { rc = SS_EDEVICE; break; }  // cannot overflow in safe mode
  }
  return rc;
}

// A COALESCED vector batch (AnnMode::All; f32 or i8 rows): queries from, and answers into, the lane's PINNED buffers; its own stream and
// staging (ss_common.h vmu / vstream).  The shard mutex is held while the pass is enqueued -- the scan buffers of the stream are bound
// into the shard's fields for that long (VecWsBind) -- and NOT while it runs: 9 ms at 10 M x 768, during which lexical searches of the
// shard (a hybrid caller's first half) used to wait for the mutex, then for the stream.
extern "C++" int ssi_vec_search_host_lane(ss_shard* s, uint32_t nq, const void* queries, size_t elem, const float* query_scale, uint32_t k, float thr,
                                uint32_t* out_doc, float* out_score, uint32_t* out_count, uint64_t* out_total) {
  if (nq == 0) return SS_OK;
  std::lock_guard<std::mutex> gv(s->vmu);
  for (int attempt = 0; attempt < 2; attempt++) {
    {
      std::lock_guard<std::mutex> g(s->mu);  // (a vector pass neither writes nor reads what the lexical lanes' kernels touch: no drain)
      SS_HIP(hipSetDevice(s->device));
      if ((elem == sizeof(float)) ? !s->d_X : !s->d_X8) return SS_ESTATE;
      const size_t qbytes = ((size_t)nq * s->dim * elem + 15) & ~(size_t)15, sbytes = query_scale ? (size_t)nq * sizeof(float) : 0;
      if (qbytes + sbytes > s->vq_cap) {  // (vstream is idle: vmu is ours and the batch before synchronised it)
        if (s->d_vq) (void)hipFree(s->d_vq);
        s->d_vq = nullptr; s->vq_cap = 0;
        SS_HIP(hipMalloc(&s->d_vq, (qbytes + sbytes) * 2));
        s->vq_cap = (qbytes + sbytes) * 2;
      }
      if ((size_t)nq * k > s->vout_cap || nq > s->vq_rows_cap) {
        for (void* p_ : {(void*)s->d_vdoc, (void*)s->d_vscore, (void*)s->d_vcount, (void*)s->d_vtotal}) if (p_) (void)hipFree(p_);
        s->d_vdoc = nullptr; s->d_vscore = nullptr; s->d_vcount = nullptr; s->d_vtotal = nullptr; s->vout_cap = 0; s->vq_rows_cap = 0;
        const size_t rows = std::max<size_t>(nq, SS_VEC_BATCH), cells = std::max<size_t>((size_t)nq * k, (size_t)SS_VEC_BATCH * k);
        SS_HIP(hipMalloc(&s->d_vdoc, cells * sizeof(uint32_t)));
        SS_HIP(hipMalloc(&s->d_vscore, cells * sizeof(float)));
        SS_HIP(hipMalloc(&s->d_vcount, rows * sizeof(uint32_t)));
        SS_HIP(hipMalloc(&s->d_vtotal, rows * sizeof(uint64_t)));
        s->vout_cap = cells; s->vq_rows_cap = rows;
      }
      float* d_qs = query_scale ? (float*)((char*)s->d_vq + qbytes) : nullptr;
      SS_HIP(hipMemcpyAsync(s->d_vq, queries, (size_t)nq * s->dim * elem, hipMemcpyHostToDevice, s->vstream));
      if (d_qs) SS_HIP(hipMemcpyAsync(d_qs, query_scale, sbytes, hipMemcpyHostToDevice, s->vstream));
      {
        VecWsBind bind(s, s->vstream);
        SS_TRY(ssi_vec_search(s, nq, s->d_vq, d_qs, k, thr, s->d_vdoc, s->d_vscore, s->d_vcount, s->d_vtotal, s->vstream, attempt == 1, nullptr, nullptr, nullptr));
      }
      SS_HIP(hipMemcpyAsync(out_count, s->d_vcount, (size_t)nq * sizeof(uint32_t), hipMemcpyDeviceToHost, s->vstream));
      SS_HIP(hipMemcpyAsync(out_doc, s->d_vdoc, (size_t)nq * k * sizeof(uint32_t), hipMemcpyDeviceToHost, s->vstream));
      SS_HIP(hipMemcpyAsync(out_score, s->d_vscore, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToHost, s->vstream));
      SS_HIP(hipMemcpyAsync(out_total, s->d_vtotal, (size_t)nq * sizeof(uint64_t), hipMemcpyDeviceToHost, s->vstream));
      if (!s->vev) SS_HIP(hipEventCreateWithFlags(&s->vev, hipEventDisableTiming | hipEventBlockingSync));
      SS_HIP(hipEventRecord(s->vev, s->vstream));
    }
    // the pass itself: nobody waits for us but this batch's callers.  The leader SLEEPS on a blocking-sync event: hipStreamSynchronize
    // spins, and a thread that spins through 9 ms on a box whose 64 callers share 16 CPUs uses up its time slice and is descheduled just
    // when the pass ends -- its whole batch then comes home a scheduling quantum late (one such batch per second or two was the p99 of the
    // T = 64 vector and hybrid callers: 17.8 / 17.0 ms against a p50 of 9.6 / 10.8, gpurun_out/r6_bench_b.json)
    SS_HIP(hipEventSynchronize(s->vev));
    bool ovf = false;
    for (uint32_t i = 0; i < nq; i++) ovf |= out_count[i] == 0xFFFFFFFFu;
    if (!ovf) return SS_OK;  // (an adversarial row order overflowed the candidate slots: once more in safe mode)
  }
  return SS_EDEVICE;  // cannot overflow in safe mode
}

// host-pointer searches: queries (f32 or i8 rows) and scales are staged in the shard's grow-only buffer, out_clusters
// (observed_cluster_count, ANN modes) rides behind them
extern "C++" int ssi_vec_search_host(ss_shard* s, uint32_t nq, const void* queries, size_t elem, const float* query_scale, uint32_t k,
                           float thr, const ss_ann_mode* mode, uint32_t* out_doc, float* out_score, uint32_t* out_count,
                           uint64_t* out_total, uint32_t* out_clusters, const float* query_norm) {
  if (nq == 0) return SS_OK;
  ShardLock g(s);
  uint32_t* d_ncl = nullptr;
  int rc = ssi_vec_search_host_lists(s, nq, queries, elem, query_scale, k, thr, mode, out_count, &d_ncl, query_norm, out_clusters != nullptr);
  if (rc == SS_OK) {
    if (hipMemcpy(out_doc, s->d_out_doc, (size_t)nq * k * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(out_score, s->d_out_score, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(out_total, s->d_out_total, (size_t)nq * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess ||
        (d_ncl && hipMemcpy(out_clusters, d_ncl, (size_t)nq * ((mode && (mode->flags & SS_ANN_REPORT_OBSERVED)) ? 3 : 1) * sizeof(uint32_t),
                            hipMemcpyDeviceToHost) != hipSuccess))
      rc = SS_EDEVICE;
  }
  return rc;
}

static int vec_search_host_deep(ss_shard* s, uint32_t nq, const void* queries, size_t elem, const float* query_scale, uint32_t k, float thr,
                                const ss_ann_mode* mode, uint32_t* out_doc, float* out_score, uint32_t* out_count, uint64_t* out_total,
                                uint32_t* out_clusters, const float* query_norm) {
  if (nq == 0) return SS_OK;
  ShardLock g(s);
  return ssi_vec_search_deep_locked(s, nq, queries, elem, query_scale, k, thr, mode, out_doc, out_score, out_count, out_total, out_clusters, query_norm);
}

static bool ann_skips_clusters(const ss_ann_mode* m) { return m->n_probe != 0 || m->cluster_threshold_raw > -3.4028234663852886e38f; }
// a mode that neither skips clusters nor filters fields is AnnMode::All
static const ss_ann_mode* ann_effective(const ss_ann_mode* m) {
  return (m && (ann_skips_clusters(m) || m->field_mask || (m->flags & SS_ANN_REPORT_OBSERVED))) ? m : nullptr;
}
static int ann_mode_ok(const ss_shard* s, const ss_ann_mode* mode) {
  if (!mode) return SS_OK;
  if (mode->cluster_threshold_raw != mode->cluster_threshold_raw) return SS_EINVAL;
  if (ann_skips_clusters(mode) && !s->d_row_cluster) return SS_ESTATE;
  if (mode->field_mask && !s->d_row_field) return SS_ESTATE;
  return SS_OK;
}

// euclidean_i8_quantized (scales present) = max(0, n1 + n2 - 2 dot s1 s2) needs BOTH norms: the reference always carries
// VectorHeader.norm / QuantizedVector.norm.  Without them the ranking would silently be that of -max(0, -2 dot s1 s2).
static int vec8_euclid_norms_ok(const ss_shard* s, bool have_qscale, bool have_qnorm) {
  if (s->vec_similarity != SS_SIM_EUCLIDEAN || (!s->d_row_scale && !have_qscale)) return SS_OK;
  if (!s->d_row_norm) return SS_ESTATE;  // ss_vec_set_row_norms
  return have_qnorm ? SS_OK : SS_EINVAL;
}

// The host-pointer entries, all of them: f32 queries on the f32 image (elem = sizeof(float); no scales, no norms) or i8 ones on the i8
// image (elem = 1).  The order of the checks decides which refusal wins where two apply.
static int vec_search_host_entry(ss_shard* s, uint32_t nq, const void* queries, size_t elem, const float* query_scale, const float* query_norm,
                                 uint32_t k, float thr, const ss_ann_mode* mode, uint32_t* out_doc, float* out_score, uint32_t* out_count,
                                 uint64_t* out_total, uint32_t* out_clusters) {
  if (!s || !queries || !out_doc || !out_score || !out_count || !out_total) return SS_EINVAL;
  if (k == 0) return SS_EINVAL;
  if (elem == 1 ? !s->d_X8 : !s->d_X) return SS_ESTATE;
  if (elem == 1) SS_TRY(vec8_euclid_norms_ok(s, query_scale != nullptr, query_norm != nullptr));
  SS_TRY(ann_mode_ok(s, mode));
  mode = ann_effective(mode);
  if (k > SS_MAX_K)  // (a page deeper than SS_MAX_K results: passes under per-query exclusion bitmaps, api_deep.hip)
    return vec_search_host_deep(s, nq, queries, elem, query_scale, k, thr, mode, out_doc, out_score, out_count, out_total, mode ? out_clusters : nullptr, query_norm);
  if (!mode && !query_norm && nq != 0 && nq <= SS_COALESCE_MAX_REQUEST && s->co_vec.max_batch) {  // AnnMode::All from concurrent callers: one pass serves them
    ss_co_req r;
    r.q = queries; r.qscale = query_scale; r.nq = nq; r.k = k; r.elem = (uint32_t)elem; r.thr = thr;
    r.out_doc = out_doc; r.out_score = out_score; r.out_count = out_count; r.out_total = out_total;
    return ssi_co_submit(s, s->co_vec, false, &r);
  }
  return ssi_vec_search_host(s, nq, queries, elem, query_scale, k, thr, mode, out_doc, out_score, out_count, out_total,
                         mode ? out_clusters : nullptr, query_norm);
}
int ss_vec_search_ann(ss_shard* s, uint32_t nq, const float* queries, uint32_t k, float thr, const ss_ann_mode* mode,
                      uint32_t* out_doc, float* out_score, uint32_t* out_count, uint64_t* out_total, uint32_t* out_clusters) {
  return vec_search_host_entry(s, nq, queries, sizeof(float), nullptr, nullptr, k, thr, mode, out_doc, out_score, out_count, out_total, out_clusters);
}
int ss_vec_search(ss_shard* s, uint32_t nq, const float* queries, uint32_t k, float thr, uint32_t* out_doc,
                  float* out_score, uint32_t* out_count, uint64_t* out_total) {
  return vec_search_host_entry(s, nq, queries, sizeof(float), nullptr, nullptr, k, thr, nullptr, out_doc, out_score, out_count, out_total, nullptr);
}

// a DEEP page on a device-pointer vector entry: the passes are steered from the host, so the queries (and their scales / norms) make one
// trip there and the call is synchronous; the page is left in the caller's device arrays, ordered on `st`.  Caller holds the shard lock.
static int vec_search_deep_dev_locked(ss_shard* s, uint32_t nq, const void* d_queries, size_t elem, const float* d_qscale, const float* d_qnorm, uint32_t k, float thr,
                                      const ss_ann_mode* mode, uint32_t* d_out_doc, float* d_out_score, uint32_t* d_out_count, uint64_t* d_out_total,
                                      uint32_t* d_out_clusters, hipStream_t st) {
  if (nq == 0) return SS_OK;
  const uint32_t ocw = (mode && (mode->flags & SS_ANN_REPORT_OBSERVED)) ? 3u : 1u;
  std::vector<char> hq((size_t)nq * s->dim * elem);
  std::vector<float> hs(d_qscale ? nq : 0), hn(d_qnorm ? nq : 0);
  SS_HIP(hipMemcpyAsync(hq.data(), d_queries, hq.size(), hipMemcpyDeviceToHost, st));
  if (d_qscale) SS_HIP(hipMemcpyAsync(hs.data(), d_qscale, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
  if (d_qnorm) SS_HIP(hipMemcpyAsync(hn.data(), d_qnorm, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
  SS_HIP(hipStreamSynchronize(st));
  std::vector<uint32_t> h_doc((size_t)nq * k), h_cnt(nq), h_ncl(d_out_clusters ? (size_t)nq * ocw : 0);
  std::vector<float> h_score((size_t)nq * k);
  std::vector<uint64_t> h_tot(nq);
  SS_TRY(ssi_vec_search_deep_locked(s, nq, hq.data(), elem, d_qscale ? hs.data() : nullptr, k, thr, mode, h_doc.data(), h_score.data(), h_cnt.data(), h_tot.data(),
                                d_out_clusters ? h_ncl.data() : nullptr, d_qnorm ? hn.data() : nullptr));
  SS_HIP(hipMemcpyAsync(d_out_doc, h_doc.data(), h_doc.size() * 4, hipMemcpyHostToDevice, st));
  SS_HIP(hipMemcpyAsync(d_out_score, h_score.data(), h_score.size() * 4, hipMemcpyHostToDevice, st));
  SS_HIP(hipMemcpyAsync(d_out_count, h_cnt.data(), (size_t)nq * 4, hipMemcpyHostToDevice, st));
  SS_HIP(hipMemcpyAsync(d_out_total, h_tot.data(), (size_t)nq * 8, hipMemcpyHostToDevice, st));
  if (d_out_clusters) SS_HIP(hipMemcpyAsync(d_out_clusters, h_ncl.data(), h_ncl.size() * 4, hipMemcpyHostToDevice, st));
  SS_HIP(hipStreamSynchronize(st));
  return SS_OK;
}

// The device-pointer entries, all of them: as vec_search_host_entry, the same checks in the same order.
static int vec_search_dev_entry(ss_shard* s, uint32_t nq, const void* d_queries, size_t elem, const float* d_query_scale, const float* d_query_norm,
                                uint32_t k, float thr, const ss_ann_mode* mode, uint32_t* d_out_doc, float* d_out_score, uint32_t* d_out_count,
                                uint64_t* d_out_total, uint32_t* d_out_clusters, void* stream) {
  if (!s || !d_queries || !d_out_doc || !d_out_score || !d_out_count || !d_out_total) return SS_EINVAL;
  if (k == 0) return SS_EINVAL;
  if (elem == 1 ? !s->d_X8 : !s->d_X) return SS_ESTATE;
  if (elem == 1) SS_TRY(vec8_euclid_norms_ok(s, d_query_scale != nullptr, d_query_norm != nullptr));
  SS_TRY(ann_mode_ok(s, mode));
  mode = ann_effective(mode);
  ShardLock g(s);
  SS_HIP(hipSetDevice(s->device));
  hipStream_t st = stream ? (hipStream_t)stream : s->stream;
  if (k > SS_MAX_K)
    return vec_search_deep_dev_locked(s, nq, d_queries, elem, d_query_scale, d_query_norm, k, thr, mode, d_out_doc, d_out_score, d_out_count, d_out_total,
                                      mode ? d_out_clusters : nullptr, st);
  VecWsBind bind(s, st);
  AnnStateGuard ann_guard(s, st, mode);
  return ssi_vec_search(s, nq, d_queries, d_query_scale, k, thr, d_out_doc, d_out_score, d_out_count, d_out_total, st, false, mode,
                        mode ? d_out_clusters : nullptr, d_query_norm);
}
int ss_vec_search_ann_dev(ss_shard* s, uint32_t nq, const float* d_queries, uint32_t k, float thr, const ss_ann_mode* mode,
                          uint32_t* d_out_doc, float* d_out_score, uint32_t* d_out_count, uint64_t* d_out_total,
                          uint32_t* d_out_clusters, void* stream) {
  return vec_search_dev_entry(s, nq, d_queries, sizeof(float), nullptr, nullptr, k, thr, mode, d_out_doc, d_out_score, d_out_count, d_out_total,
                              d_out_clusters, stream);
}
int ss_vec_search_dev(ss_shard* s, uint32_t nq, const float* d_queries, uint32_t k, float thr, uint32_t* d_out_doc,
                      float* d_out_score, uint32_t* d_out_count, uint64_t* d_out_total, void* stream) {
  return vec_search_dev_entry(s, nq, d_queries, sizeof(float), nullptr, nullptr, k, thr, nullptr, d_out_doc, d_out_score, d_out_count, d_out_total,
                              nullptr, stream);
}

// ---- VectorSimilarity of the image (vector_similarity.rs:118-345): must precede the upload (layout of the f32 image)
int ss_vec_set_similarity(ss_shard* s, int similarity) {
  if (!s || (similarity != SS_SIM_DOT && similarity != SS_SIM_EUCLIDEAN)) return SS_EINVAL;
  ShardLock g(s);
  if ((s->d_X || s->d_X8) && similarity != s->vec_similarity) return SS_ESTATE;
  s->vec_similarity = similarity;
  return SS_OK;
}
int ss_vec_set_row_norms(ss_shard* s, uint64_t n_rows, const float* row_norm) {
  if (!s || !row_norm) return SS_EINVAL;
  ShardLock g(s);
  if (s->vstream) (void)hipStreamSynchronize(s->vstream);  // (a coalesced scan in flight reads what this call replaces; none starts while mu is ours)
  SS_HIP(hipSetDevice(s->device));
  if (!s->d_X8) return SS_ESTATE;
  if (n_rows != s->n_rows) return SS_EINVAL;
  SS_HIP(hipStreamSynchronize(s->stream));
  if (!s->d_row_norm) SS_HIP(hipMalloc(&s->d_row_norm, std::max<uint64_t>(n_rows, s->vec_rows_cap) * sizeof(float)));
  SS_HIP(hipMemcpy(s->d_row_norm, row_norm, n_rows * sizeof(float), hipMemcpyHostToDevice));
  return SS_OK;
}

// ---- cluster structure of the vector image (ANN modes, vec_ann.hip)
int ss_vec_set_clusters(ss_shard* s, uint32_t n_levels, const uint32_t* level_clusters, const uint32_t* child_count) {
  if (!s) return SS_EINVAL;
  ShardLock g(s);
  if (s->vstream) (void)hipStreamSynchronize(s->vstream);  // (a coalesced scan in flight reads what this call replaces; none starts while mu is ours)
  SS_HIP(hipSetDevice(s->device));
  return ssi_vec_set_clusters(s, n_levels, level_clusters, child_count);
}
int ss_vec_set_fields(ss_shard* s, uint64_t n_rows, const uint16_t* row_field) {
  if (!s || !row_field) return SS_EINVAL;
  ShardLock g(s);
  if (s->vstream) (void)hipStreamSynchronize(s->vstream);  // (a coalesced scan in flight reads what this call replaces; none starts while mu is ours)
  SS_HIP(hipSetDevice(s->device));
  if (!s->d_X && !s->d_X8) return SS_ESTATE;
  if (n_rows != s->n_rows) return SS_EINVAL;
  SS_HIP(hipStreamSynchronize(s->stream));
  if (!s->d_row_field) SS_HIP(hipMalloc(&s->d_row_field, std::max<uint64_t>(n_rows, s->vec_rows_cap) * sizeof(uint16_t)));
  SS_HIP(hipMemcpy(s->d_row_field, row_field, n_rows * sizeof(uint16_t), hipMemcpyHostToDevice));
  return SS_OK;
}
int ss_vec_cluster_info(ss_shard* s, uint32_t* n_levels, uint32_t* n_clusters) {
  if (!s) return SS_EINVAL;
  // no lock: two words that only an image (re)build changes, read by every vector search of the host mirrors -- behind s->mu each
  // such read queued up with the batch in flight (64 concurrent callers: mean merged batch 1.3, p99 0.6 s; bench round 3)
  if (n_levels) *n_levels = s->vec_n_levels;
  if (n_clusters) *n_clusters = s->vec_n_clusters;
  return SS_OK;
}

// ------------------------------------------------------------------ i8 (quantised) vectors
// i8 image: rows as the reference stores them for Precision::I8 (quantize_f32_to_i8, vector_similarity.rs:1226-1232, or a
// per-record scale = VectorHeader.scale with ScalarQuantizationI8).  Score = dot_i8 as f32 (vector_similarity.rs:1011-1016)
// or, with scales, dot_i8_quantized = dot as f32 * query_scale * embedding_scale (1754-1758).
int ss_vec_upload_i8(ss_shard* s, uint64_t n_rows, uint32_t dim, const int8_t* rows, const float* row_scale,
                     const uint32_t* row_doc_ids) {
  if (!s || !rows || n_rows == 0 || dim == 0) return SS_EINVAL;
  if (n_rows > 0xFFFFFFFEull) return SS_ENOTSUP;
  bool multi = false;
  SS_TRY(row_doc_ids_ok(row_doc_ids, n_rows, &multi));
  ShardLock g(s);
  SS_HIP(hipSetDevice(s->device));
  SS_HIP(hipStreamSynchronize(s->stream));
  int rc = vec8_alloc(s, n_rows, dim);
  if (rc) { ssi_vec_free(s); return rc; }
  {  // row-major staging on the device, then into fragment order
    int8_t* stage = nullptr;
    SS_HIP(hipMalloc(&stage, (size_t)n_rows * dim));
    if (hipMemcpyAsync(stage, rows, (size_t)n_rows * dim, hipMemcpyHostToDevice, s->stream) != hipSuccess) { (void)hipFree(stage); ssi_vec_free(s); return SS_EDEVICE; }
    rc = ssi_vec8_permute(s, stage, s->stream);
    (void)hipStreamSynchronize(s->stream);
    (void)hipFree(stage);
    if (rc) { ssi_vec_free(s); return rc; }
  }
  s->vec_multi_record = multi;
  if (row_scale) {
    SS_HIP(hipMalloc(&s->d_row_scale, n_rows * sizeof(float)));
    SS_HIP(hipMemcpyAsync(s->d_row_scale, row_scale, n_rows * sizeof(float), hipMemcpyHostToDevice, s->stream));
  }
  if (row_doc_ids) {
    SS_HIP(hipMalloc(&s->d_row_doc, n_rows * sizeof(uint32_t)));
    SS_HIP(hipMemcpyAsync(s->d_row_doc, row_doc_ids, n_rows * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
  }
  SS_HIP(hipStreamSynchronize(s->stream));
  return vec_finish(s);
}

// ------------------------------------------------------------------ append of one committed level of vector records
// The reference commits 65 536 docs at a time and writes the level's clusters and records behind the earlier ones
// (vector.rs:1066-1094); a rebuild of the whole image per commit would cost O(shard).  Rows are independent, so the new records are
// written behind the image's rows IN PLACE (f32: a strided copy; i8: through a row-major staging and the fragment-order scatter of the
// rows' range), the Euclidean side data is computed for the new range only, the per-row side arrays (doc ids, scales, norms, field
// ids) are extended, and the cluster structure -- if the image has one -- is declared again with the level added (O(rows) words, not
// O(image bytes)).  The image and the side arrays grow by half when their room is used up (one device-to-device copy, amortised).
// room for new_cap rows in the image and every per-row array it carries (caller holds s->mu, the device is idle).  ALL OR NOTHING:
// every new array is allocated before anything is copied or swapped, so a failure (SS_ENOMEM) leaves the shard as it was.
// grow_image = false: the image already has the room (its row padding), only the side arrays follow.
static int vec_grow(ss_shard* s, uint64_t new_cap, bool grow_image = true) {
  const bool i8 = s->d_X8 != nullptr;
  const size_t row_bytes = i8 ? (size_t)s->dim_pad8 : (size_t)s->dim_pad * sizeof(float);
  const uint64_t old_n = s->n_rows;
  struct G { void** p; size_t elem; uint64_t old_rows; bool zero_tail; void* q; };
  // the image: rows [0, n_rows_pad) are data + zero padding, the room behind them starts as padding (zero)
  G gs[] = {{i8 ? (void**)&s->d_X8 : (void**)&s->d_X, row_bytes, s->n_rows_pad, true, nullptr},
            {(void**)&s->d_row_doc, sizeof(uint32_t), old_n, false, nullptr},   {(void**)&s->d_row_scale, sizeof(float), old_n, false, nullptr},
            {(void**)&s->d_row_norm, sizeof(float), old_n, false, nullptr},     {(void**)&s->d_row_sq, sizeof(int32_t), old_n, false, nullptr},
            {(void**)&s->d_row_field, sizeof(uint16_t), old_n, false, nullptr}};
  int rc = SS_OK;
  for (size_t i = grow_image ? 0 : 1; i < sizeof(gs) / sizeof(gs[0]) && rc == SS_OK; i++) {
    G& g = gs[i];
    if (!*g.p) continue;
    const hipError_t e = hipMalloc(&g.q, (size_t)new_cap * g.elem);
    if (e != hipSuccess) { g.q = nullptr; rc = e == hipErrorOutOfMemory ? SS_ENOMEM : SS_EDEVICE; break; }
    if (hipMemcpy(g.q, *g.p, (size_t)g.old_rows * g.elem, hipMemcpyDeviceToDevice) != hipSuccess ||
        (g.zero_tail && hipMemset((char*)g.q + (size_t)g.old_rows * g.elem, 0, (size_t)(new_cap - g.old_rows) * g.elem) != hipSuccess))
      rc = SS_EDEVICE;
  }
  if (rc != SS_OK) {
    for (G& g : gs) if (g.q) (void)hipFree(g.q);
    return rc;
  }
  for (G& g : gs)
    if (g.q) { (void)hipFree(*g.p); *g.p = g.q; }
  s->vec_rows_cap = new_cap;
  return SS_OK;
}

int ss_vec_reserve_rows(ss_shard* s, uint64_t n_rows_cap) {
  if (!s) return SS_EINVAL;
  ShardLock g(s);
  if (s->vstream) (void)hipStreamSynchronize(s->vstream);  // (a coalesced scan in flight reads what this call replaces; none starts while mu is ours)
  SS_HIP(hipSetDevice(s->device));
  if (!s->d_X && !s->d_X8) return SS_ESTATE;
  if (n_rows_cap > 0xFFFFFFFEull) return SS_ENOTSUP;
  const uint64_t cap = s->vec_rows_cap ? s->vec_rows_cap : s->n_rows_pad, want = (n_rows_cap + VS_TR - 1) / VS_TR * VS_TR;
  if (want <= cap && s->vec_rows_cap) return SS_OK;
  SS_HIP(hipDeviceSynchronize());
  return vec_grow(s, std::max(want, cap));
}

int ss_vec_append_rows(ss_shard* s, const ss_vec_level* lv) {
  if (!s || !lv || !lv->rows || lv->n_rows == 0) return SS_EINVAL;
  const uint64_t n_new = lv->n_rows;
  bool multi = false;  // (a level's records share doc ids only among themselves: (level << 16) | doc_id, vector.rs:1448)
  SS_TRY(row_doc_ids_ok(lv->row_doc_ids, n_new, &multi));
  ShardLock g(s);
  if (s->vstream) (void)hipStreamSynchronize(s->vstream);  // (a coalesced scan in flight reads what this call replaces; none starts while mu is ours)
  SS_HIP(hipSetDevice(s->device));
  if (!s->d_X && !s->d_X8) return SS_ESTATE;
  const bool i8 = s->d_X8 != nullptr;
  if ((lv->elem_i8 != 0) != i8) return SS_EINVAL;
  // what the image carries per row, the level must bring -- and nothing else
  if ((s->d_row_doc != nullptr) != (lv->row_doc_ids != nullptr) || (s->d_row_scale != nullptr) != (lv->row_scale != nullptr) ||
      (s->d_row_norm != nullptr) != (lv->row_norm != nullptr) || (s->d_row_field != nullptr) != (lv->row_field != nullptr) ||
      (s->vec_n_clusters != 0) != (lv->n_clusters != 0))
    return SS_EINVAL;
  if (lv->n_clusters) {
    if (!lv->child_count) return SS_EINVAL;
    uint64_t sum = 0;
    for (uint32_t c = 0; c < lv->n_clusters; c++) { if (lv->child_count[c] == 0) return SS_ENOTSUP; sum += lv->child_count[c]; }
    if (sum != n_new) return SS_EINVAL;
  }
  const uint64_t old_n = s->n_rows, new_n = old_n + n_new;
  if (new_n > 0xFFFFFFFEull) return SS_ENOTSUP;
  const uint64_t new_pad = (new_n + VS_TR - 1) / VS_TR * VS_TR;
  SS_HIP(hipDeviceSynchronize());  // searches on the callers' own streams read the arrays that are written / replaced here
  const uint64_t cap = s->vec_rows_cap ? s->vec_rows_cap : s->n_rows_pad;
  // (an opener that expects commits reserves the room once: ss_vec_reserve_rows).  Otherwise: what is needed plus a bounded headroom
  // -- half of what there is, at most 4 M rows: old and new image are both live during the copy -- and on the FIRST append only the side
  // arrays (allocated for exactly n_rows) when the level still fits the image's own row padding
  if (new_pad > cap)
    SS_TRY(vec_grow(s, (std::max<uint64_t>(new_pad, std::min<uint64_t>(cap + cap / 2, new_pad + (4u << 20))) + VS_TR - 1) / VS_TR * VS_TR));
  else if (!s->vec_rows_cap)
    SS_TRY(vec_grow(s, cap, /*grow_image=*/false));
  if (!i8) {
    SS_HIP(hipMemcpy2DAsync(s->d_X + (size_t)old_n * s->dim_pad, (size_t)s->dim_pad * sizeof(float), lv->rows, (size_t)s->dim * sizeof(float),
                            (size_t)s->dim * sizeof(float), n_new, hipMemcpyHostToDevice, s->stream));
  } else {
    int8_t* stage = nullptr;
    SS_HIP(hipMalloc(&stage, (size_t)n_new * s->dim));
    int rc = hipMemcpyAsync(stage, lv->rows, (size_t)n_new * s->dim, hipMemcpyHostToDevice, s->stream) == hipSuccess ? SS_OK : SS_EDEVICE;
    if (rc == SS_OK) rc = ssi_vec8_permute_range(s, stage, old_n, n_new, s->stream);
    (void)hipStreamSynchronize(s->stream);
    (void)hipFree(stage);
    if (rc) return rc;
  }
  if (lv->row_doc_ids) SS_HIP(hipMemcpyAsync(s->d_row_doc + old_n, lv->row_doc_ids, n_new * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
  if (lv->row_scale) SS_HIP(hipMemcpyAsync(s->d_row_scale + old_n, lv->row_scale, n_new * sizeof(float), hipMemcpyHostToDevice, s->stream));
  if (lv->row_norm) SS_HIP(hipMemcpyAsync(s->d_row_norm + old_n, lv->row_norm, n_new * sizeof(float), hipMemcpyHostToDevice, s->stream));
  if (lv->row_field) SS_HIP(hipMemcpyAsync(s->d_row_field + old_n, lv->row_field, n_new * sizeof(uint16_t), hipMemcpyHostToDevice, s->stream));
  s->n_rows = new_n;
  s->n_rows_pad = new_pad;
  s->vec_multi_record = s->vec_multi_record || multi;
  if (s->vec_similarity == SS_SIM_EUCLIDEAN) SS_TRY(s->d_X ? ssi_vec_augment(s, s->stream, old_n) : ssi_vec8_row_sq(s, s->stream, old_n));
  SS_HIP(hipStreamSynchronize(s->stream));
  if (lv->n_clusters) {  // the structure with the level added, declared again (row -> cluster words, the new medoids, tile lists)
    std::vector<uint32_t> lc = s->h_level_clusters, cc = s->h_child_count;
    lc.push_back(lv->n_clusters);
    cc.insert(cc.end(), lv->child_count, lv->child_count + lv->n_clusters);
    SS_TRY(ssi_vec_set_clusters(s, (uint32_t)lc.size(), lc.data(), cc.data()));
  }
  return SS_OK;
}

// bench / test utility: the synthetic f32 corpus of ss_vec_synth quantised on the device with quantize_f32_to_i8
int ss_vec_synth_i8(ss_shard* s, uint64_t seed, uint64_t n_rows, uint32_t dim) {
  if (!s || n_rows == 0 || dim == 0) return SS_EINVAL;
  if (n_rows > 0xFFFFFFFEull) return SS_ENOTSUP;
  ShardLock g(s);
  SS_HIP(hipSetDevice(s->device));
  SS_HIP(hipStreamSynchronize(s->stream));
  int rc = vec_alloc(s, n_rows, dim);  // f32 rows first ...
  if (rc) { ssi_vec_free(s); return rc; }
  SS_TRY(ssi_vec_synth(s, seed, s->stream));
  float* x32 = s->d_X;
  const uint32_t pad32 = s->dim_pad;
  s->d_X = nullptr;  // ... kept aside while the i8 image is allocated (ssi_vec_free must not release them)
  rc = vec8_alloc(s, n_rows, dim);
  if (rc) { (void)hipFree(x32); return rc; }
  s->d_X = x32;
  s->dim_pad = pad32;
  rc = ssi_vec8_quantize(s, s->stream);
  (void)hipStreamSynchronize(s->stream);
  (void)hipFree(x32);
  s->d_X = nullptr;
  s->dim_pad = 0;
  if (rc) { ssi_vec_free(s); return rc; }
  return vec_finish(s);
}

int ss_vec_read_rows_i8(ss_shard* s, uint64_t r0, uint64_t n, int8_t* out) {
  if (!s || !out) return SS_EINVAL;
  if (!s->d_X8) return SS_ESTATE;
  if (r0 + n > s->n_rows) return SS_EINVAL;
  ShardLock g(s);
  SS_HIP(hipSetDevice(s->device));
  SS_HIP(hipStreamSynchronize(s->stream));
  if (n == 0) return SS_OK;
  int8_t* tmp = nullptr;
  SS_HIP(hipMalloc(&tmp, (size_t)n * s->dim));
  int rc = ssi_vec8_gather_rows(s, r0, n, tmp, s->stream);
  if (rc == SS_OK && hipMemcpyAsync(out, tmp, (size_t)n * s->dim, hipMemcpyDeviceToHost, s->stream) != hipSuccess) rc = SS_EDEVICE;
  (void)hipStreamSynchronize(s->stream);
  (void)hipFree(tmp);
  return rc;
}

int ss_vec_search_i8_euclid(ss_shard* s, uint32_t nq, const int8_t* queries, const float* query_scale, const float* query_norm,
                            uint32_t k, float thr, const ss_ann_mode* mode, uint32_t* out_doc, float* out_score, uint32_t* out_count,
                            uint64_t* out_total, uint32_t* out_clusters) {
  return vec_search_host_entry(s, nq, queries, 1, query_scale, query_norm, k, thr, mode, out_doc, out_score, out_count, out_total, out_clusters);
}
int ss_vec_search_i8_ann(ss_shard* s, uint32_t nq, const int8_t* queries, const float* query_scale, uint32_t k, float thr,
                         const ss_ann_mode* mode, uint32_t* out_doc, float* out_score, uint32_t* out_count, uint64_t* out_total,
                         uint32_t* out_clusters) {
  return vec_search_host_entry(s, nq, queries, 1, query_scale, nullptr, k, thr, mode, out_doc, out_score, out_count, out_total, out_clusters);
}
int ss_vec_search_i8(ss_shard* s, uint32_t nq, const int8_t* queries, const float* query_scale, uint32_t k, float thr,
                     uint32_t* out_doc, float* out_score, uint32_t* out_count, uint64_t* out_total) {
  return vec_search_host_entry(s, nq, queries, 1, query_scale, nullptr, k, thr, nullptr, out_doc, out_score, out_count, out_total, nullptr);
}

int ss_vec_search_i8_euclid_dev(ss_shard* s, uint32_t nq, const int8_t* d_queries, const float* d_query_scale, const float* d_query_norm,
                                uint32_t k, float thr, const ss_ann_mode* mode, uint32_t* d_out_doc, float* d_out_score,
                                uint32_t* d_out_count, uint64_t* d_out_total, uint32_t* d_out_clusters, void* stream) {
  return vec_search_dev_entry(s, nq, d_queries, 1, d_query_scale, d_query_norm, k, thr, mode, d_out_doc, d_out_score, d_out_count, d_out_total,
                              d_out_clusters, stream);
}
int ss_vec_search_i8_ann_dev(ss_shard* s, uint32_t nq, const int8_t* d_queries, const float* d_query_scale, uint32_t k, float thr,
                             const ss_ann_mode* mode, uint32_t* d_out_doc, float* d_out_score, uint32_t* d_out_count,
                             uint64_t* d_out_total, uint32_t* d_out_clusters, void* stream) {
  return vec_search_dev_entry(s, nq, d_queries, 1, d_query_scale, nullptr, k, thr, mode, d_out_doc, d_out_score, d_out_count, d_out_total,
                              d_out_clusters, stream);
}
int ss_vec_search_i8_dev(ss_shard* s, uint32_t nq, const int8_t* d_queries, const float* d_query_scale, uint32_t k, float thr,
                         uint32_t* d_out_doc, float* d_out_score, uint32_t* d_out_count, uint64_t* d_out_total, void* stream) {
  return vec_search_dev_entry(s, nq, d_queries, 1, d_query_scale, nullptr, k, thr, nullptr, d_out_doc, d_out_score, d_out_count, d_out_total,
                              nullptr, stream);
}
}  // extern "C"
