// Expression queries (DESIGN.md "Expression queries"): a weighted sum of stored rows as the query, and the operands
// removed from its answer, without leaving the device.
//   compose_rows_kernel   term lists (CSR: offsets, rows, weights) -> query vectors.  Per term Index.lookup(row) --
//                         row_decode.hpp's decoded_coordinate, with lookup_base for a GroupedIndex -- optionally
//                         MathUtils.normalize (MathUtils.scala:100-120); per coordinate
//                           acc = w_0 * v_0[e];  acc = acc + (w_t * v_t[e])  for t = 1, 2, ... in list order,
//                         every product and every sum a binary32 operation of its own; optionally MathUtils.normalize
//                         of the sum (SortedIndex.prepare, Index.scala:324-331).
//   drop_rows_kernel      the index's answer at depth k_nn + extra -> the first k_nn entries whose row is none of the
//                         query's term rows, in their order, padded as gulon_index_batch_query pads.
// Between the two runs the handle's own *_dev batch query, on the same stream: tie flags, the peeled order above 63
// neighbours and the limits of the index form are inherited.
#include "compose.hpp"
#include "row_decode.hpp"

namespace gulon {

// One wavefront per query.  in_*: [b][kin] lists with in_count[q] live entries (row ids carry the index's row_base, the
// term rows do not).  The live entries are walked 64 at a time; an entry is kept unless its row is one of the query's
// term rows; kept entries are compacted in order by ballot + prefix popcount until k_nn are out.
__global__ __launch_bounds__(64) void drop_rows_kernel(const int *__restrict__ in_idx, const float *__restrict__ in_dist,
                                                       const int *__restrict__ in_count, int kin, int k_nn,
                                                       const int *__restrict__ term_offsets,
                                                       const int *__restrict__ term_rows, int row_base,
                                                       int *__restrict__ out_idx, float *__restrict__ out_dist,
                                                       int *__restrict__ out_count) {
  const int q = blockIdx.x, lane = threadIdx.x;
  const int live = min(max(in_count[q], 0), kin);
  const int t0 = term_offsets[q], t1 = term_offsets[q + 1];
  const int *ii = in_idx + (size_t)q * kin;
  const float *iv = in_dist + (size_t)q * kin;
  int *oi = out_idx + (size_t)q * k_nn;
  float *ov = out_dist + (size_t)q * k_nn;
  int kept = 0;
  for (int c0 = 0; c0 < live && kept < k_nn; c0 += 64) {
    const int p = c0 + lane;
    const bool have = p < live;
    const int id = have ? ii[p] : -1;
    const float dv = have ? iv[p] : 0.f;
    bool keep = have;
    for (int t = t0; t < t1; t++) keep = keep && (id - row_base != term_rows[t]);
    const unsigned long long mask = __ballot(keep);
    const int pos = kept + __popcll(mask & ((1ull << lane) - 1ull));
    if (keep && pos < k_nn) { oi[pos] = id; ov[pos] = dv; }
    kept += __popcll(mask);
  }
  kept = min(kept, k_nn);
  for (int p = kept + lane; p < k_nn; p += 64) { oi[p] = -1; ov[p] = INFINITY; }
  if (lane == 0 && out_count) out_count[q] = kept;
}

void launch_drop(const int *in_idx, const float *in_dist, const int *in_count, int b, int kin, int k_nn,
                 const int *d_off, const int *d_rows, int row_base, int *out_idx, float *out_dist, int *out_count,
                 hipStream_t st) {
  if (b == 0) return;
  hipLaunchKernelGGL(drop_rows_kernel, dim3(b), dim3(64), 0, st, in_idx, in_dist, in_count, kin, k_nn, d_off, d_rows,
                     row_base, out_idx, out_dist, out_count);
  HIP_CHECK(hipGetLastError());
}

int check_terms_host(const int32_t *off, const int32_t *rows, const float *w, int b, int n) {
  GULON_REQUIRE(b >= 0, "batch size must be non-negative");
  if (b == 0) return 0;
  GULON_REQUIRE(off != nullptr && rows != nullptr && w != nullptr, "null argument");
  GULON_REQUIRE(off[0] == 0, "term_offsets[0] = %d, expected 0", off[0]);
  for (int q = 0; q < b; q++)
    GULON_REQUIRE(off[q + 1] > off[q], "expression %d is empty (term offsets must ascend strictly)", q);
  for (int t = 0; t < off[b]; t++)
    GULON_REQUIRE(rows[t] >= 0 && rows[t] < n, "term %d: row %d outside [0, %d)", t, rows[t], n);
  return off[b];
}

namespace {

// One workgroup per expression (compose.hpp's compose_terms), a term row read as Index.lookup reads it.  An expression
// without terms, or with a term row outside [0, n), gives an all-NaN vector and sets *err (nothing is read for it).
template <int CPT>
__global__ __launch_bounds__(CR_THREADS) void compose_rows_kernel(
    CodeSrc src, const float *__restrict__ cents, int n, int d, int k, const int *__restrict__ term_offsets,
    const int *__restrict__ term_rows, const float *__restrict__ term_weights, const float *__restrict__ gcent,
    const int *__restrict__ offsets, int n_offsets, int normalize_terms, int normalize_query, float *__restrict__ out,
    int *__restrict__ err) {
  extern __shared__ float xs[];   // [d], and [d] more when terms are normalised
  const int b = blockIdx.x;
  const int t0 = term_offsets[b], t1 = term_offsets[b + 1];
  float *o = out + (size_t)b * d;
  if (terms_unusable(term_rows, t0, t1, n)) {   // (uniform over the workgroup: no barrier is skipped by a part of it)
    write_nan_vector(o, d, threadIdx.x, err);
    return;
  }
  const SubvectorMap sv(d, src.m);
  compose_terms<CPT>(t0, t1, term_rows, term_weights, d, normalize_terms, normalize_query, xs, o, [&](int row) {
    const float *base = gcent ? lookup_base(gcent, offsets, n_offsets, row, d) : nullptr;
    return [&, row, base](int e) { return decoded_coordinate(src, sv, cents, k, row, e, base); };
  });
}

void launch_compose(const gulon_index *ix, const int *d_off, const int *d_rows, const float *d_w, int b,
                    const float *gcent, const int *offsets, int n_offsets, bool norm_terms, bool norm_query,
                    float *d_out, int *d_err, hipStream_t st) {
  GULON_REQUIRE(b >= 0, "batch size must be non-negative");
  GULON_UNSUPPORTED((size_t)ix->d * sizeof(float) > 64 * 1024, "d = %d: a decoded row does not fit in LDS", ix->d);
  if (b == 0) return;
  GULON_REQUIRE(d_off != nullptr && d_rows != nullptr && d_w != nullptr && d_out != nullptr, "null argument");
  const size_t lds = compose_lds_bytes(ix->d, norm_terms, norm_query);
#define CR(CPT) hipLaunchKernelGGL(compose_rows_kernel<CPT>, dim3(b), dim3(CR_THREADS), lds, st, code_src(ix), \
                                   ix->cents.p, ix->n, ix->d, ix->k, d_off, d_rows, d_w, gcent, offsets, n_offsets, \
                                   norm_terms ? 1 : 0, norm_query ? 1 : 0, d_out, d_err)
  if (ix->d <= CR_THREADS) CR(1);
  else if (ix->d <= 4 * CR_THREADS) CR(4);
  else if (ix->d <= 16 * CR_THREADS) CR(16);
  else {
    if (lds > 64 * 1024)   // xs and ys of a row above 8192 coordinates: more than the default dynamic LDS of a launch
      HIP_CHECK(hipFuncSetAttribute((const void *)compose_rows_kernel<64>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds));
    CR(64);
  }
#undef CR
  HIP_CHECK(hipGetLastError());
}

void upload_terms(ExprWork &x, const int32_t *off, const int32_t *rows, const float *w, int b, int terms,
                  hipStream_t st) {
  x.off.upload(off, (size_t)b + 1, st);
  x.rows.upload(rows, (size_t)terms, st);
  x.w.upload(w, (size_t)terms, st);
}

void check_depth(int b, int k_nn, int extra) {
  GULON_REQUIRE(b >= 0 && k_nn >= 0 && extra >= 0, "k, extra and batch size must be non-negative");
  GULON_REQUIRE((long long)k_nn + extra <= INT_MAX, "k + extra overflows");
}

void rethrow(int32_t rc) {   // a nested entry point has recorded its message
  if (rc != GULON_OK) throw DeviceError{rc};
}

// ---- flat index -------------------------------------------------------------------------------------------------------

void compose_flat(gulon_index *idx, const int *d_off, const int *d_rows, const float *d_w, int b, bool nt, bool nq,
                  float *d_out, bool dev_rows, hipStream_t st) {
  std::lock_guard<std::mutex> lock(idx->mu);
  idx->pend_b = -1;
  StreamOrder so(idx, st);
  if (dev_rows) ensure_row_err(idx);
  launch_compose(idx, d_off, d_rows, d_w, b, nullptr, nullptr, 0, nt, nq, d_out, dev_rows ? idx->row_err.p : nullptr, st);
  so.done();
}

// compose -> the handle's own batch query at k_nn + extra -> drop.  Called with idx->expr.mu held.
void query_terms_flat(gulon_index *idx, const int *d_off, const int *d_rows, const float *d_w, int b, int k_nn, int extra,
                      bool nt, bool nq, int from, int until, int *d_oi, float *d_od, int *d_oc, int *d_of,
                      bool dev_rows, hipStream_t st) {
  ExprWork &x = idx->expr;
  const int kin = k_nn + extra;
  x.q.ensure((size_t)b * idx->d + 1);
  x.oi.ensure((size_t)b * kin + 1);
  x.od.ensure((size_t)b * kin + 1);
  x.oc.ensure((size_t)b + 1);
  compose_flat(idx, d_off, d_rows, d_w, b, nt, nq, x.q.p, dev_rows, st);
  rethrow(gulon_index_batch_query_dev(idx, x.q.p, b, kin, from, until, x.oi.p, x.od.p, x.oc.p, d_of, st));
  std::lock_guard<std::mutex> lock(idx->mu);
  StreamOrder so(idx, st);
  launch_drop(x.oi.p, x.od.p, x.oc.p, b, kin, k_nn, d_off, d_rows, idx->row_base, d_oi, d_od, d_oc, st);
  so.done();   // the next call on another stream waits for the drop, which reads this workspace
}

// ---- grouped index ----------------------------------------------------------------------------------------------------

void compose_grouped(const GroupedParts &g, const int *d_off, const int *d_rows, const float *d_w, int b, bool nt,
                     bool nq, float *d_out, bool dev_rows, hipStream_t st) {
  std::lock_guard<std::mutex> lock(*g.mu);
  StreamOrder so(g.pq, st);
  if (dev_rows) ensure_row_err(g.pq);
  launch_compose(g.pq, d_off, d_rows, d_w, b, g.gcent, g.offsets, g.n_offsets, nt, nq, d_out,
                 dev_rows ? g.pq->row_err.p : nullptr, st);
  so.done();
}

void query_terms_grouped(gulon_grouped_index *idx, const GroupedParts &g, const int *d_off, const int *d_rows,
                         const float *d_w, int b, int k_nn, int extra, bool nt, bool nq, int strategy, int limit,
                         int *d_oi, float *d_od, int *d_oc, bool dev_rows, hipStream_t st) {
  ExprWork &x = g.pq->expr;
  const int kin = k_nn + extra;
  x.q.ensure((size_t)b * g.pq->d + 1);
  x.oi.ensure((size_t)b * kin + 1);
  x.od.ensure((size_t)b * kin + 1);
  x.oc.ensure((size_t)b + 1);
  compose_grouped(g, d_off, d_rows, d_w, b, nt, nq, x.q.p, dev_rows, st);
  rethrow(gulon_grouped_index_batch_query_dev(idx, x.q.p, b, kin, strategy, limit, x.oi.p, x.od.p, x.oc.p, st));
  std::lock_guard<std::mutex> lock(*g.mu);
  StreamOrder so(g.pq, st);
  launch_drop(x.oi.p, x.od.p, x.oc.p, b, kin, k_nn, d_off, d_rows, 0, d_oi, d_od, d_oc, st);
  so.done();   // the next call on another stream waits for the drop, which reads this workspace
}

}  // namespace
}  // namespace gulon

using namespace gulon;

GULON_API int32_t gulon_index_compose_rows_dev(gulon_index *idx, const int32_t *d_term_offsets,
                                               const int32_t *d_term_rows, const float *d_term_weights, int32_t b,
                                               int32_t normalize_terms, int32_t normalize_query, float *d_out,
                                               void *stream) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    compose_flat(idx, d_term_offsets, d_term_rows, d_term_weights, b, normalize_terms != 0, normalize_query != 0, d_out,
                 true, (hipStream_t)stream);
  });
}

GULON_API int32_t gulon_index_compose_rows(gulon_index *idx, const int32_t *term_offsets, const int32_t *term_rows,
                                           const float *term_weights, int32_t b, int32_t normalize_terms,
                                           int32_t normalize_query, float *out) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    const int terms = check_terms_host(term_offsets, term_rows, term_weights, b, idx->n);
    if (b == 0) return;
    GULON_REQUIRE(out != nullptr, "null argument");
    ExprWork &x = idx->expr;
    std::lock_guard<std::mutex> work(x.mu);
    const hipStream_t st = nullptr;
    upload_terms(x, term_offsets, term_rows, term_weights, b, terms, st);
    x.q.ensure((size_t)b * idx->d);
    compose_flat(idx, x.off.p, x.rows.p, x.w.p, b, normalize_terms != 0, normalize_query != 0, x.q.p, false, st);
    x.q.download(out, (size_t)b * idx->d, st);
    HIP_CHECK(hipStreamSynchronize(st));
  });
}

GULON_API int32_t gulon_grouped_index_compose_rows_dev(gulon_grouped_index *idx, const int32_t *d_term_offsets,
                                                       const int32_t *d_term_rows, const float *d_term_weights,
                                                       int32_t b, int32_t normalize_terms, int32_t normalize_query,
                                                       float *d_out, void *stream) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    compose_grouped(grouped_parts(idx), d_term_offsets, d_term_rows, d_term_weights, b, normalize_terms != 0,
                    normalize_query != 0, d_out, true, (hipStream_t)stream);
  });
}

GULON_API int32_t gulon_grouped_index_compose_rows(gulon_grouped_index *idx, const int32_t *term_offsets,
                                                   const int32_t *term_rows, const float *term_weights, int32_t b,
                                                   int32_t normalize_terms, int32_t normalize_query, float *out) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    const GroupedParts g = grouped_parts(idx);
    const int terms = check_terms_host(term_offsets, term_rows, term_weights, b, g.pq->n);
    if (b == 0) return;
    GULON_REQUIRE(out != nullptr, "null argument");
    ExprWork &x = g.pq->expr;
    std::lock_guard<std::mutex> work(x.mu);
    const hipStream_t st = nullptr;
    upload_terms(x, term_offsets, term_rows, term_weights, b, terms, st);
    x.q.ensure((size_t)b * g.pq->d);
    compose_grouped(g, x.off.p, x.rows.p, x.w.p, b, normalize_terms != 0, normalize_query != 0, x.q.p, false, st);
    x.q.download(out, (size_t)b * g.pq->d, st);
    HIP_CHECK(hipStreamSynchronize(st));
  });
}

GULON_API int32_t gulon_index_query_terms_dev(gulon_index *idx, const int32_t *d_term_offsets,
                                              const int32_t *d_term_rows, const float *d_term_weights, int32_t b,
                                              int32_t k_nn, int32_t extra, int32_t normalize_terms,
                                              int32_t normalize_query, int32_t from, int32_t until, int32_t *d_out_idx,
                                              float *d_out_dist, int32_t *d_out_count, int32_t *d_out_flags,
                                              void *stream) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    check_depth(b, k_nn, extra);
    std::lock_guard<std::mutex> work(idx->expr.mu);
    query_terms_flat(idx, d_term_offsets, d_term_rows, d_term_weights, b, k_nn, extra, normalize_terms != 0,
                     normalize_query != 0, from, until, d_out_idx, d_out_dist, d_out_count, d_out_flags, true,
                     (hipStream_t)stream);
  });
}

GULON_API int32_t gulon_index_query_terms(gulon_index *idx, const int32_t *term_offsets, const int32_t *term_rows,
                                          const float *term_weights, int32_t b, int32_t k_nn, int32_t extra,
                                          int32_t normalize_terms, int32_t normalize_query, int32_t from,
                                          int32_t until, int32_t *out_idx, float *out_dist, int32_t *out_count,
                                          int32_t *out_flags) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    check_depth(b, k_nn, extra);
    const int terms = check_terms_host(term_offsets, term_rows, term_weights, b, idx->n);
    ExprWork &x = idx->expr;
    std::lock_guard<std::mutex> work(x.mu);
    const hipStream_t st = nullptr;
    const size_t bk = (size_t)b * (size_t)k_nn;
    if (b > 0) upload_terms(x, term_offsets, term_rows, term_weights, b, terms, st);
    x.fi.ensure(bk + 1); x.fd.ensure(bk + 1); x.fc.ensure((size_t)b + 1); x.ff.ensure((size_t)b + 1);
    query_terms_flat(idx, x.off.p, x.rows.p, x.w.p, b, k_nn, extra, normalize_terms != 0, normalize_query != 0, from,
                     until, x.fi.p, x.fd.p, x.fc.p, x.ff.p, false, st);
    if (bk) { x.fi.download(out_idx, bk, st); x.fd.download(out_dist, bk, st); }
    if (b > 0 && out_count) x.fc.download(out_count, (size_t)b, st);
    if (b > 0 && out_flags) x.ff.download(out_flags, (size_t)b, st);
    HIP_CHECK(hipStreamSynchronize(st));
  });
}

GULON_API int32_t gulon_grouped_index_query_terms_dev(gulon_grouped_index *idx, const int32_t *d_term_offsets,
                                                      const int32_t *d_term_rows, const float *d_term_weights,
                                                      int32_t b, int32_t k_nn, int32_t extra, int32_t normalize_terms,
                                                      int32_t normalize_query, int32_t strategy, int32_t limit,
                                                      int32_t *d_out_idx, float *d_out_dist, int32_t *d_out_count,
                                                      void *stream) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    check_depth(b, k_nn, extra);
    const GroupedParts g = grouped_parts(idx);
    std::lock_guard<std::mutex> work(g.pq->expr.mu);
    query_terms_grouped(idx, g, d_term_offsets, d_term_rows, d_term_weights, b, k_nn, extra, normalize_terms != 0,
                        normalize_query != 0, strategy, limit, d_out_idx, d_out_dist, d_out_count, true,
                        (hipStream_t)stream);
  });
}

GULON_API int32_t gulon_grouped_index_query_terms(gulon_grouped_index *idx, const int32_t *term_offsets,
                                                  const int32_t *term_rows, const float *term_weights, int32_t b,
                                                  int32_t k_nn, int32_t extra, int32_t normalize_terms,
                                                  int32_t normalize_query, int32_t strategy, int32_t limit,
                                                  int32_t *out_idx, float *out_dist, int32_t *out_count) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    check_depth(b, k_nn, extra);
    const GroupedParts g = grouped_parts(idx);
    const int terms = check_terms_host(term_offsets, term_rows, term_weights, b, g.pq->n);
    ExprWork &x = g.pq->expr;
    std::lock_guard<std::mutex> work(x.mu);
    const hipStream_t st = nullptr;
    const size_t bk = (size_t)b * (size_t)k_nn;
    if (b > 0) upload_terms(x, term_offsets, term_rows, term_weights, b, terms, st);
    x.fi.ensure(bk + 1); x.fd.ensure(bk + 1); x.fc.ensure((size_t)b + 1);
    query_terms_grouped(idx, g, x.off.p, x.rows.p, x.w.p, b, k_nn, extra, normalize_terms != 0, normalize_query != 0,
                        strategy, limit, x.fi.p, x.fd.p, x.fc.p, false, st);
    if (bk) { x.fi.download(out_idx, bk, st); x.fd.download(out_dist, bk, st); }
    if (b > 0 && out_count) x.fc.download(out_count, (size_t)b, st);
    HIP_CHECK(hipStreamSynchronize(st));
  });
}
