// Offset queries and the mean similarity of CSLS (Conneau et al. 2018).  Per query q and per row r of the
// handle's range:
//   d   the distance the handle's ordinary query returns between q and r;
//   t   = d + offsets[r], one binary32 addition;
// a row is a candidate if and only if t is finite and r is not exclude[q]; the answer is the candidates by (t ascending,
// row id ascending), the first k_nn.  On unit vectors CSLS(x, y) = 2 - d(x, y) - r_T(x) - r_S(y), so with
// offsets = r_S the order is that of CSLS descending; an offset of +inf masks a row.
//
//   exact index   offset_exact_scan: knn.hip's knn_kernel with the offset -- 16 queries per workgroup, lane = row, the d
//                 by exact_tile (exact.hpp), the row's offset loaded once per 256-row step and added to each of the 16
//                 sums
//   flat index    launch_build_tables(): Index.prepareQuery of every query; offset_flat_scan: the flat table scan
//                 (table_scan.hpp) of a workgroup's E queries, one offset load per row shared by the E queries, each
//                 with its own WaveList and excluded row
//   both          t into the query's WaveList (wave_offer), which orders by (key ascending, row ascending); the
//                 workgroup's lists merged (merge_wave_lists) into the chunk's; launch_merge: the row chunks' lists ->
//                 the first k_nn, -1 / +inf after the last.  The lists' own padding is (+inf, INT_MAX); a candidate's
//                 key is finite, so the two are never confused.
//   mean_similarity_kernel   out[q] = the mean of 1 - 0.5 * d_j over the first min(count, K) entries of a distance list
//                 (r_S of CSLS from the source's answer to a target row), one thread per list.
#include "offset.hpp"
#include "exact.hpp"

namespace gulon {
namespace {

// ---- exact index ------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(KNN_THREADS) void offset_exact_scan(const float *__restrict__ X, int n, int d,
                                                                 const float *__restrict__ Qt,
                                                                 const float *__restrict__ offsets,
                                                                 const int *__restrict__ exclude, int b, int row_from,
                                                                 int row_until, int rows_per_chunk, int nchunks,
                                                                 int keff, float *__restrict__ part_v,
                                                                 int *__restrict__ part_i) {
  constexpr int NW = KNN_THREADS / 64;
  __shared__ float xs[KNN_THREADS * (KNN_DT + 1)];
  __shared__ float sv[KNN_QT * NW * 64];
  __shared__ int si[KNN_QT * NW * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tile = blockIdx.x, chunk = blockIdx.y;
  const float *qt = Qt + (size_t)tile * d * KNN_QT;

  WaveList wl[KNN_QT];
  int cnt[KNN_QT], ex[KNN_QT];
#pragma unroll
  for (int q = 0; q < KNN_QT; q++) {
    wl[q].init(); cnt[q] = 0;
    const int qg = tile * KNN_QT + q;
    ex[q] = __builtin_amdgcn_readfirstlane((exclude != nullptr && qg < b) ? exclude[qg] : -1);
  }

  const int r0 = (row_from / KNN_THREADS) * KNN_THREADS + chunk * rows_per_chunk;
  const int r1 = min(row_until, r0 + rows_per_chunk);
  for (int base = r0; base < r1; base += KNN_THREADS) {
    float acc[KNN_QT];
    exact_tile(X, n, d, qt, xs, tid, [&](int r) { return base + r; }, acc);
    const int row = base + tid;
    const bool in = row >= row_from && row < row_until;
    const float off = in ? offsets[row] : 0.f;
#pragma unroll
    for (int q = 0; q < KNN_QT; q++) {
      const float t = __fadd_rn(acc[q], off);
      const bool valid = in && finite_key(t) && row != ex[q];
      wave_offer(wl[q], cnt[q], t, valid, __ballot(valid), base + wave * 64, keff, lane);
    }
  }
  __syncthreads();
  merge_wave_lists<KNN_QT, NW>(wl, sv, si, keff, lane, wave, [&](int q, const WaveList &out) {
    if (lane < keff) {   // (part_* hold ceil(b / 16) * 16 queries)
      const size_t o = ((size_t)(tile * KNN_QT + q) * nchunks + chunk) * keff + lane;
      part_v[o] = out.v;
      part_i[o] = out.i;
    }
  });
}

// ---- flat index -------------------------------------------------------------------------------------------------------

// A workgroup is (E query slots, row chunk): slot t is query blockIdx.x * E + t, its table in LDS (table_scan.hpp); the
// slots past the batch hold zero tables and offer nothing.
template <int E, int VEC>
__global__ __launch_bounds__(TABLE_SCAN_THREADS) void offset_flat_scan(
    const uint8_t *__restrict__ codes, int ng, int m_pad, const float *__restrict__ tables,
    const float *__restrict__ offsets, const int *__restrict__ exclude, int b, int row_from, int row_until, int row_base,
    int rb_begin, int rb_end, int rb_per_chunk, int nchunks, int keff, float *__restrict__ part_v,
    int *__restrict__ part_i) {
  constexpr int NW = TABLE_SCAN_THREADS / 64;
  extern __shared__ float4 lds4[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q0 = blockIdx.x * E, chunk = blockIdx.y;
  const int tab = m_pad * 256;
  const int nq = min(E, b - q0);   // live slots (uniform over the workgroup)
  stage_tables(lds4, tables + (size_t)q0 * tab, tab, nq, E, tid);

  WaveList wl[E];
  int cnt[E], ex[E];
#pragma unroll
  for (int t = 0; t < E; t++) {
    wl[t].init(); cnt[t] = 0;
    ex[t] = __builtin_amdgcn_readfirstlane((exclude != nullptr && t < nq) ? exclude[q0 + t] : -1);
  }

  const int rb0 = rb_begin + chunk * rb_per_chunk, rb1 = min(rb_end, rb0 + rb_per_chunk);
  table_scan_rows<E, VEC>(codes, ng, tab, reinterpret_cast<const float *>(lds4), rb0, rb1, lane, wave,
                          [&](int rb, const float (&acc)[E]) {
    const int row = rb * 64 + lane;
    const bool in = row >= row_from && row < row_until;
    const float off = in ? offsets[row] : 0.f;
    const int id = row + row_base;
#pragma unroll
    for (int t = 0; t < E; t++) {
      if (t < nq) {   // (uniform over the workgroup)
        const float key = __fadd_rn(acc[t], off);
        const bool valid = in && finite_key(key) && id != ex[t];
        wave_offer(wl[t], cnt[t], key, valid, __ballot(valid), rb * 64 + row_base, keff, lane);
      }
    }
  });
  __syncthreads();   // every wave is done with the tables: their LDS takes the lists
  float *sv = reinterpret_cast<float *>(lds4);
  int *si = reinterpret_cast<int *>(sv + E * NW * 64);
  merge_wave_lists<E, NW>(wl, sv, si, keff, lane, wave, [&](int t, const WaveList &out) {
    if (lane < keff && t < nq) {
      const size_t o = ((size_t)(q0 + t) * nchunks + chunk) * keff + lane;
      part_v[o] = out.v;
      part_i[o] = out.i;
    }
  });
}

// Rows [from, until) of a flat byte-code index against the b queries at d_q; called with x.mu held and the handle's
// mutex free.  The arguments are checked (check_flat) by the caller; the passes by flat_passes (offset.hpp).
void launch_offset_flat(gulon_index *ix, OffsetWork &x, const float *d_q, int b, int k_nn, int from, int until,
                        const float *d_off, const int *d_ex, int *out_idx, float *out_key, int *out_count,
                        hipStream_t st) {
  if (b == 0) return;
  GULON_REQUIRE(d_q != nullptr && d_off != nullptr && out_idx != nullptr && out_key != nullptr, "null argument");
  const int keff = k_nn + 1;
  flat_passes(ix, x.tables, d_q, b, from, until, st, [&](int q0, int nb, int E, const FlatShape &s) {
    x.pv.ensure((size_t)nb * s.nchunks * keff); x.pi.ensure((size_t)nb * s.nchunks * keff);
    dispatch_e_vec(E, ix->vec, [&](auto e, auto vec) {
      const auto scan = offset_flat_scan<decltype(e)::value, decltype(vec)::value>;
      const size_t lds_bytes = (size_t)e * flat_slot_bytes(ix->m_pad);
      HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(scan), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds_bytes));
      hipLaunchKernelGGL(scan, dim3(ceil_div(nb, e), s.nchunks), dim3(TABLE_SCAN_THREADS), lds_bytes, st, ix->codes.p,
                         ix->ng, ix->m_pad, x.tables.p, d_off, d_ex ? d_ex + q0 : nullptr, nb, from, until, ix->row_base,
                         from / 64, ceil_div(until, 64), s.rb_per_chunk, s.nchunks, keff, x.pv.p, x.pi.p);
      HIP_CHECK(hipGetLastError());
    });
    launch_merge(x.pv.p, x.pi.p, s.nchunks, (long long)keff, (long long)s.nchunks * keff, nb, k_nn,
                 QueryOut::final_lists(out_idx, out_key, out_count, nullptr).from_query(q0, k_nn), st);
  });
}

// ---- mean similarity ----------------------------------------------------------------------------------------------------

__global__ void mean_similarity_kernel(const float *__restrict__ dist, const int *__restrict__ counts, int b, int kin,
                                       int K, float *__restrict__ out) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= b) return;
  const int c = min(max(counts ? counts[q] : kin, 0), min(kin, K));
  float sum = 0.f;
  const float *dq = dist + (size_t)q * kin;
  for (int j = 0; j < c; j++) {
    const float s = __fsub_rn(1.f, __fmul_rn(0.5f, dq[j]));
    sum = j == 0 ? s : __fadd_rn(sum, s);
  }
  out[q] = c == 0 ? 0.f : __fdiv_rn(sum, (float)c);
}

void launch_mean_similarity(const float *d_dist, const int *d_counts, int b, int kin, int K, float *d_out,
                            hipStream_t st) {
  GULON_REQUIRE(b >= 0 && kin >= 1 && K >= 1, "expected: b >= 0, kin >= 1, K >= 1");
  if (b == 0) return;
  GULON_REQUIRE(d_dist != nullptr && d_out != nullptr, "null argument");
  hipLaunchKernelGGL(mean_similarity_kernel, dim3(ceil_div(b, 256)), dim3(256), 0, st, d_dist, d_counts, b, kin, K,
                     d_out);
  HIP_CHECK(hipGetLastError());
}

}  // namespace

void check_rows_host(const float *offsets, bool nullable, int rows, const int *exclude, int b, int id_base) {
  GULON_REQUIRE(nullable || rows == 0 || offsets != nullptr, "row_offsets is null");
  if (offsets)
    for (int r = 0; r < rows; r++)
      GULON_REQUIRE(offsets[r] == offsets[r] && offsets[r] != -INFINITY,
                    "row_offsets[%d] = %g: NaN and -inf are not offsets", r, (double)offsets[r]);
  if (exclude)
    for (int q = 0; q < b; q++)
      GULON_REQUIRE(exclude[q] == -1 || (exclude[q] >= id_base && exclude[q] - id_base < rows),
                    "exclude[%d] = %d: expected -1 or a row in [%d, %d)", q, exclude[q], id_base, id_base + rows);
}

void check_offset_host(const float *offsets, int rows, const int *exclude, int b, int k_nn, int id_base) {
  GULON_REQUIRE(b >= 0, "batch size must be non-negative");
  GULON_UNSUPPORTED(k_nn < 1 || k_nn > GULON_MAX_K, "k_nn = %d outside [1, %d]", k_nn, GULON_MAX_K);
  check_rows_host(offsets, false, rows, exclude, b, id_base);
}

// (the passes, their query tiles and row chunks: exact_passes in exact.hpp, by knn_row_chunks())
void launch_offset_exact(const gulon_dataset *ds, int from, int until, OffsetWork &x, const float *d_q, int b, int k_nn,
                         const float *d_offsets, const int *d_exclude, int *out_idx, float *out_key, int *out_count,
                         hipStream_t st) {
  GULON_REQUIRE(b >= 0, "batch size must be non-negative");
  GULON_UNSUPPORTED(k_nn < 1 || k_nn > GULON_MAX_K, "k_nn = %d outside [1, %d]", k_nn, GULON_MAX_K);
  if (b == 0) return;
  GULON_REQUIRE(d_q != nullptr && d_offsets != nullptr && out_idx != nullptr && out_key != nullptr, "null argument");
  const int keff = k_nn + 1;
  exact_passes(d_q, b, ds->d, from, until, x.qt, st, [&](const ExactPass &p) {
    const size_t lists = (size_t)p.tiles * KNN_QT * p.nchunks * keff;
    x.pv.ensure(lists); x.pi.ensure(lists);
    hipLaunchKernelGGL(offset_exact_scan, dim3(p.tiles, p.nchunks), dim3(KNN_THREADS), 0, st, ds->x.p, ds->n, ds->d,
                       x.qt.p, d_offsets, d_exclude ? d_exclude + p.q0 : nullptr, p.nb, from, until, p.rows_per_chunk,
                       p.nchunks, keff, x.pv.p, x.pi.p);
    HIP_CHECK(hipGetLastError());
    launch_merge(x.pv.p, x.pi.p, p.nchunks, (long long)keff, (long long)p.nchunks * keff, p.nb, k_nn,
                 QueryOut::final_lists(out_idx, out_key, out_count, nullptr).from_query(p.q0, k_nn), st);
  });
}

}  // namespace gulon

using namespace gulon;

GULON_API int32_t gulon_index_query_offset_dev(gulon_index *idx, const float *d_queries, int32_t b, int32_t k_nn,
                                               int32_t from, int32_t until, const float *d_row_offsets,
                                               const int32_t *d_exclude, int32_t *d_out_idx, float *d_out_key,
                                               int32_t *d_out_count, void *stream) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    check_flat(idx, b, k_nn, from, until);
    std::lock_guard<std::mutex> work(idx->offset.mu);
    launch_offset_flat(idx, idx->offset, d_queries, b, k_nn, from, until, d_row_offsets, d_exclude, d_out_idx, d_out_key,
                       d_out_count, (hipStream_t)stream);
  });
}

GULON_API int32_t gulon_index_query_offset(gulon_index *idx, const float *queries, int32_t b, int32_t k_nn, int32_t from,
                                           int32_t until, const float *row_offsets, const int32_t *exclude,
                                           int32_t *out_idx, float *out_key, int32_t *out_count) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    check_flat(idx, b, k_nn, from, until);
    check_offset_host(row_offsets, idx->n, exclude, b, k_nn, idx->row_base);
    if (b == 0) return;
    GULON_REQUIRE(queries != nullptr && out_idx != nullptr && out_key != nullptr, "null argument");
    OffsetWork &x = idx->offset;
    std::lock_guard<std::mutex> work(x.mu);
    const hipStream_t st = nullptr;
    const size_t bk = (size_t)b * (size_t)k_nn;
    {
      std::lock_guard<std::mutex> lock(idx->mu);
      StreamOrder so(idx, st);   // the workspace may still be read by the last call, on another stream
      x.q.upload(queries, (size_t)b * idx->d, st);
      x.off.upload(row_offsets, (size_t)idx->n, st);
      x.off.ensure(1);   // (an index without rows: the scan still takes a pointer)
      if (exclude) x.ex.upload(exclude, (size_t)b, st);
      x.fi.ensure(bk); x.fd.ensure(bk); x.fc.ensure((size_t)b);
    }
    launch_offset_flat(idx, x, x.q.p, b, k_nn, from, until, x.off.p, exclude ? x.ex.p : nullptr, x.fi.p, x.fd.p, x.fc.p,
                       st);
    x.fi.download(out_idx, bk, st); x.fd.download(out_key, bk, st);
    if (out_count) x.fc.download(out_count, (size_t)b, st);
    HIP_CHECK(hipStreamSynchronize(st));
  });
}

GULON_API int32_t gulon_mean_similarity_dev(const float *d_dist_lists, const int32_t *d_counts, int32_t b, int32_t kin,
                                            int32_t K, float *d_out, void *stream) {
  return guarded([&] { launch_mean_similarity(d_dist_lists, d_counts, b, kin, K, d_out, (hipStream_t)stream); });
}

GULON_API int32_t gulon_mean_similarity(const float *dist_lists, const int32_t *counts, int32_t b, int32_t kin, int32_t K,
                                        float *out) {
  return guarded([&] {
    GULON_REQUIRE(b >= 0 && kin >= 1 && K >= 1, "expected: b >= 0, kin >= 1, K >= 1");
    if (b == 0) return;
    GULON_REQUIRE(dist_lists != nullptr && out != nullptr, "null argument");
    DevBuf<float> dd, dout((size_t)b);
    DevBuf<int> dc;
    dd.upload(dist_lists, (size_t)b * kin);
    if (counts) dc.upload(counts, (size_t)b);
    launch_mean_similarity(dd.p, counts ? dc.p : nullptr, b, kin, K, dout.p, nullptr);
    dout.download(out, (size_t)b);
    HIP_CHECK(hipStreamSynchronize(nullptr));
  });
}
