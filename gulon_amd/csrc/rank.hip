// Rank queries: the counting twin of the offset query (offset.hip).  Candidates, keys and
// order are the offset query's -- per query q and row r of the handle's range, d the handle's own distance bits,
// t = d + offsets[r] in one binary32 addition (no offsets: + 0), r a candidate if and only if t is finite and its id is
// not exclude[q], the order (t ascending, id ascending) -- but the answer is one position per query, not a list: how many
// candidates come strictly before the best row of the query's gold list.  Three stages per pass, all on one stream:
//
//   gold keys     the t of every (query, gold row) pair, in the bits the scan forms for that row, and per query the
//                 first pair by (t, id) among the candidates: (key*, row*), or (+inf, -1) where no gold row is one.
//                 exact index: rank_exact_gold -- exact_tile (exact.hpp) over the gold rows of the tile's 16 queries,
//                 every slot keeps the sum of the query that owns it.  flat index: rank_flat_gold -- a wave per query,
//                 a lane per gold row, the row's code words gathered and its entries of the query's Index.prepareQuery
//                 table summed quantizer 0 first from 0.f, as the scan sums them
//   counting      rank_exact_scan: knn.hip's knn_kernel geometry (16 queries per workgroup, lane = row, exact_tile, one
//                 offset load per 256-row step, knn_row_chunks).  rank_flat_scan<E, VEC>: the flat table scan
//                 (table_scan.hpp) in the flat offset scan's geometry, one offset load per row for the E queries; the
//                 slots, the grid and the passes by offset.hpp.  Per query (key*, row*) and the excluded id are
//                 wave-uniform; per row  valid = in range && finite(t) && id != ex,
//                 ahead = valid && (t < key* || (t == key* && id < row*)), and two scalar counters advance by the
//                 population of the two ballots.  No list, no merge, no atomics; one LDS reduction over the waves
//                 gives one (ahead, total) pair per (query, row chunk)
//   finish        rank_finish: the chunk pairs summed in int32; rank, row, key, total out, -1 / -1 / +inf without a
//                 best gold row
#include "rank.hpp"
#include "exact.hpp"

namespace gulon {
namespace {

// The lanes of a wave whose (t, id) comes before the wave-uniform (key, gold) in the order (t ascending, id ascending):
// four compares, their masks combined by scalar instructions -- no branch, nothing per lane but the compares.
__device__ __forceinline__ unsigned long long ahead_mask(float t, int id, float key, int gold) {
  return __ballot(t < key) | (__ballot(t == key) & __ballot(id < gold));
}

// ---- exact index ------------------------------------------------------------------------------------------------------

// One workgroup per query tile.  The gold rows of the tile's queries are consecutive in gold_rows (CSR): slot s of a
// 256-slot step holds pair g0 + s, exact_tile sums the 16 queries against it and the slot keeps the sum of its own
// query.  gk[g] = t of pair g, +inf where the pair is no candidate.  Then thread u < 16 walks the pairs of query u in
// list order and keeps the first by (t, row).
__global__ __launch_bounds__(KNN_THREADS) void rank_exact_gold(const float *__restrict__ X, int n, int d,
                                                               const float *__restrict__ Qt,
                                                               const float *__restrict__ offsets,
                                                               const int *__restrict__ exclude, int b, int row_from,
                                                               int row_until, const int *__restrict__ gold_off,
                                                               const int *__restrict__ gold_rows, float *gk,
                                                               float *__restrict__ best_key, int *__restrict__ best_row) {
  __shared__ float xs[KNN_THREADS * (KNN_DT + 1)];
  __shared__ int goff[KNN_QT + 1];
  const int tid = threadIdx.x, tile = blockIdx.x;
  const float *qt = Qt + (size_t)tile * d * KNN_QT;
  const int q0 = tile * KNN_QT;
  if (tid <= KNN_QT) goff[tid] = gold_off[min(q0 + tid, b)];
  __syncthreads();
  const int g0 = goff[0], g1 = goff[KNN_QT];
  for (int base = g0; base < g1; base += KNN_THREADS) {
    float acc[KNN_QT];
    exact_tile(X, n, d, qt, xs, tid, [&](int r) { return base + r < g1 ? gold_rows[base + r] : -1; }, acc);
    const int g = base + tid;
    if (g < g1) {
      int own = 0;   // the query that owns pair g: the last u with goff[u] <= g
#pragma unroll
      for (int u = 1; u < KNN_QT; u++) own += goff[u] <= g;
      float dist = acc[0];
#pragma unroll
      for (int u = 1; u < KNN_QT; u++) dist = own == u ? acc[u] : dist;
      const int row = gold_rows[g];
      const bool in = row >= row_from && row < row_until;
      const float off = (in && offsets != nullptr) ? offsets[row] : 0.f;
      const float t = __fadd_rn(dist, off);
      const int ex = exclude != nullptr ? exclude[q0 + own] : -1;
      gk[g] = (in && finite_key(t) && row != ex) ? t : INFINITY;
    }
  }
  __syncthreads();   // the keys of the tile's pairs are written (by this workgroup: visible after the barrier)
  if (tid < KNN_QT && q0 + tid < b) {
    float bk = INFINITY;
    int br = -1;
    for (int g = goff[tid]; g < goff[tid + 1]; g++) {
      const float t = gk[g];
      const int row = gold_rows[g];
      if (finite_key(t) && (br < 0 || t < bk || (t == bk && row < br))) { bk = t; br = row; }
    }
    best_key[q0 + tid] = bk;
    best_row[q0 + tid] = br;
  }
}

// part[(query * nchunks + chunk) * 2 + {0, 1}] = the candidates of the chunk ahead of (key*, row*), the candidates
__global__ __launch_bounds__(KNN_THREADS) void rank_exact_scan(const float *__restrict__ X, int n, int d,
                                                               const float *__restrict__ Qt,
                                                               const float *__restrict__ offsets,
                                                               const int *__restrict__ exclude,
                                                               const float *__restrict__ best_key,
                                                               const int *__restrict__ best_row, int b, int row_from,
                                                               int row_until, int rows_per_chunk, int nchunks,
                                                               int *__restrict__ part) {
  constexpr int NW = KNN_THREADS / 64;
  __shared__ float xs[KNN_THREADS * (KNN_DT + 1)];
  __shared__ int sc[NW][KNN_QT][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tile = blockIdx.x, chunk = blockIdx.y;
  const float *qt = Qt + (size_t)tile * d * KNN_QT;

  float key[KNN_QT];
  int gold[KNN_QT], ex[KNN_QT], ahead[KNN_QT], total[KNN_QT];
#pragma unroll
  for (int q = 0; q < KNN_QT; q++) {
    const int qg = tile * KNN_QT + q;
    key[q] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(qg < b ? best_key[qg] : INFINITY)));
    gold[q] = __builtin_amdgcn_readfirstlane(qg < b ? best_row[qg] : -1);
    ex[q] = __builtin_amdgcn_readfirstlane((exclude != nullptr && qg < b) ? exclude[qg] : -1);
    ahead[q] = 0; total[q] = 0;
  }

  const int r0 = (row_from / KNN_THREADS) * KNN_THREADS + chunk * rows_per_chunk;
  const int r1 = min(row_until, r0 + rows_per_chunk);
  for (int base = r0; base < r1; base += KNN_THREADS) {
    float acc[KNN_QT];
    exact_tile(X, n, d, qt, xs, tid, [&](int r) { return base + r; }, acc);
    const int row = base + tid;
    const bool in = row >= row_from && row < row_until;
    const float off = (in && offsets != nullptr) ? offsets[row] : 0.f;
    const unsigned long long min = __ballot(in);
#pragma unroll
    for (int q = 0; q < KNN_QT; q++) {
      const float t = __fadd_rn(acc[q], off);
      const unsigned long long valid = min & __ballot(finite_key(t)) & __ballot(row != ex[q]);
      ahead[q] += __popcll(valid & ahead_mask(t, row, key[q], gold[q]));
      total[q] += __popcll(valid);
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < KNN_QT; q++) { sc[wave][q][0] = ahead[q]; sc[wave][q][1] = total[q]; }
  }
  __syncthreads();
  if (tid < KNN_QT * 2) {   // (part holds ceil(b / 16) * 16 queries)
    int sum = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) sum += sc[w][tid >> 1][tid & 1];
    part[((size_t)(tile * KNN_QT + (tid >> 1)) * nchunks + chunk) * 2 + (tid & 1)] = sum;
  }
}

// ---- flat index -------------------------------------------------------------------------------------------------------

// One wave per query of the pass, lane l its gold rows l, l + 64, ...: the row's code words gathered, acc += T[j][code_j]
// with j ascending over the m_pad quantizers from 0.f -- the sum the scan forms for that row -- then the first pair by
// (t, id) over the lanes.
template <int VEC>
__global__ __launch_bounds__(256) void rank_flat_gold(const uint8_t *__restrict__ codes, int ng, int m_pad,
                                                      const float *__restrict__ tables,
                                                      const float *__restrict__ offsets,
                                                      const int *__restrict__ exclude, int b, int row_from,
                                                      int row_until, int row_base, const int *__restrict__ gold_off,
                                                      const int *__restrict__ gold_rows, float *__restrict__ best_key,
                                                      int *__restrict__ best_row) {
  using Word = typename CodeWord<VEC>::type;
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
  if (q >= b) return;   // (whole waves)
  const float *tq = tables + (size_t)q * m_pad * 256;
  const Word *cw = reinterpret_cast<const Word *>(codes);
  const int ex = exclude != nullptr ? exclude[q] : -1;
  float bk = INFINITY;
  int br = INT_MAX;
  for (int g = gold_off[q] + lane; g < gold_off[q + 1]; g += 64) {
    const int id = gold_rows[g], row = id - row_base;
    if (row < row_from || row >= row_until) continue;
    float acc = 0.f;
    const Word *p = cw + ((size_t)(row >> 6) * ng) * 64 + (row & 63);
    for (int w = 0; w < ng; w++) {
      const Word word = p[(size_t)w * 64];
      for (int c = 0; c < VEC; c++) acc += tq[(w * VEC + c) * 256 + code_byte<VEC>(word, c)];
    }
    const float t = __fadd_rn(acc, offsets != nullptr ? offsets[row] : 0.f);
    if (finite_key(t) && id != ex && (t < bk || (t == bk && id < br))) { bk = t; br = id; }
  }
  for (int s = 32; s >= 1; s >>= 1) {
    const float ok = __shfl_xor(bk, s);
    const int orow = __shfl_xor(br, s);
    if (ok < bk || (ok == bk && orow < br)) { bk = ok; br = orow; }
  }
  if (lane == 0) {
    best_key[q] = bk;
    best_row[q] = br == INT_MAX ? -1 : br;
  }
}

// A workgroup is (E query slots, row chunk), as in the flat offset scan: slot t is query blockIdx.x * E + t, its table in
// LDS (table_scan.hpp); the slots past the batch hold zero tables and their counters are not written.
template <int E, int VEC>
__global__ __launch_bounds__(TABLE_SCAN_THREADS) void rank_flat_scan(
    const uint8_t *__restrict__ codes, int ng, int m_pad, const float *__restrict__ tables,
    const float *__restrict__ offsets, const int *__restrict__ exclude, const float *__restrict__ best_key,
    const int *__restrict__ best_row, int b, int row_from, int row_until, int row_base, int rb_begin, int rb_end,
    int rb_per_chunk, int nchunks, int *__restrict__ part) {
  constexpr int NW = TABLE_SCAN_THREADS / 64;
  extern __shared__ float4 lds4[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q0 = blockIdx.x * E, chunk = blockIdx.y;
  const int tab = m_pad * 256;
  const int nq = min(E, b - q0);   // live slots (uniform over the workgroup)
  stage_tables(lds4, tables + (size_t)q0 * tab, tab, nq, E, tid);

  float key[E];
  int gold[E], ex[E], ahead[E], total[E];
#pragma unroll
  for (int t = 0; t < E; t++) {
    key[t] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(t < nq ? best_key[q0 + t] : INFINITY)));
    gold[t] = __builtin_amdgcn_readfirstlane(t < nq ? best_row[q0 + t] : -1);
    ex[t] = __builtin_amdgcn_readfirstlane((exclude != nullptr && t < nq) ? exclude[q0 + t] : -1);
    ahead[t] = 0; total[t] = 0;
  }

  const int rb0 = rb_begin + chunk * rb_per_chunk, rb1 = min(rb_end, rb0 + rb_per_chunk);
  table_scan_rows<E, VEC>(codes, ng, tab, reinterpret_cast<const float *>(lds4), rb0, rb1, lane, wave,
                          [&](int rb, const float (&acc)[E]) {
    const int row = rb * 64 + lane;
    const bool in = row >= row_from && row < row_until;
    const float off = (in && offsets != nullptr) ? offsets[row] : 0.f;
    const int id = row + row_base;
    const unsigned long long min = __ballot(in);
#pragma unroll
    for (int t = 0; t < E; t++) {
      const float k = __fadd_rn(acc[t], off);
      const unsigned long long valid = min & __ballot(finite_key(k)) & __ballot(id != ex[t]);
      ahead[t] += __popcll(valid & ahead_mask(k, id, key[t], gold[t]));
      total[t] += __popcll(valid);
    }
  });
  __syncthreads();   // every wave is done with the tables: their LDS takes the waves' counters [NW][E][2]
  int *sc = reinterpret_cast<int *>(lds4);
  if (lane == 0) {
#pragma unroll
    for (int t = 0; t < E; t++) { sc[(wave * E + t) * 2] = ahead[t]; sc[(wave * E + t) * 2 + 1] = total[t]; }
  }
  __syncthreads();
  if (tid < nq * 2) {
    int sum = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) sum += sc[w * E * 2 + tid];
    part[((size_t)(q0 + (tid >> 1)) * nchunks + chunk) * 2 + (tid & 1)] = sum;
  }
}

// ---- finish -------------------------------------------------------------------------------------------------------------

__global__ void rank_finish(const int *__restrict__ part, int nchunks, const float *__restrict__ best_key,
                            const int *__restrict__ best_row, int b, int *__restrict__ out_rank,
                            int *__restrict__ out_row, float *__restrict__ out_key, int *__restrict__ out_total) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= b) return;
  int ahead = 0, total = 0;
  for (int c = 0; c < nchunks; c++) {
    ahead += part[((size_t)q * nchunks + c) * 2];
    total += part[((size_t)q * nchunks + c) * 2 + 1];
  }
  const int row = best_row[q];
  out_rank[q] = row < 0 ? -1 : ahead;
  out_row[q] = row < 0 ? -1 : row;
  out_key[q] = row < 0 ? INFINITY : best_key[q];
  if (out_total != nullptr) out_total[q] = total;
}

void launch_finish(const RankWork &x, int nchunks, int nb, int *out_rank, int *out_row, float *out_key, int *out_total,
                   hipStream_t st) {
  hipLaunchKernelGGL(rank_finish, dim3(ceil_div(nb, 256)), dim3(256), 0, st, x.part.p, nchunks, x.bk.p, x.br.p, nb,
                     out_rank, out_row, out_key, out_total);
  HIP_CHECK(hipGetLastError());
}

}  // namespace

int check_rank_host(const float *offsets, int rows, const int *exclude, const int *gold_offsets, const int *gold_rows,
                    int b, int id_base) {
  GULON_REQUIRE(b >= 0, "batch size must be non-negative");
  check_rows_host(offsets, true, rows, exclude, b, id_base);
  GULON_REQUIRE(gold_offsets != nullptr, "gold_offsets is null");
  GULON_REQUIRE(gold_offsets[0] == 0, "gold_offsets[0] = %d: expected 0", gold_offsets[0]);
  for (int q = 0; q < b; q++)
    GULON_REQUIRE(gold_offsets[q + 1] >= gold_offsets[q], "gold_offsets[%d] = %d < gold_offsets[%d] = %d: expected "
                  "a non-decreasing array", q + 1, gold_offsets[q + 1], q, gold_offsets[q]);
  const int gold = gold_offsets[b];
  GULON_REQUIRE(gold == 0 || gold_rows != nullptr, "gold_rows is null");
  for (int g = 0; g < gold; g++)
    GULON_REQUIRE(gold_rows[g] >= id_base && gold_rows[g] - id_base < rows, "gold_rows[%d] = %d: expected a row in [%d, %d)",
                  g, gold_rows[g], id_base, id_base + rows);
  return gold;
}

// (the passes, their query tiles and row chunks: exact_passes in exact.hpp, by knn_row_chunks())
void launch_rank_exact(const gulon_dataset *ds, int from, int until, RankWork &x, const float *d_q, int b,
                       const float *d_offsets, const int *d_exclude, const int *d_gold_off, const int *d_gold_rows,
                       int gold, int *out_rank, int *out_row, float *out_key, int *out_total, hipStream_t st) {
  GULON_REQUIRE(b >= 0 && gold >= 0, "batch size must be non-negative");
  if (b == 0) return;
  GULON_REQUIRE(d_q != nullptr && d_gold_off != nullptr && out_rank != nullptr && out_row != nullptr &&
                out_key != nullptr, "null argument");
  x.gk.ensure((size_t)std::max(gold, 1));
  exact_passes(d_q, b, ds->d, from, until, x.qt, st, [&](const ExactPass &p) {
    const size_t bp = (size_t)p.tiles * KNN_QT;
    x.bk.ensure(bp); x.br.ensure(bp);
    x.part.ensure(bp * p.nchunks * 2);
    const int *ex = d_exclude ? d_exclude + p.q0 : nullptr;
    hipLaunchKernelGGL(rank_exact_gold, dim3(p.tiles), dim3(KNN_THREADS), 0, st, ds->x.p, ds->n, ds->d, x.qt.p,
                       d_offsets, ex, p.nb, from, until, d_gold_off + p.q0, d_gold_rows, x.gk.p, x.bk.p, x.br.p);
    hipLaunchKernelGGL(rank_exact_scan, dim3(p.tiles, p.nchunks), dim3(KNN_THREADS), 0, st, ds->x.p, ds->n, ds->d,
                       x.qt.p, d_offsets, ex, x.bk.p, x.br.p, p.nb, from, until, p.rows_per_chunk, p.nchunks, x.part.p);
    HIP_CHECK(hipGetLastError());
    launch_finish(x, p.nchunks, p.nb, out_rank + p.q0, out_row + p.q0, out_key + p.q0,
                  out_total ? out_total + p.q0 : nullptr, st);
  });
}

// The passes by flat_passes (offset.hpp): the slots by offset_flat_max_e(), the grid by offset_flat_shape(), the tables by
// launch_build_tables(), under the handle's mutex and one StreamOrder.
void launch_rank_flat(gulon_index *ix, RankWork &x, const float *d_q, int b, int from, int until, const float *d_off,
                      const int *d_ex, const int *d_goff, const int *d_grows, int *out_rank, int *out_row,
                      float *out_key, int *out_total, hipStream_t st) {
  if (b == 0) return;
  GULON_REQUIRE(d_q != nullptr && d_goff != nullptr && out_rank != nullptr && out_row != nullptr && out_key != nullptr,
                "null argument");
  flat_passes(ix, x.tables, d_q, b, from, until, st, [&](int q0, int nb, int E, const FlatShape &s) {
    x.bk.ensure((size_t)nb); x.br.ensure((size_t)nb);
    x.part.ensure((size_t)nb * s.nchunks * 2);
    const int *ex = d_ex ? d_ex + q0 : nullptr;
    dispatch_e_vec(E, ix->vec, [&](auto e, auto vec) {
      hipLaunchKernelGGL(rank_flat_gold<decltype(vec)::value>, dim3(ceil_div(nb, 4)), dim3(256), 0, st, ix->codes.p,
                         ix->ng, ix->m_pad, x.tables.p, d_off, ex, nb, from, until, ix->row_base, d_goff + q0, d_grows,
                         x.bk.p, x.br.p);
      HIP_CHECK(hipGetLastError());
      const auto scan = rank_flat_scan<decltype(e)::value, decltype(vec)::value>;
      const size_t lds_bytes = (size_t)e * flat_slot_bytes(ix->m_pad);
      HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(scan), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds_bytes));
      hipLaunchKernelGGL(scan, dim3(ceil_div(nb, e), s.nchunks), dim3(TABLE_SCAN_THREADS), lds_bytes, st, ix->codes.p,
                         ix->ng, ix->m_pad, x.tables.p, d_off, ex, x.bk.p, x.br.p, nb, from, until, ix->row_base, from / 64,
                         ceil_div(until, 64), s.rb_per_chunk, s.nchunks, x.part.p);
      HIP_CHECK(hipGetLastError());
    });
    launch_finish(x, s.nchunks, nb, out_rank + q0, out_row + q0, out_key + q0, out_total ? out_total + q0 : nullptr, st);
  });
}

}  // namespace gulon

using namespace gulon;

GULON_API int32_t gulon_index_query_rank(gulon_index *idx, const float *queries, int32_t b, int32_t from, int32_t until,
                                         const float *row_offsets, const int32_t *exclude, const int32_t *gold_offsets,
                                         const int32_t *gold_rows, int32_t *out_rank, int32_t *out_row, float *out_key,
                                         int32_t *out_total) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    check_flat(idx, b, 1, from, until);
    if (b == 0) return;
    const int gold = check_rank_host(row_offsets, idx->n, exclude, gold_offsets, gold_rows, b, idx->row_base);
    GULON_REQUIRE(queries != nullptr && out_rank != nullptr && out_row != nullptr && out_key != nullptr, "null argument");
    RankWork &x = idx->rank;
    std::lock_guard<std::mutex> work(x.mu);
    const hipStream_t st = nullptr;
    {
      std::lock_guard<std::mutex> lock(idx->mu);
      StreamOrder so(idx, st);   // the workspace may still be read by the last call, on another stream
      x.q.upload(queries, (size_t)b * idx->d, st);
      if (row_offsets) x.off.upload(row_offsets, (size_t)idx->n, st);
      if (exclude) x.ex.upload(exclude, (size_t)b, st);
      x.goff.upload(gold_offsets, (size_t)b + 1, st);
      x.grows.upload(gold_rows, (size_t)gold, st);
      x.grows.ensure(1);
      x.frank.ensure((size_t)b); x.frow.ensure((size_t)b); x.fk.ensure((size_t)b); x.ftotal.ensure((size_t)b);
    }
    launch_rank_flat(idx, x, x.q.p, b, from, until, row_offsets ? x.off.p : nullptr, exclude ? x.ex.p : nullptr,
                     x.goff.p, x.grows.p, x.frank.p, x.frow.p, x.fk.p, x.ftotal.p, st);
    x.frank.download(out_rank, (size_t)b, st); x.frow.download(out_row, (size_t)b, st);
    x.fk.download(out_key, (size_t)b, st);
    if (out_total) x.ftotal.download(out_total, (size_t)b, st);
    HIP_CHECK(hipStreamSynchronize(st));
  });
}
