// The exact distance tile and what is built on it: the brute-force kNN (knn.hip), the exact index (exact.hip) and the
// exact 3CosMul scan (cosmul.hip) all compute their distances by exact_tile(); the exact index answers small k_nn and
// its fallbacks by knn.hip's single-pass / peeled driver, exact_knn_dev(); the offset and rank scans (offset.hip,
// rank.hip) walk their queries by exact_passes().
#pragma once
#include "table_scan.hpp"   // EXACT_SUB_BATCH

namespace gulon {

constexpr int KNN_QT = 16;       // queries per workgroup
constexpr int KNN_DT = 32;       // dims staged per step
constexpr int KNN_THREADS = 256; // 4 waves, lane = row

// Qt[tile][dim][KNN_QT]: the 16 query vectors of a workgroup transposed, so that one uniform (scalar) load of
// Qt[tile][dim] serves a wave.  transpose_queries (knn.hip) fills it with queries tile * 16 + u, zeros past B;
// cosmul_transpose (cosmul.hip) with the term vectors of 16 / E' questions.
__global__ void transpose_queries(const float *__restrict__ Q, int B, int d, int ntiles, float *__restrict__ Qt);

// One step of a KNN_THREADS workgroup: acc[q] = the squared L2 distance between query q of `qt` (one tile of Qt) and
// the row of slot `tid`; row_of(r) is the row of X that slot r holds, -1 -- or any row outside [0, n) -- for an empty
// slot (its acc is that of a zero row).  The rows are staged in the caller's xs[KNN_THREADS * (KNN_DT + 1)], KNN_DT
// dims at a time, lane = row.
//
// The order of operations is the contract with the JVM reference, MathUtils.distanceSq (MathUtils.scala:85-95):
// acc = 0; acc += (q_e - x_e) * (q_e - x_e) with e ascending, query minus row, every operation a binary32 rounding of
// its own (the library is built with -ffp-contract=off).
//
// All threads call.  Each staging step starts with a barrier (the readers of the last one are done, and so is
// whatever row_of reads) and has one between the stores and the sums; none follows the last sums.
template <class RowOf>
__device__ __forceinline__ void exact_tile(const float *__restrict__ X, int n, int d, const float *__restrict__ qt,
                                           float *xs, int tid, RowOf row_of, float (&acc)[KNN_QT]) {
#pragma unroll
  for (int q = 0; q < KNN_QT; q++) acc[q] = 0.f;
  for (int d0 = 0; d0 < d; d0 += KNN_DT) {
    __syncthreads();
    for (int e = tid; e < KNN_THREADS * KNN_DT; e += KNN_THREADS) {
      const int r = e / KNN_DT, c = e % KNN_DT;
      const int row = row_of(r), dim = d0 + c;
      // (one unsigned compare, and then an unsigned product: what the staging loop cost before it was shared)
      const bool in = (unsigned)row < (unsigned)n && dim < d;
      xs[r * (KNN_DT + 1) + c] = in ? X[(size_t)(unsigned)row * (unsigned)d + dim] : 0.f;
    }
    __syncthreads();
    const int dl = min(KNN_DT, d - d0);
    for (int c = 0; c < dl; c++) {
      const float x = xs[tid * (KNN_DT + 1) + c];
      const float *qv = qt + (size_t)(d0 + c) * KNN_QT;
#pragma unroll
      for (int q = 0; q < KNN_QT; q++) {
        const float dx = qv[q] - x;   // dx = y(i) - x(i), y = query (MathUtils.scala:90)
        acc[q] += dx * dx;
      }
    }
  }
}

// The 256-row groups that cover [from, until), from rounded down to a group, and their split into row chunks for
// about `want` workgroups per query tile: as many groups in every chunk, no empty chunk.
struct RowChunks { int nchunks, groups_per_chunk; };
inline int row_groups(int from, int until) {
  return std::max(1, ceil_div(until - from / KNN_THREADS * KNN_THREADS, KNN_THREADS));
}
inline RowChunks split_groups(int groups, int want) {
  const int per = ceil_div(groups, std::min(std::max(want, 1), groups));
  return {ceil_div(groups, per), per};
}
// knn_kernel's and cosmul_exact_scan's grids: about 2048 workgroups over `tiles` query tiles
inline RowChunks knn_row_chunks(int from, int until, int tiles) {
  return split_groups(row_groups(from, until), ceil_div(2048, tiles));
}

// The passes of a scan in knn_kernel's geometry over the b >= 1 queries at d_q [b][d], rows [from, until):
// EXACT_SUB_BATCH queries each, their Qt into `qt` (transpose_queries) on `st`, then pass(p) -- the caller's buffers,
// kernels and tail for queries [q0, q0 + nb), `tiles` query tiles by `nchunks` row chunks of `rows_per_chunk` rows.
struct ExactPass { int q0, nb, tiles, nchunks, rows_per_chunk; };
template <class Pass>
void exact_passes(const float *d_q, int b, int d, int from, int until, DevBuf<float> &qt, hipStream_t st, Pass pass) {
  for (int q0 = 0; q0 < b; q0 += EXACT_SUB_BATCH) {
    const int nb = std::min(EXACT_SUB_BATCH, b - q0), tiles = ceil_div(nb, KNN_QT);
    const RowChunks ch = knn_row_chunks(from, until, tiles);
    const long long tq = (long long)tiles * d * KNN_QT;
    qt.ensure((size_t)tq);
    hipLaunchKernelGGL(transpose_queries, dim3(ceil_div(tq, 256)), dim3(256), 0, st, d_q + (size_t)q0 * d, nb, d, tiles,
                       qt.p);
    pass(ExactPass{q0, nb, tiles, ch.nchunks, ch.groups_per_chunk * KNN_THREADS});
  }
}

// gulon_exact_knn's device work, all on `st`: b >= 1 queries at d_q against rows [from, until) of ds, from < until,
// 1 <= K <= GULON_MAX_K_PEELED.  K <= GULON_MAX_K: one knn_kernel pass and launch_merge; larger K peeled, 64 entries
// per pass behind the lower bound (lbv, lbi) of the last.  Outputs are device pointers [b][K] / [b], none null.  The
// scratch grows on demand and is the caller's to keep between calls.
struct KnnScratch {
  DevBuf<float> qt, pv, accv, tv, lbv;
  DevBuf<int> pi, acci, ti, lbi;
};
void exact_knn_dev(const gulon_dataset *ds, int from, int until, const float *d_q, int b, int K, KnnScratch &s, int *oi,
                   float *od, int *oc, int *of, hipStream_t st);

}  // namespace gulon
