// The log-sum-exp scan: the twin of the rank queries' counting scan on the exact index (rank.hip;
// DESIGN.md 9ab), with a binary64 sum per query where that kernel keeps two counters.  Per query q and row r of the
// handle's range, d the handle's own distance bits (exact_tile, exact.hpp): r is a term if and only if d is finite and
// r is not exclude[q]; z = (double)d * zscale, e = exp(z), S_q = the sum of e over the terms, L_q = log(S_q).  With
// zscale = -beta / 2 and the rows of the source language's unit vectors, (2 / beta) * L is the offset of the inverted
// softmax (Smith et al. 2017) for the target row that was the query.  Two stages per pass, on one stream:
//
//   scan     logsumexp_exact_scan: knn.hip's knn_kernel geometry (16 queries per workgroup, lane = row, exact_tile,
//            knn_row_chunks).  Per lane 16 binary64 accumulators advance by one term per 256-row step, steps ascending;
//            a lane that holds no term adds +0 (a select after the exp, no branch).  The excluded id is wave-uniform
//            and the terms are counted by ballot and popcount.  Then the lanes of a wave by an xor butterfly, 32 down to
//            1, the waves in wave order through LDS: one sum and one count per (query, row chunk), no atomics
//   finish   logsumexp_finish: the chunk sums added chunk ascending, the log, the counts summed in int32
#include "logsumexp.hpp"

namespace gulon {
namespace {

// part_sum / part_terms[(tile * 16 + u) * nchunks + chunk]: query tile * 16 + u against the rows of the chunk.  The
// slots past the batch are not written.
__global__ __launch_bounds__(KNN_THREADS) void logsumexp_exact_scan(const float *__restrict__ X, int n, int d,
                                                                    const float *__restrict__ Qt,
                                                                    const int *__restrict__ exclude, int b,
                                                                    int row_from, int row_until, int rows_per_chunk,
                                                                    int nchunks, double zscale,
                                                                    double *__restrict__ part_sum,
                                                                    int *__restrict__ part_terms) {
  constexpr int NW = KNN_THREADS / 64;
  __shared__ float xs[KNN_THREADS * (KNN_DT + 1)];
  __shared__ double sd[NW][KNN_QT];
  __shared__ int sc[NW][KNN_QT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tile = blockIdx.x, chunk = blockIdx.y;
  const float *qt = Qt + (size_t)tile * d * KNN_QT;

  int ex[KNN_QT], terms[KNN_QT];
  double sum[KNN_QT];
#pragma unroll
  for (int q = 0; q < KNN_QT; q++) {
    const int qg = tile * KNN_QT + q;
    ex[q] = __builtin_amdgcn_readfirstlane((exclude != nullptr && qg < b) ? exclude[qg] : -1);
    terms[q] = 0; sum[q] = 0.0;
  }

  const int r0 = (row_from / KNN_THREADS) * KNN_THREADS + chunk * rows_per_chunk;
  const int r1 = min(row_until, r0 + rows_per_chunk);
  for (int base = r0; base < r1; base += KNN_THREADS) {
    float acc[KNN_QT];
    exact_tile(X, n, d, qt, xs, tid, [&](int r) { return base + r; }, acc);
    const int row = base + tid;
    const bool in = row >= row_from && row < row_until;
#pragma unroll
    for (int q = 0; q < KNN_QT; q++) {
      const bool term = in && finite_key(acc[q]) && row != ex[q];
      const double e = exp((double)acc[q] * zscale);
      sum[q] += term ? e : 0.0;
      terms[q] += __popcll(__ballot(term));
    }
  }
#pragma unroll
  for (int q = 0; q < KNN_QT; q++) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) sum[q] += __shfl_xor(sum[q], s);
  }
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < KNN_QT; q++) { sd[wave][q] = sum[q]; sc[wave][q] = terms[q]; }
  }
  __syncthreads();
  if (tid < KNN_QT && tile * KNN_QT + tid < b) {
    double s = sd[0][tid];
    int c = sc[0][tid];
#pragma unroll
    for (int w = 1; w < NW; w++) { s += sd[w][tid]; c += sc[w][tid]; }
    const size_t at = (size_t)(tile * KNN_QT + tid) * nchunks + chunk;
    part_sum[at] = s;
    part_terms[at] = c;
  }
}

__global__ void logsumexp_finish(const double *__restrict__ part_sum, const int *__restrict__ part_terms, int nchunks,
                                 int b, double *__restrict__ out_lse, int *__restrict__ out_terms) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= b) return;
  double s = part_sum[(size_t)q * nchunks];
  int c = part_terms[(size_t)q * nchunks];
  for (int k = 1; k < nchunks; k++) {
    s += part_sum[(size_t)q * nchunks + k];
    c += part_terms[(size_t)q * nchunks + k];
  }
  out_lse[q] = log(s);   // log(+0) = -inf: no term, or every term underflowed
  out_terms[q] = c;
}

}  // namespace

// (the passes, their query tiles and row chunks: exact_passes in exact.hpp, by knn_row_chunks())
void launch_logsumexp_exact(const gulon_dataset *ds, int from, int until, LseWork &x, const float *d_q, int b,
                            double zscale, const int *d_exclude, double *out_lse, int *out_terms, hipStream_t st) {
  GULON_REQUIRE(b >= 0, "batch size must be non-negative");
  if (b == 0) return;
  GULON_REQUIRE(d_q != nullptr && out_lse != nullptr && out_terms != nullptr, "null argument");
  exact_passes(d_q, b, ds->d, from, until, x.qt, st, [&](const ExactPass &p) {
    const size_t slots = (size_t)p.tiles * KNN_QT * p.nchunks;
    x.part.ensure(slots); x.cnt.ensure(slots);
    hipLaunchKernelGGL(logsumexp_exact_scan, dim3(p.tiles, p.nchunks), dim3(KNN_THREADS), 0, st, ds->x.p, ds->n, ds->d,
                       x.qt.p, d_exclude ? d_exclude + p.q0 : nullptr, p.nb, from, until, p.rows_per_chunk, p.nchunks,
                       zscale, x.part.p, x.cnt.p);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(logsumexp_finish, dim3(ceil_div(p.nb, 256)), dim3(256), 0, st, x.part.p, x.cnt.p, p.nchunks, p.nb,
                       out_lse + p.q0, out_terms + p.q0);
    HIP_CHECK(hipGetLastError());
  });
}

}  // namespace gulon
