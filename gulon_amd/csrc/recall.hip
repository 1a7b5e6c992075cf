// Tests.recallOf (Tests.scala:18-41), the per-batch part: for every query the exact MathUtils.distanceSq
// (MathUtils.scala:85-95) to each returned row of the dataset and, for every k of the caller's list, the number of
// entries among the first k whose distance is <= that k's cutoff.  One workgroup per query, its rows gathered through
// row_tile.hpp's tile; the B x max_k distances stay on the device unless the caller asks for them.
#include "row_tile.hpp"

namespace gulon {

constexpr int RC_MAX_KS = 16;

// The rows are gathered and summed by tile_distance_sq (row_tile.hpp), VEC4 as there.
template <bool VEC4>
__global__ __launch_bounds__(RC_THREADS) void recall_counts_kernel(
    const float *__restrict__ X, int n, int d, const float *__restrict__ Q, const int *__restrict__ rows, int max_k,
    const int *__restrict__ ks, int nks, const float *__restrict__ cutoffs, int *__restrict__ out_tp,
    float *__restrict__ out_dist, int *__restrict__ bad_row) {
  constexpr int NW = RC_THREADS / 64;
  __shared__ RowTile tile;
  __shared__ int sc[NW * RC_MAX_KS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = blockIdx.x;
  const float *query = Q + (size_t)q * d;
  const int *qrows = rows + (size_t)q * max_k;

  int kk[RC_MAX_KS], cnt[RC_MAX_KS];
  float cut[RC_MAX_KS];
#pragma unroll
  for (int j = 0; j < RC_MAX_KS; j++) {
    kk[j] = j < nks ? ks[j] : 0;
    cut[j] = j < nks ? cutoffs[(size_t)q * nks + j] : 0.f;
    cnt[j] = 0;
  }

  const bool whole_query = d <= RC_QS;
  for (int p0 = 0; p0 < max_k; p0 += RC_THREADS) {
    const int p = p0 + tid;
    int row = p < max_k ? qrows[p] : -1;
    if (row >= n) { *bad_row = row; row = -1; }   // any one offender is reported; the entry is not read
    const float acc = tile_distance_sq<VEC4>(tile, X, d, query, row, !whole_query || p0 == 0);
    const bool present = row >= 0;
    if (out_dist != nullptr && p < max_k) out_dist[(size_t)q * max_k + p] = present ? acc : 0.f;
#pragma unroll
    for (int j = 0; j < RC_MAX_KS; j++)                       // NaN <= cutoff is false: a NaN distance is a miss
      cnt[j] += __popcll(__ballot(present && p < kk[j] && acc <= cut[j]));
  }
#pragma unroll
  for (int j = 0; j < RC_MAX_KS; j++)
    if (lane == 0) sc[wave * RC_MAX_KS + j] = cnt[j];
  __syncthreads();
  if (tid < nks) {
    int s = 0;
    for (int w = 0; w < NW; w++) s += sc[w * RC_MAX_KS + tid];
    out_tp[(size_t)q * nks + tid] = s;
  }
}

}  // namespace gulon

using namespace gulon;

GULON_API int32_t gulon_recall_counts(const gulon_dataset *ds, const float *queries, int32_t b, const int32_t *rows,
                                      int32_t max_k, const int32_t *ks, int32_t nks, const float *cutoffs,
                                      int32_t *out_tp, float *out_dist) {
  return guarded([&] {
    GULON_REQUIRE(ds != nullptr, "dataset is null");
    GULON_REQUIRE(b >= 0 && max_k >= 0 && nks >= 0 && nks <= RC_MAX_KS, "bad arguments b=%d max_k=%d nks=%d (<= %d)", b,
                  max_k, nks, RC_MAX_KS);
    GULON_UNSUPPORTED(max_k > GULON_MAX_K_PEELED, "max_k = %d > %d", max_k, GULON_MAX_K_PEELED);
    GULON_REQUIRE(nks == 0 || ks != nullptr, "ks is null");
    for (int j = 0; j < nks; j++)
      GULON_REQUIRE(ks[j] >= 1 && ks[j] <= max_k && (j == 0 || ks[j] > ks[j - 1]),
                    "ks must ascend within [1, max_k = %d]: ks[%d] = %d", max_k, j, ks[j]);
    if (b == 0 || (nks == 0 && out_dist == nullptr)) return;
    GULON_REQUIRE(queries != nullptr && (rows != nullptr || max_k == 0) && (nks == 0 || (cutoffs && out_tp)),
                  "null argument");
    const int d = ds->d;
    const size_t bk = (size_t)b * max_k, bn = (size_t)b * nks;
    DevBuf<float> dq, dcut, dout(out_dist ? bk : 0);
    DevBuf<int> dr, dks, dtp(std::max<size_t>(bn, 1)), bad(1);
    dq.upload(queries, (size_t)b * d);
    dr.upload(rows, bk);
    dks.upload(ks, (size_t)nks);
    dcut.upload(cutoffs, bn);
    HIP_CHECK(hipMemsetAsync(bad.p, 0xFF, sizeof(int), 0));   // -1: every row id is inside the dataset
    if (d % 4 == 0 && (uintptr_t)ds->x.p % 16 == 0)
      hipLaunchKernelGGL(recall_counts_kernel<true>, dim3(b), dim3(RC_THREADS), 0, 0, ds->x.p, ds->n, d, dq.p, dr.p,
                         max_k, dks.p, nks, dcut.p, dtp.p, dout.p, bad.p);
    else
      hipLaunchKernelGGL(recall_counts_kernel<false>, dim3(b), dim3(RC_THREADS), 0, 0, ds->x.p, ds->n, d, dq.p, dr.p,
                         max_k, dks.p, nks, dcut.p, dtp.p, dout.p, bad.p);
    HIP_CHECK(hipGetLastError());
    int bad_row = -1;
    bad.download(&bad_row, 1);
    dtp.download(out_tp, bn);
    if (out_dist) dout.download(out_dist, bk);
    HIP_CHECK(hipDeviceSynchronize());
    GULON_REQUIRE(bad_row < 0, "row %d out of range [0,%d)", bad_row, ds->n);
  });
}
