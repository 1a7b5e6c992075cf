// MathUtils.distanceSq (MathUtils.scala:85-95) of one query to a workgroup's rows, gathered from a dataset: the tile
// scheme that recall.hip and refine.hip share.  One workgroup per query, lane = position in the query's row list.
#pragma once

#include "common.hpp"

namespace gulon {

constexpr int RC_THREADS = 256;   // positions of one query handled per pass, lane = position
constexpr int RC_DT = 32;         // dims staged per step
constexpr int RC_QS = 4096;       // query components held in LDS (the whole query for d <= 4096)

struct RowTile {
  float xs[RC_THREADS * (RC_DT + 1)];
  float qs[RC_QS];
  int rs[RC_THREADS];
};

// The distance of `query` to row `row` of X (row < 0: no row, the sum of the query's squares -- callers ignore it).
// Called by ALL RC_THREADS threads of the workgroup, once per pass over the query's positions; load_query: qs does not
// hold the query's first RC_QS components yet (the first pass, or every pass when d > RC_QS).
// VEC4: d % 4 == 0, rows are 16-byte aligned -- eight lanes read the 128 bytes of a row's RC_DT floats with one
// 16-byte load each; otherwise 32 lanes read them with 4-byte loads.  Either way the sum of a row is taken afterwards
// from LDS by the row's own lane, i ascending (the tile is padded to RC_DT + 1 floats: no bank conflicts there).
template <bool VEC4>
__device__ __forceinline__ float tile_distance_sq(RowTile &t, const float *__restrict__ X, int d,
                                                  const float *__restrict__ query, int row, bool load_query) {
  const int tid = threadIdx.x;
  __syncthreads();                               // the previous pass has finished with rs, xs and qs
  t.rs[tid] = row;
  float acc = 0.f;
  for (int s0 = 0; s0 < d; s0 += RC_QS) {
    const int s1 = min(d, s0 + RC_QS);
    if (load_query) {
      __syncthreads();
      for (int i = s0 + tid; i < s1; i += RC_THREADS) t.qs[i - s0] = query[i];
    }
    for (int d0 = s0; d0 < s1; d0 += RC_DT) {
      __syncthreads();
      if (VEC4) {
        for (int e = tid; e < RC_THREADS * (RC_DT / 4); e += RC_THREADS) {
          const int r = e / (RC_DT / 4), c = (e % (RC_DT / 4)) * 4;
          const int rr = t.rs[r];
          f32x4 v = {0.f, 0.f, 0.f, 0.f};
          if (rr >= 0 && d0 + c < s1) v = *(const f32x4 *)(X + (size_t)rr * d + d0 + c);
          float *o = t.xs + r * (RC_DT + 1) + c;
          o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
        }
      } else {
        for (int e = tid; e < RC_THREADS * RC_DT; e += RC_THREADS) {
          const int r = e / RC_DT, c = e % RC_DT;
          const int rr = t.rs[r];
          t.xs[r * (RC_DT + 1) + c] = (rr >= 0 && d0 + c < s1) ? X[(size_t)rr * d + d0 + c] : 0.f;
        }
      }
      __syncthreads();
      const int dl = min(RC_DT, s1 - d0);
      for (int c = 0; c < dl; c++) {
        float dx = t.qs[d0 - s0 + c] - t.xs[tid * (RC_DT + 1) + c];   // dx = y(i) - x(i), y = query (MathUtils.scala:90)
        acc += dx * dx;
      }
    }
  }
  return acc;
}

}  // namespace gulon
