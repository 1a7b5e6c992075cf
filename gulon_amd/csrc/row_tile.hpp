// The gathered LDS tile (DESIGN.md "Row reading"): ROWS scattered rows of a dataset staged RC_DT coordinates at a time,
// so that reads which a row list scatters are still coalesced per row and the row's own lane then walks its
// coordinates in order.  On top of it MathUtils.distanceSq (MathUtils.scala:85-95) of one query to a workgroup's rows,
// which recall.hip and refine.hip share: one workgroup per query, lane = position in the query's row list.
#pragma once

#include "common.hpp"

namespace gulon {

constexpr int RC_THREADS = 256;   // positions of one query handled per pass, lane = position
constexpr int RC_DT = 32;         // dims staged per step
constexpr int RC_QS = 4096;       // query components held in LDS (the whole query for d <= 4096)

// A tile of ROWS rows is ROWS * (RC_DT + 1) floats: the padding keeps the lane = row accesses free of bank conflicts.
constexpr int tile_floats(int rows) { return rows * (RC_DT + 1); }
__device__ inline float &tile_at(float *xs, int r, int c) { return xs[r * (RC_DT + 1) + c]; }
__device__ inline const float &tile_at(const float *xs, int r, int c) { return xs[r * (RC_DT + 1) + c]; }

// Cooperative (ROWS threads, a barrier on either side): xs[r][c] = X[rs[r]][d0 + c] for c < RC_DT, 0 where rs[r] < 0 or
// d0 + c >= dend.  VEC4: d % 4 == 0 and X 16-byte aligned -- eight lanes read the 128 bytes of a row's RC_DT floats with
// one 16-byte load each; otherwise 32 lanes read them with 4-byte loads.
template <int ROWS, bool VEC4>
__device__ __forceinline__ void tile_load(float *xs, const int *rs, const float *__restrict__ X, int d, int d0,
                                          int dend) {
  const int tid = threadIdx.x;
  if (VEC4) {
    for (int e = tid; e < ROWS * (RC_DT / 4); e += ROWS) {
      const int r = e / (RC_DT / 4), c = (e % (RC_DT / 4)) * 4;
      const int rr = rs[r];
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (rr >= 0 && d0 + c < dend) v = *(const f32x4 *)(X + (size_t)rr * d + d0 + c);
      float *o = &tile_at(xs, r, c);
      o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
    }
  } else {
    for (int e = tid; e < ROWS * RC_DT; e += ROWS) {
      const int r = e / RC_DT, c = e % RC_DT;
      const int rr = rs[r];
      tile_at(xs, r, c) = (rr >= 0 && d0 + c < dend) ? X[(size_t)rr * d + d0 + c] : 0.f;
    }
  }
}

// The mirror image: out[row0 + r][d0 + c] = xs[r][c] for r < nrows, d0 + c < d, by the same pattern (VEC4: out 16-byte
// aligned as well), so the stores are coalesced too.
template <int ROWS, bool VEC4>
__device__ __forceinline__ void tile_store(const float *xs, float *__restrict__ out, int row0, int nrows, int d,
                                           int d0) {
  const int tid = threadIdx.x;
  if (VEC4) {
    for (int e = tid; e < ROWS * (RC_DT / 4); e += ROWS) {
      const int r = e / (RC_DT / 4), c = (e % (RC_DT / 4)) * 4;
      if (r < nrows && d0 + c < d) {
        const float *o = &tile_at(xs, r, c);
        const f32x4 v = {o[0], o[1], o[2], o[3]};
        *(f32x4 *)(out + (size_t)(row0 + r) * d + d0 + c) = v;
      }
    }
  } else {
    for (int e = tid; e < ROWS * RC_DT; e += ROWS) {
      const int r = e / RC_DT, c = e % RC_DT;
      if (r < nrows && d0 + c < d) out[(size_t)(row0 + r) * d + d0 + c] = tile_at(xs, r, c);
    }
  }
}

struct RowTile {
  float xs[tile_floats(RC_THREADS)];
  float qs[RC_QS];
  int rs[RC_THREADS];
};

// The distance of `query` to row `row` of X (row < 0: no row, the sum of the query's squares -- callers ignore it).
// Called by ALL RC_THREADS threads of the workgroup, once per pass over the query's positions; load_query: qs does not
// hold the query's first RC_QS components yet (the first pass, or every pass when d > RC_QS).
// VEC4 as in tile_load.  The sum of a row is taken from the tile by the row's own lane, i ascending.
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
      tile_load<RC_THREADS, VEC4>(t.xs, t.rs, X, d, d0, s1);
      __syncthreads();
      const int dl = min(RC_DT, s1 - d0);
      for (int c = 0; c < dl; c++) {
        float dx = t.qs[d0 - s0 + c] - tile_at(t.xs, tid, c);   // dx = y(i) - x(i), y = query (MathUtils.scala:90)
        acc += dx * dx;
      }
    }
  }
  return acc;
}

}  // namespace gulon
