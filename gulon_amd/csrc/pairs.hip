// Word-pair similarity: the distance between two stored rows, for many pairs at once, and the integer sums
// from which Spearman's rank correlation of two score lists is finished on the host.
//   pair distances   out[i] = MathUtils.distanceSq(y_a[i], y_b[i]) (MathUtils.scala:85-95): binary32, t = y_a[e] - y_b[e];
//                    sum += t * t, unfused, e ascending, one running sum from 0.f -- the arithmetic of inspect.hip's
//                    row_errors_kernel                                    -- index_pair_distances_kernel (an index),
//                                                                            dataset_pair_distances_kernel (a dataset)
//   rank sums        per section {n_s, sum cx * cy, sum cx^2, sum cy^2, dropped} over the centred doubled average ranks
//                    cx = 2 * less_x + eq_x - n_s of the section's live pairs      -- rank_sums_kernel
// y_r is the vector `lookup` returns for row r.  Flat index (byte and wide codes, a view through its own handle):
// ProductQuantizer.decode of row r (ProductQuantizer.scala:37-50).  Grouped index: centroid(c) + decode(r), one fp32 add
// per coordinate (MathUtils.add, the centroid first), c = the partition of GroupedIndex.lookup (Index.scala:247-253) --
// row_decode.hpp's lookup_base, the rule decode.hip and compose.hip use, deliberately NOT group_centroid (the two rules
// are set side by side there): these are distances between the vectors the index hands out for two words, not between
// a query and a row in the group it is scanned in.  Dataset: the stored row as it is.
// Codes are read in the layout the handle keeps, by two RowWalks per lane (row_decode.hpp RowCodes, clamped to the code
// book); dataset rows go through the gathered tile (row_tile.hpp).  Nothing decoded is written to HBM, and the calls use
// scratch of their own: a handle keeps no trace of them.
#include "row_decode.hpp"
#include "row_tile.hpp"

namespace gulon {
namespace {

constexpr int RS_TILE = 256;            // threads of rank_sums_kernel = pairs staged per step
constexpr int RS_MAX_N = 1 << 20;       // |cx|, |cy| < 2^20, so every sum stays below 2^60

__device__ inline float quiet_nan() { return __int_as_float(0x7FC00000); }

// ---- pair distances ------------------------------------------------------------------------------------------------
// One wavefront per 64 pairs, lane = pair: the sum is sequential per pair, so it is never reduced across lanes.  Every
// lane walks its two rows e ascending; the quantizer the walk is in is wave-uniform.  A pair with a row outside
// [0, n_rows) sets *bad, reads nothing and stores NaN.
template <bool GROUPED>
__global__ __launch_bounds__(64) void index_pair_distances_kernel(CodeSrc src, const float *__restrict__ cents,
                                                                  int n_rows, int d, int k,
                                                                  const int *__restrict__ rows_a,
                                                                  const int *__restrict__ rows_b, int n,
                                                                  const float *__restrict__ gcent,
                                                                  const int *__restrict__ offsets, int n_offsets,
                                                                  float *__restrict__ out, int *__restrict__ bad) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const int ra = rows_a[i], rb = rows_b[i];
  if (ra < 0 || ra >= n_rows || rb < 0 || rb >= n_rows) {   // reported by the host; nothing is read for the pair
    *bad = 1;
    out[i] = quiet_nan();
    return;
  }
  const float *base_a = GROUPED ? lookup_base(gcent, offsets, n_offsets, ra, d) : nullptr;
  const float *base_b = GROUPED ? lookup_base(gcent, offsets, n_offsets, rb, d) : nullptr;
  RowWalk<RowCodes> ya(RowCodes(src, ra), cents, d, src.m, k, k - 1);   // a code at or above k reads as k - 1
  RowWalk<RowCodes> yb(RowCodes(src, rb), cents, d, src.m, k, k - 1);
  float sum = 0.f;
  for (int e = 0; e < d; e++) {
    const float ca = ya.value(e), cb = yb.value(e);
    const float va = GROUPED ? base_a[e] + ca : ca;         // MathUtils.add
    const float vb = GROUPED ? base_b[e] + cb : cb;
    const float t = va - vb;                                // MathUtils.distanceSq: unfused, e ascending
    sum += t * t;
  }
  out[i] = sum;
}

// The dataset form: the 64 `a` rows and the 64 `b` rows of the wave's pairs go through two gathered tiles, RC_DT
// coordinates at a time, so the loads are coalesced per row although the pairs scatter.
template <bool VEC4>
__global__ __launch_bounds__(64) void dataset_pair_distances_kernel(const float *__restrict__ X, int n_rows, int d,
                                                                    const int *__restrict__ rows_a,
                                                                    const int *__restrict__ rows_b, int n,
                                                                    float *__restrict__ out, int *__restrict__ bad) {
  __shared__ float xa[tile_floats(64)], xb[tile_floats(64)];
  __shared__ int ra[64], rb[64];
  const int lane = threadIdx.x, i = blockIdx.x * 64 + lane;
  int a = -1, b = -1;
  if (i < n) {
    a = rows_a[i];
    b = rows_b[i];
    if (a < 0 || a >= n_rows || b < 0 || b >= n_rows) { *bad = 1; a = b = -1; }   // neither row is read
  }
  ra[lane] = a;
  rb[lane] = b;
  float sum = 0.f;
  for (int d0 = 0; d0 < d; d0 += RC_DT) {
    __syncthreads();                            // ra / rb are written; the previous step's tiles have been read
    tile_load<64, VEC4>(xa, ra, X, d, d0, d);
    tile_load<64, VEC4>(xb, rb, X, d, d0, d);
    __syncthreads();
    const int dl = min(RC_DT, d - d0);
    for (int c = 0; c < dl; c++) {
      const float t = tile_at(xa, lane, c) - tile_at(xb, lane, c);
      sum += t * t;
    }
  }
  if (i < n) out[i] = a >= 0 ? sum : quiet_nan();
}

// What the index forms resolve their handle to: IndexRef with the raw offsets lookup_base searches
struct PairIndex {
  gulon_index *ix; std::mutex *mu;
  const float *gcent; const int *offsets; int n_offsets;
};
PairIndex pair_index(gulon_index *idx) {
  GULON_REQUIRE(idx != nullptr, "index is null");
  return {idx, &idx->mu, nullptr, nullptr, 0};
}
PairIndex pair_index(gulon_grouped_index *idx) {
  GULON_REQUIRE(idx != nullptr, "index is null");
  const GroupedParts gp = grouped_parts(idx);
  return {gp.pq, gp.mu, gp.gcent, gp.offsets, gp.n_offsets};
}

void check_pair_args(int n, const void *rows_a, const void *rows_b, const void *out) {
  GULON_REQUIRE(n >= 0, "the number of pairs must be non-negative, got %d", n);
  GULON_REQUIRE(n == 0 || (rows_a != nullptr && rows_b != nullptr && out != nullptr), "null argument");
}

void check_pair_rows_host(const int32_t *rows_a, const int32_t *rows_b, int n, int n_rows) {
  for (int i = 0; i < n; i++)
    GULON_REQUIRE(rows_a[i] >= 0 && rows_a[i] < n_rows && rows_b[i] >= 0 && rows_b[i] < n_rows,
                  "pair %d = (%d, %d) outside [0, %d)", i, rows_a[i], rows_b[i], n_rows);
}

// Launches on `st` (n >= 1) and waits for it: the status comes back with the call
template <class Launch>
void run_pairs(int n, int n_rows, hipStream_t st, Launch launch) {
  DevBuf<int> bad(1);
  HIP_CHECK(hipMemsetAsync(bad.p, 0, sizeof(int), st));
  launch(ceil_div(n, 64), bad.p);
  HIP_CHECK(hipGetLastError());
  int h_bad = 0;
  HIP_CHECK(hipMemcpyAsync(&h_bad, bad.p, sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  GULON_REQUIRE(!h_bad, "a pair of the %d holds a row outside [0, %d)", n, n_rows);
}

// Device pointers; the caller holds the handle's lock
void run_index_pairs(const PairIndex &r, const int *d_a, const int *d_b, int n, float *d_out, hipStream_t st) {
  gulon_index *ix = r.ix;
  require_code_layout(ix);
  StreamOrder so(ix, st);
  run_pairs(n, ix->n, st, [&](int grid, int *bad) {
    if (r.gcent)
      hipLaunchKernelGGL(index_pair_distances_kernel<true>, dim3(grid), dim3(64), 0, st, code_src(ix), ix->cents.p,
                         ix->n, ix->d, ix->k, d_a, d_b, n, r.gcent, r.offsets, r.n_offsets, d_out, bad);
    else
      hipLaunchKernelGGL(index_pair_distances_kernel<false>, dim3(grid), dim3(64), 0, st, code_src(ix), ix->cents.p,
                         ix->n, ix->d, ix->k, d_a, d_b, n, nullptr, nullptr, 0, d_out, bad);
    so.done();
  });
}

void run_dataset_pairs(const gulon_dataset *ds, const int *d_a, const int *d_b, int n, float *d_out, hipStream_t st) {
  const bool v4 = ds->d % 4 == 0 && (uintptr_t)ds->x.p % 16 == 0;
  run_pairs(n, ds->n, st, [&](int grid, int *bad) {
    if (v4)
      hipLaunchKernelGGL(dataset_pair_distances_kernel<true>, dim3(grid), dim3(64), 0, st, ds->x.p, ds->n, ds->d, d_a,
                         d_b, n, d_out, bad);
    else
      hipLaunchKernelGGL(dataset_pair_distances_kernel<false>, dim3(grid), dim3(64), 0, st, ds->x.p, ds->n, ds->d, d_a,
                         d_b, n, d_out, bad);
  });
}

// The host-pointer forms: the rows are checked here, so the offending pair is named; run(d_a, d_b, d_out) on the null
// stream
template <class Run>
void pairs_host(const int32_t *rows_a, const int32_t *rows_b, int n, int n_rows, float *out, Run run) {
  check_pair_rows_host(rows_a, rows_b, n, n_rows);
  DevBuf<int> da, db;
  DevBuf<float> dout((size_t)n);
  da.upload(rows_a, (size_t)n);
  db.upload(rows_b, (size_t)n);
  run(da.p, db.p, dout.p);
  dout.download(out, (size_t)n);
  HIP_CHECK(hipStreamSynchronize(nullptr));
}

void index_pairs_dev(const PairIndex &r, const int *d_a, const int *d_b, int n, float *d_out, hipStream_t st) {
  check_pair_args(n, d_a, d_b, d_out);
  if (n == 0) return;
  std::lock_guard<std::mutex> lock(*r.mu);
  run_index_pairs(r, d_a, d_b, n, d_out, st);
}

void index_pairs_host(const PairIndex &r, const int32_t *rows_a, const int32_t *rows_b, int n, float *out) {
  check_pair_args(n, rows_a, rows_b, out);
  if (n == 0) return;
  std::lock_guard<std::mutex> lock(*r.mu);
  pairs_host(rows_a, rows_b, n, r.ix->n, out,
             [&](const int *da, const int *db, float *dout) { run_index_pairs(r, da, db, n, dout, nullptr); });
}

// ---- rank sums -------------------------------------------------------------------------------------------------------
// An O(n^2) all-pairs count: thread = pair i, the j side staged through LDS RS_TILE entries of (x, y, section) per step;
// a j that is not live is staged with section -1 and so matches nobody.  The comparisons are IEEE (-0 == +0, an infinity
// ties with itself) and eq counts i itself.  Sections may be interleaved.  Every live i adds its four integers to its
// section's sums with 64-bit atomics: integer work only, so the result is exact and does not depend on the order.
// out [nsections][5] = {n_s, sum cx * cy, sum cx^2, sum cy^2, dropped}, zeroed by the caller.
__global__ __launch_bounds__(RS_TILE) void rank_sums_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                            const int *__restrict__ section, int n, int nsections,
                                                            unsigned long long *__restrict__ out) {
  __shared__ float xs[RS_TILE], ys[RS_TILE];
  __shared__ int ss[RS_TILE];
  const int tid = threadIdx.x, i = blockIdx.x * RS_TILE + tid;
  float xi = 0.f, yi = 0.f;
  int si = -1;                                   // -1: i takes no part
  if (i < n) {
    xi = x[i];
    yi = y[i];
    const int s = section ? section[i] : 0;
    if (s >= 0 && s < nsections) {
      if (xi != xi || yi != yi) atomicAdd(&out[(size_t)s * 5 + 4], 1ull);   // dropped: a NaN score
      else si = s;
    }
  }
  int less_x = 0, eq_x = 0, less_y = 0, eq_y = 0, ns = 0;
  for (int j0 = 0; j0 < n; j0 += RS_TILE) {
    __syncthreads();                             // the previous step's tile has been read
    const int j = j0 + tid;
    float xj = 0.f, yj = 0.f;
    int sj = -1;
    if (j < n) {
      xj = x[j];
      yj = y[j];
      const int s = section ? section[j] : 0;
      if (s >= 0 && s < nsections && xj == xj && yj == yj) sj = s;
    }
    xs[tid] = xj; ys[tid] = yj; ss[tid] = sj;
    __syncthreads();
    if (si >= 0) {
      const int jn = min(RS_TILE, n - j0);
      for (int t = 0; t < jn; t++) {
        const bool same = ss[t] == si;
        const float xt = xs[t], yt = ys[t];
        ns += same ? 1 : 0;
        less_x += (same && xt < xi) ? 1 : 0;
        eq_x += (same && xt == xi) ? 1 : 0;
        less_y += (same && yt < yi) ? 1 : 0;
        eq_y += (same && yt == yi) ? 1 : 0;
      }
    }
  }
  if (si < 0) return;
  const long long cx = 2ll * less_x + eq_x - ns, cy = 2ll * less_y + eq_y - ns;   // |c| < n <= 2^20
  unsigned long long *o = out + (size_t)si * 5;
  atomicAdd(&o[0], 1ull);
  atomicAdd(&o[1], (unsigned long long)(cx * cy));   // two's complement: the sum of the int64 products
  atomicAdd(&o[2], (unsigned long long)(cx * cx));
  atomicAdd(&o[3], (unsigned long long)(cy * cy));
}

void check_rank_args(const void *x, const void *y, const void *section, int n, int nsections, const void *out) {
  GULON_REQUIRE(n >= 0 && n <= RS_MAX_N, "the number of pairs must lie in [0, %d], got %d", RS_MAX_N, n);
  GULON_REQUIRE(nsections >= 1, "the number of sections must be at least 1, got %d", nsections);
  GULON_REQUIRE(section != nullptr || nsections == 1, "no section ids: expected 1 section, got %d", nsections);
  GULON_REQUIRE(out != nullptr && (n == 0 || (x != nullptr && y != nullptr)), "null argument");
}

// Device pointers; d_out [nsections][5] is zeroed here.  Does not synchronise.
void launch_rank_sums(const float *d_x, const float *d_y, const int *d_section, int n, int nsections, int64_t *d_out,
                      hipStream_t st) {
  static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the sums are added as unsigned words");
  HIP_CHECK(hipMemsetAsync(d_out, 0, (size_t)nsections * 5 * sizeof(int64_t), st));
  if (n == 0) return;
  hipLaunchKernelGGL(rank_sums_kernel, dim3(ceil_div(n, RS_TILE)), dim3(RS_TILE), 0, st, d_x, d_y, d_section, n,
                     nsections, (unsigned long long *)d_out);
  HIP_CHECK(hipGetLastError());
}

}  // namespace
}  // namespace gulon

using namespace gulon;

GULON_API int32_t gulon_index_pair_distances(gulon_index *idx, const int32_t *rows_a, const int32_t *rows_b, int32_t n,
                                             float *out_dist) {
  return guarded([&] { index_pairs_host(pair_index(idx), rows_a, rows_b, n, out_dist); });
}

GULON_API int32_t gulon_index_pair_distances_dev(gulon_index *idx, const int32_t *d_rows_a, const int32_t *d_rows_b,
                                                 int32_t n, float *d_out_dist, void *stream) {
  return guarded([&] { index_pairs_dev(pair_index(idx), d_rows_a, d_rows_b, n, d_out_dist, (hipStream_t)stream); });
}

GULON_API int32_t gulon_grouped_index_pair_distances(gulon_grouped_index *idx, const int32_t *rows_a,
                                                     const int32_t *rows_b, int32_t n, float *out_dist) {
  return guarded([&] { index_pairs_host(pair_index(idx), rows_a, rows_b, n, out_dist); });
}

GULON_API int32_t gulon_grouped_index_pair_distances_dev(gulon_grouped_index *idx, const int32_t *d_rows_a,
                                                         const int32_t *d_rows_b, int32_t n, float *d_out_dist,
                                                         void *stream) {
  return guarded([&] { index_pairs_dev(pair_index(idx), d_rows_a, d_rows_b, n, d_out_dist, (hipStream_t)stream); });
}

GULON_API int32_t gulon_dataset_pair_distances(const gulon_dataset *ds, const int32_t *rows_a, const int32_t *rows_b,
                                               int32_t n, float *out_dist) {
  return guarded([&] {
    GULON_REQUIRE(ds != nullptr, "dataset is null");
    check_pair_args(n, rows_a, rows_b, out_dist);
    if (n == 0) return;
    pairs_host(rows_a, rows_b, n, ds->n, out_dist,
               [&](const int *da, const int *db, float *dout) { run_dataset_pairs(ds, da, db, n, dout, nullptr); });
  });
}

GULON_API int32_t gulon_dataset_pair_distances_dev(const gulon_dataset *ds, const int32_t *d_rows_a,
                                                   const int32_t *d_rows_b, int32_t n, float *d_out_dist,
                                                   void *stream) {
  return guarded([&] {
    GULON_REQUIRE(ds != nullptr, "dataset is null");
    check_pair_args(n, d_rows_a, d_rows_b, d_out_dist);
    if (n == 0) return;
    run_dataset_pairs(ds, d_rows_a, d_rows_b, n, d_out_dist, (hipStream_t)stream);
  });
}

GULON_API int32_t gulon_rank_sums(const float *x, const float *y, const int32_t *section, int32_t n, int32_t nsections,
                                  int64_t *out) {
  return guarded([&] {
    check_rank_args(x, y, section, n, nsections, out);
    const size_t cells = (size_t)nsections * 5;
    if (n == 0) {
      memset(out, 0, cells * sizeof(int64_t));
      return;
    }
    DevBuf<float> dx, dy;
    DevBuf<int> ds;
    DevBuf<int64_t> dout(cells);
    dx.upload(x, (size_t)n);
    dy.upload(y, (size_t)n);
    if (section) ds.upload(section, (size_t)n);
    launch_rank_sums(dx.p, dy.p, section ? ds.p : nullptr, n, nsections, dout.p, nullptr);
    dout.download(out, cells);
    HIP_CHECK(hipStreamSynchronize(nullptr));
  });
}

GULON_API int32_t gulon_rank_sums_dev(const float *d_x, const float *d_y, const int32_t *d_section, int32_t n,
                                      int32_t nsections, int64_t *d_out, void *stream) {
  return guarded([&] {
    check_rank_args(d_x, d_y, d_section, n, nsections, d_out);
    launch_rank_sums(d_x, d_y, d_section, n, nsections, d_out, (hipStream_t)stream);
  });
}
