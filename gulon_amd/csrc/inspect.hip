// Index diagnostics (DESIGN.md "Index diagnostics"): how an index's code books are used and how well its rows
// represent the vectors they were built from, computed over the device-resident index.
//   code histogram   H[j][c] = #{rows r in [from, until) : code of r at quantizer j == c}      -- code_histogram_kernel
//   row errors       row_error[r] = MathUtils.distanceSq(V[map[r]], y_r) (MathUtils.scala:85-95), the summand of
//                    ProductQuantizerSpec.quality (ProductQuantizerSpec.scala:70-73); row_norm_sq[r] the same sum with
//                    y = 0; quantizer_error[j] = the sum over the rows of the same sum restarted over the coordinates
//                    of quantizer j (Vectors.subvectors ranges)                                  -- row_errors_kernel
// y_r is the vector the index's distances are about.  Flat index: ProductQuantizer.decode of row r
// (ProductQuantizer.scala:37-50).  Grouped index: centroid(c) + decode(r), one fp32 add per coordinate (MathUtils.add),
// c = the group whose range [bounds[c], bounds[c + 1]) holds r -- row_decode.hpp's group_centroid, deliberately NOT the
// partition of GroupedIndex.lookup (the two rules are set side by side there).
// Codes are read in the layout the handle keeps: the row errors walk a staged block (row_decode.hpp StagedCodes, RowWalk,
// clamped to the code book) beside the gathered tile of the originals (row_tile.hpp); the histogram reads whole code
// words itself, every quantizer of a word unrolled.  Nothing decoded is written to HBM.  The calls use scratch of their
// own: a handle keeps no trace of them.
#include "row_decode.hpp"
#include "row_tile.hpp"

namespace gulon {
namespace {

// ---- code histogram --------------------------------------------------------------------------------------------
// Lane = row, wave = one 64-row block at a time, a workgroup walks every (gridDim.x * IH_WAVES)-th block.  A lane whose
// row is outside [from, until) counts nothing: the padding rows of a ragged last block hold zero words and lie at or
// above n >= until.  Padding quantizers (j >= m) of the byte layout are skipped.  IN_LDS: the workgroup's counts sit in
// LDS ([m][k] uint32) and are flushed with one global add per non-zero entry; otherwise (m * k * 4 bytes beyond LDS)
// every count is a global add.  A code at or above k (not a code of this code book) is not counted.
constexpr int IH_THREADS = 256, IH_WAVES = IH_THREADS / 64;
constexpr size_t IH_LDS_MAX = 64 * 1024;

template <bool WIDE, bool IN_LDS>
__global__ __launch_bounds__(IH_THREADS) void code_histogram_kernel(CodeSrc src, int k, int from, int until, int rb0,
                                                                    int nrb, unsigned long long *__restrict__ out) {
  extern __shared__ unsigned ih_lds[];   // IN_LDS: [m][k]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m = src.m;
  const int cells = m * k;
  if (IN_LDS) {
    for (int e = tid; e < cells; e += IH_THREADS) ih_lds[e] = 0u;
    __syncthreads();
  }
  auto count = [&](int j, unsigned c) {
    if (c >= (unsigned)k) return;
    if (IN_LDS) atomicAdd(&ih_lds[j * k + c], 1u);
    else atomicAdd(&out[(size_t)j * k + c], 1ull);
  };
  for (int b = blockIdx.x * IH_WAVES + wave; b < nrb; b += gridDim.x * IH_WAVES) {
    const int rb = rb0 + b;
    const int row = rb * 64 + lane;
    if (row < from || row >= until) continue;
    if (WIDE) {
      const uint16_t *p = src.wcodes + (size_t)rb * m * 64 + lane;
      for (int j = 0; j < m; j++) count(j, p[(size_t)j * 64]);
    } else if (src.vec == 16) {
      const uint4 *cw = reinterpret_cast<const uint4 *>(src.codes);
      for (int gi = 0; gi < src.ng; gi++) {
        const uint4 w = cw[((size_t)rb * src.ng + gi) * 64 + lane];
#pragma unroll
        for (int x = 0; x < 16; x++)
          if (gi * 16 + x < m) count(gi * 16 + x, code_byte<16>(w, x));
      }
    } else {
      const uint32_t *cw = reinterpret_cast<const uint32_t *>(src.codes);
      for (int gi = 0; gi < src.ng; gi++) {
        const uint32_t w = cw[((size_t)rb * src.ng + gi) * 64 + lane];
#pragma unroll
        for (int x = 0; x < 4; x++)
          if (gi * 4 + x < m) count(gi * 4 + x, code_byte<4>(w, x));
      }
    }
  }
  if (IN_LDS) {
    __syncthreads();
    for (int e = tid; e < cells; e += IH_THREADS) {
      const unsigned v = ih_lds[e];
      if (v) atomicAdd(&out[e], (unsigned long long)v);
    }
  }
}

// out (host): [m][k] int64
void code_histogram(const IndexRef &r, int from, int until, int64_t *out) {
  gulon_index *ix = r.ix;
  GULON_REQUIRE(out != nullptr, "out is null");
  GULON_REQUIRE(0 <= from && from <= until && until <= ix->n, "expected: 0 <= from <= until <= length");
  const size_t cells = (size_t)ix->m * ix->k;
  if (cells == 0) return;
  if (from == until) {
    memset(out, 0, cells * sizeof(int64_t));
    return;
  }
  require_code_layout(ix);
  std::lock_guard<std::mutex> lock(*r.mu);
  DevBuf<unsigned long long> d_out(cells);
  StreamOrder so(ix, nullptr);
  HIP_CHECK(hipMemsetAsync(d_out.p, 0, cells * sizeof(unsigned long long), nullptr));
  const int rb0 = from / 64, nrb = ceil_div(until, 64) - rb0;
  const bool in_lds = cells * sizeof(unsigned) <= IH_LDS_MAX;
  // few workgroups, many blocks each: every workgroup clears and flushes m * k counters
  const int grid = std::max(1, std::min(1024, ceil_div(nrb, IH_WAVES * 16)));
  const size_t lds = in_lds ? cells * sizeof(unsigned) : 0;
  dispatch_flags(ix->wide, in_lds, [&](auto wide, auto lds_counts) {
    hipLaunchKernelGGL((code_histogram_kernel<wide.value, lds_counts.value>), dim3(grid), dim3(IH_THREADS), lds, nullptr,
                       code_src(ix), ix->k, from, until, rb0, nrb, d_out.p);
  });
  HIP_CHECK(hipGetLastError());
  so.done();
  static_assert(sizeof(unsigned long long) == sizeof(int64_t), "counts are downloaded as they are");
  HIP_CHECK(hipMemcpyAsync(out, d_out.p, cells * sizeof(int64_t), hipMemcpyDeviceToHost, nullptr));
  HIP_CHECK(hipStreamSynchronize(nullptr));
}

// ---- row errors --------------------------------------------------------------------------------------------------
// One wavefront per 64-row block, lane = row: MathUtils.distanceSq is one running binary32 sum over e ascending, so a
// row's coordinates are never reduced across lanes.  The block's codes are staged in LDS once (StagedCodes, as
// decode_range_kernel does) and walked per lane by a RowWalk; the 64 originals V[map[r]] go through the gathered tile
// (row_tile.hpp tile_load), so the loads are coalesced per row although the map scatters the rows.  Code-book
// entries come through the caches.  One pass gives row_error, row_norm_sq and the per-quantizer sums p[r][j]; at the end
// of every quantizer's coordinates the wave adds its 64 p up in binary64 and stores the block's partial sum
// (qpart[block][j]); quantizer_error_kernel then adds the blocks up, in a fixed order: the result is deterministic.
// A lane whose row is outside [from, until) takes no part; a map entry outside [0, vn) sets *bad and nothing is read for
// that row.
template <bool WIDE, bool VEC4>
__global__ __launch_bounds__(64) void row_errors_kernel(CodeSrc src, const float *__restrict__ cents, int d, int k,
                                                        const float *__restrict__ X, int vn,
                                                        const int *__restrict__ row_map, GroupBase gb, int from,
                                                        int until, int rb0, float *__restrict__ row_error,
                                                        float *__restrict__ row_norm_sq, double *__restrict__ qpart,
                                                        int *__restrict__ bad) {
  __shared__ float xs[tile_floats(64)];
  __shared__ int rs[64];
  extern __shared__ __attribute__((aligned(16))) uint8_t re_code[];
  const int lane = threadIdx.x, m = src.m;
  const int rb = rb0 + blockIdx.x;
  const StagedCodes<WIDE> staged{re_code, src.vec};
  staged.stage(src, rb, lane, 64);
  const int row = rb * 64 + lane;
  const bool inside = row >= from && row < until;
  int vrow = -1;
  if (inside) {
    vrow = row_map ? row_map[row] : row;
    if (vrow < 0 || vrow >= vn) { *bad = 1; vrow = -1; }   // reported by the host; the row of V is not read
  }
  rs[lane] = vrow;
  const bool active = vrow >= 0;
  const float *base = (active && gb.gcent) ? group_centroid(gb, row, d) : nullptr;   // the row's own group
  __syncthreads();
  RowWalk<StagedRow<WIDE>> y(StagedRow<WIDE>{staged, lane}, cents, d, m, k, k - 1);   // a code >= k reads as k - 1
  y.enter_next();                               // quantizer 0
  double *qp = qpart + (size_t)blockIdx.x * m;
  float err = 0.f, nrm = 0.f, p = 0.f;
  auto flush = [&](int j) {                     // all 64 lanes: the block's binary64 sum of p[r][j]; p starts again
    double v = active ? (double)p : 0.0;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    if (lane == 0) qp[j] = v;
    p = 0.f;
  };
  for (int d0 = 0; d0 < d; d0 += RC_DT) {
    __syncthreads();                            // the previous step's tile has been read
    tile_load<64, VEC4>(xs, rs, X, d, d0, d);
    __syncthreads();
    const int dl = min(RC_DT, d - d0);
    for (int c = 0; c < dl; c++) {
      const int e = d0 + c;
      if (y.behind(e)) {                        // (wave-uniform) quantizer y.j is complete
        flush(y.j);
        y.enter_next();
      }
      if (active) {
        const float x = tile_at(xs, lane, c);
        const float ce = y.at(e);
        const float yv = base ? base[e] + ce : ce;          // MathUtils.add
        const float t = x - yv;                             // MathUtils.distanceSq: unfused, e ascending
        err += t * t;
        p += t * t;
        nrm += x * x;
      }
    }
  }
  flush(y.j);
  if (inside) {
    row_error[row - from] = err;
    if (row_norm_sq) row_norm_sq[row - from] = nrm;
  }
}

// quantizer_error[j] = the blocks' partial sums added up in binary64: thread t takes blocks t, t + 256, ... in order,
// then a tree over the 256 threads
__global__ __launch_bounds__(256) void quantizer_error_kernel(const double *__restrict__ qpart, int nblk, int m,
                                                              double *__restrict__ out) {
  __shared__ double acc[256];
  const int j = blockIdx.x, tid = threadIdx.x;
  double v = 0.0;
  for (int b = tid; b < nblk; b += 256) v += qpart[(size_t)b * m + j];
  acc[tid] = v;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (tid < o) acc[tid] += acc[tid + o];
    __syncthreads();
  }
  if (tid == 0) out[j] = acc[0];
}

void check_row_error_args(const gulon_index *ix, const gulon_dataset *ds, bool have_map, int map_len, int from,
                          int until, const double *quantizer_error) {
  GULON_REQUIRE(ds != nullptr, "vectors is null");
  GULON_REQUIRE(0 <= from && from <= until && until <= ix->n, "expected: 0 <= from <= until <= length");
  GULON_REQUIRE(ds->d == ix->d, "vectors of dimension %d for an index of dimension %d", ds->d, ix->d);
  if (have_map) GULON_REQUIRE(map_len == ix->n, "a row map of %d entries for an index of %d rows", map_len, ix->n);
  else GULON_REQUIRE(ds->n >= ix->n, "%d vectors for an index of %d rows and no row map", ds->n, ix->n);
  GULON_REQUIRE(quantizer_error != nullptr || ix->m == 0, "quantizer_error is null");
}

// Everything in device memory but quantizer_error (host, [m]); the caller holds the handle's lock.  Synchronises `st`.
void run_row_errors(gulon_index *ix, const gulon_dataset *ds, const int *d_map, GroupBase gb, int from, int until,
                    float *d_err, float *d_norm, double *quantizer_error, hipStream_t st) {
  const int m = ix->m;
  for (int j = 0; j < m; j++) quantizer_error[j] = 0.0;
  if (from == until) return;
  GULON_REQUIRE(d_err != nullptr, "row_error is null");
  const size_t lds = block_code_bytes(ix);
  GULON_UNSUPPORTED(lds + sizeof(float) * (tile_floats(64) + 64) > 64 * 1024,
                    "m = %d: one row block's codes do not fit in LDS", m);
  const int rb0 = from / 64, nrb = ceil_div(until, 64) - rb0;
  DevBuf<double> qpart((size_t)nrb * m), qsum((size_t)m);
  DevBuf<int> bad(1);
  StreamOrder so(ix, st);
  HIP_CHECK(hipMemsetAsync(bad.p, 0, sizeof(int), st));
  const bool v4 = ix->d % 4 == 0 && (uintptr_t)ds->x.p % 16 == 0;
  dispatch_flags(ix->wide, v4, [&](auto wide, auto vec4) {
    hipLaunchKernelGGL((row_errors_kernel<wide.value, vec4.value>), dim3(nrb), dim3(64), lds, st, code_src(ix),
                       ix->cents.p, ix->d, ix->k, ds->x.p, ds->n, d_map, gb, from, until, rb0, d_err, d_norm, qpart.p,
                       bad.p);
  });
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(quantizer_error_kernel, dim3(m), dim3(256), 0, st, qpart.p, nrb, m, qsum.p);
  HIP_CHECK(hipGetLastError());
  so.done();
  int h_bad = 0;
  HIP_CHECK(hipMemcpyAsync(&h_bad, bad.p, sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(quantizer_error, qsum.p, sizeof(double) * m, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  GULON_REQUIRE(!h_bad, "a row map entry of rows [%d, %d) lies outside the %d vectors", from, until, ds->n);
}

void row_errors_dev(const IndexRef &r, const gulon_dataset *ds, const int *d_map, int map_len, int from, int until,
                    float *d_err, float *d_norm, double *quantizer_error, hipStream_t st) {
  check_row_error_args(r.ix, ds, d_map != nullptr, map_len, from, until, quantizer_error);
  std::lock_guard<std::mutex> lock(*r.mu);
  run_row_errors(r.ix, ds, d_map, r.gb, from, until, d_err, d_norm, quantizer_error, st);
}

void row_errors_host(const IndexRef &r, const gulon_dataset *ds, const int *row_map, int map_len, int from, int until,
                     float *row_error, float *row_norm_sq, double *quantizer_error) {
  gulon_index *ix = r.ix;
  check_row_error_args(ix, ds, row_map != nullptr, map_len, from, until, quantizer_error);
  const size_t rows = (size_t)(until - from);
  GULON_REQUIRE(rows == 0 || row_error != nullptr, "row_error is null");
  std::lock_guard<std::mutex> lock(*r.mu);
  DevBuf<int> dmap;
  DevBuf<float> derr(rows), dnorm(row_norm_sq ? rows : 0);
  if (row_map && map_len) dmap.upload(row_map, (size_t)map_len);
  try {
    run_row_errors(ix, ds, row_map ? dmap.p : nullptr, r.gb, from, until, derr.p, row_norm_sq ? dnorm.p : nullptr,
                   quantizer_error, nullptr);
  } catch (const DeviceError &e) {
    if (e.code == GULON_ERR_INVALID_ARGUMENT && row_map)   // the device found it: name the offender
      for (int r = from; r < until; r++)
        GULON_REQUIRE(row_map[r] >= 0 && row_map[r] < ds->n, "row map entry %d = %d outside [0, %d)", r, row_map[r],
                      ds->n);
    throw;
  }
  derr.download(row_error, rows);
  if (row_norm_sq) dnorm.download(row_norm_sq, rows);
  HIP_CHECK(hipStreamSynchronize(nullptr));
}

}  // namespace
}  // namespace gulon

using namespace gulon;

GULON_API int32_t gulon_index_code_histogram(gulon_index *idx, int32_t from, int32_t until, int64_t *out) {
  return guarded([&] { code_histogram(index_ref(idx), from, until, out); });
}

GULON_API int32_t gulon_grouped_index_code_histogram(gulon_grouped_index *idx, int32_t from, int32_t until,
                                                     int64_t *out) {
  return guarded([&] { code_histogram(index_ref(idx), from, until, out); });
}

GULON_API int32_t gulon_index_row_errors(gulon_index *idx, const gulon_dataset *vectors, const int32_t *row_map,
                                         int32_t map_len, int32_t from, int32_t until, float *row_error,
                                         float *row_norm_sq, double *quantizer_error) {
  return guarded([&] {
    row_errors_host(index_ref(idx), vectors, row_map, map_len, from, until, row_error, row_norm_sq, quantizer_error);
  });
}

GULON_API int32_t gulon_index_row_errors_dev(gulon_index *idx, const gulon_dataset *vectors, const int32_t *d_row_map,
                                             int32_t map_len, int32_t from, int32_t until, float *d_row_error,
                                             float *d_row_norm_sq, double *quantizer_error, void *stream) {
  return guarded([&] {
    row_errors_dev(index_ref(idx), vectors, d_row_map, map_len, from, until, d_row_error, d_row_norm_sq, quantizer_error,
                   (hipStream_t)stream);
  });
}

GULON_API int32_t gulon_grouped_index_row_errors(gulon_grouped_index *idx, const gulon_dataset *vectors,
                                                 const int32_t *row_map, int32_t map_len, int32_t from, int32_t until,
                                                 float *row_error, float *row_norm_sq, double *quantizer_error) {
  return guarded([&] {
    row_errors_host(index_ref(idx), vectors, row_map, map_len, from, until, row_error, row_norm_sq, quantizer_error);
  });
}

GULON_API int32_t gulon_grouped_index_row_errors_dev(gulon_grouped_index *idx, const gulon_dataset *vectors,
                                                     const int32_t *d_row_map, int32_t map_len, int32_t from,
                                                     int32_t until, float *d_row_error, float *d_row_norm_sq,
                                                     double *quantizer_error, void *stream) {
  return guarded([&] {
    row_errors_dev(index_ref(idx), vectors, d_row_map, map_len, from, until, d_row_error, d_row_norm_sq, quantizer_error,
                   (hipStream_t)stream);
  });
}
