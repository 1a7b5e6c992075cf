// Index diagnostics (DESIGN.md "Index diagnostics"): how an index's code books are used and how well its rows
// represent the vectors they were built from, computed over the device-resident index.
//   code histogram   H[j][c] = #{rows r in [from, until) : code of r at quantizer j == c}      -- code_histogram_kernel
//   row errors       row_error[r] = MathUtils.distanceSq(V[map[r]], y_r) (MathUtils.scala:85-95), the summand of
//                    ProductQuantizerSpec.quality (ProductQuantizerSpec.scala:70-73); row_norm_sq[r] the same sum with
//                    y = 0; quantizer_error[j] = the sum over the rows of the same sum restarted over the coordinates
//                    of quantizer j (Vectors.subvectors ranges)                                  -- row_errors_kernel
// y_r is the vector the index's distances are about.  Flat index: ProductQuantizer.decode of row r
// (ProductQuantizer.scala:37-50).  Grouped index: centroid(c) + decode(r), one fp32 add per coordinate (MathUtils.add),
// c = the group whose range [bounds[c], bounds[c + 1]) holds r -- the group a query scans the row in.  That is
// deliberately NOT the partition GroupedIndex.lookup finds with Arrays.binarySearch over the raw offsets
// (gulon_grouped_index_lookup_rows): where offsets repeat (empty groups) that rule can name another group, whose
// centroid no query ever pairs with the row.
// Codes are read in the layout the handle keeps (row_decode.hpp); nothing decoded is written to HBM.  The calls use
// scratch of their own: a handle keeps no trace of them.
#include "row_decode.hpp"

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

// out (host): [m][k] int64; mu: the lock of the handle the caller was given
void code_histogram(gulon_index *ix, std::mutex &mu, int from, int until, int64_t *out) {
  GULON_REQUIRE(out != nullptr, "out is null");
  GULON_REQUIRE(0 <= from && from <= until && until <= ix->n, "expected: 0 <= from <= until <= length");
  const size_t cells = (size_t)ix->m * ix->k;
  if (cells == 0) return;
  if (from == until) {
    memset(out, 0, cells * sizeof(int64_t));
    return;
  }
  GULON_REQUIRE(ix->vec == 4 || ix->vec == 16 || ix->wide, "unexpected code word of %d bytes", ix->vec);
  std::lock_guard<std::mutex> lock(mu);
  DevBuf<unsigned long long> d_out(cells);
  StreamOrder so(ix, nullptr);
  HIP_CHECK(hipMemsetAsync(d_out.p, 0, cells * sizeof(unsigned long long), nullptr));
  const int rb0 = from / 64, nrb = ceil_div(until, 64) - rb0;
  const bool in_lds = cells * sizeof(unsigned) <= IH_LDS_MAX;
  // few workgroups, many blocks each: every workgroup clears and flushes m * k counters
  const int grid = std::max(1, std::min(1024, ceil_div(nrb, IH_WAVES * 16)));
  const size_t lds = in_lds ? cells * sizeof(unsigned) : 0;
#define IH(W, L) hipLaunchKernelGGL((code_histogram_kernel<W, L>), dim3(grid), dim3(IH_THREADS), lds, nullptr, \
                                    code_src(ix), ix->k, from, until, rb0, nrb, d_out.p)
  if (ix->wide) { if (in_lds) IH(true, true); else IH(true, false); }
  else { if (in_lds) IH(false, true); else IH(false, false); }
#undef IH
  HIP_CHECK(hipGetLastError());
  so.done();
  static_assert(sizeof(unsigned long long) == sizeof(int64_t), "counts are downloaded as they are");
  HIP_CHECK(hipMemcpyAsync(out, d_out.p, cells * sizeof(int64_t), hipMemcpyDeviceToHost, nullptr));
  HIP_CHECK(hipStreamSynchronize(nullptr));
}

// ---- row errors --------------------------------------------------------------------------------------------------
// One wavefront per 64-row block, lane = row: MathUtils.distanceSq is one running binary32 sum over e ascending, so a
// row's coordinates are never reduced across lanes.  The block's codes are staged in LDS once (16-byte loads, as
// decode_range_kernel does); the 64 originals V[map[r]] go through an LDS tile RE_DT coordinates at a time (row_tile.hpp's
// scheme: eight lanes read the 128 bytes of one row with a 16-byte load each, so the loads are coalesced per row
// although the map scatters the rows; the tile is padded to RE_DT + 1 floats for the lane = row reads).  Code-book
// entries come through the caches.  One pass gives row_error, row_norm_sq and the per-quantizer sums p[r][j]; at the end
// of every quantizer's coordinates the wave adds its 64 p up in binary64 and stores the block's partial sum
// (qpart[block][j]); quantizer_error_kernel then adds the blocks up, in a fixed order: the result is deterministic.
// A lane whose row is outside [from, until) takes no part; a map entry outside [0, vn) sets *bad and nothing is read for
// that row.
constexpr int RE_DT = 32;

template <bool WIDE, bool VEC4>
__global__ __launch_bounds__(64) void row_errors_kernel(CodeSrc src, const float *__restrict__ cents, int d, int k,
                                                        const float *__restrict__ X, int vn,
                                                        const int *__restrict__ row_map, const float *__restrict__ gcent,
                                                        const int *__restrict__ bounds, int g, int from, int until,
                                                        int rb0, float *__restrict__ row_error,
                                                        float *__restrict__ row_norm_sq, double *__restrict__ qpart,
                                                        int *__restrict__ bad) {
  __shared__ float xs[64 * (RE_DT + 1)];
  __shared__ int rs[64];
  extern __shared__ __attribute__((aligned(16))) uint8_t re_code[];
  const int lane = threadIdx.x, m = src.m;
  const int rb = rb0 + blockIdx.x;
  // stage: byte layout [ng][64][vec] bytes, wide [m][64] uint16 -- both contiguous per block, multiples of 16 bytes
  const int chunk = WIDE ? m * 128 : src.ng * 64 * src.vec;
  const uint4 *gsrc = WIDE ? (const uint4 *)(src.wcodes + (size_t)rb * m * 64)
                           : (const uint4 *)(src.codes + (size_t)rb * chunk);
  for (int t = lane; t < chunk / 16; t += 64) ((uint4 *)re_code)[t] = gsrc[t];
  const int row = rb * 64 + lane;
  const bool inside = row >= from && row < until;
  int vrow = -1;
  if (inside) {
    vrow = row_map ? row_map[row] : row;
    if (vrow < 0 || vrow >= vn) { *bad = 1; vrow = -1; }   // reported by the host; the row of V is not read
  }
  rs[lane] = vrow;
  const bool active = vrow >= 0;
  const float *base = nullptr;                  // grouped: the centroid of the row's own group
  if (active && gcent) {
    int lo = 0, hi = g;                         // largest c with bounds[c] <= row: [bounds[c], bounds[c + 1]) holds it
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (bounds[mid] <= row) lo = mid; else hi = mid; }
    base = gcent + (size_t)lo * d;
  }
  __syncthreads();
  auto code_of = [&](int j) -> int {
    const int c = WIDE ? ((const uint16_t *)re_code)[j * 64 + lane]
                       : re_code[(j / src.vec) * 64 * src.vec + lane * src.vec + j % src.vec];
    return min(c, k - 1);
  };
  const SubvectorMap sv(d, m);
  double *qp = qpart + (size_t)blockIdx.x * m;
  auto flush = [&](int j, float p) {            // all 64 lanes: the block's binary64 sum of p[r][j]
    double v = active ? (double)p : 0.0;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    if (lane == 0) qp[j] = v;
  };
  int j = 0, jfrom = 0, jend = sv.sdim(0);
  const float *cj = active ? cents + (size_t)code_of(0) * sv.sdim(0) : nullptr;   // entry of quantizer j for this row
  float err = 0.f, nrm = 0.f, p = 0.f;
  for (int d0 = 0; d0 < d; d0 += RE_DT) {
    __syncthreads();                            // the previous step's tile has been read
    if (VEC4) {
      for (int e = lane; e < 64 * (RE_DT / 4); e += 64) {
        const int r = e / (RE_DT / 4), c = (e % (RE_DT / 4)) * 4;
        const int rr = rs[r];
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (rr >= 0 && d0 + c < d) v = *(const f32x4 *)(X + (size_t)rr * d + d0 + c);
        float *o = xs + r * (RE_DT + 1) + c;
        o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
      }
    } else {
      for (int e = lane; e < 64 * RE_DT; e += 64) {
        const int r = e / RE_DT, c = e % RE_DT;
        const int rr = rs[r];
        xs[r * (RE_DT + 1) + c] = (rr >= 0 && d0 + c < d) ? X[(size_t)rr * d + d0 + c] : 0.f;
      }
    }
    __syncthreads();
    const int dl = min(RE_DT, d - d0);
    for (int c = 0; c < dl; c++) {
      const int e = d0 + c;
      while (e == jend && j + 1 < m) {          // (wave-uniform) quantizer j is complete
        flush(j, p);
        p = 0.f;
        j++;
        jfrom = jend;
        jend += sv.sdim(j);
        if (active) cj = cents + (size_t)k * jfrom + (size_t)code_of(j) * sv.sdim(j);
      }
      if (active) {
        const float x = xs[lane * (RE_DT + 1) + c];
        const float ce = cj[e - jfrom];
        const float y = base ? base[e] + ce : ce;           // MathUtils.add
        const float t = x - y;                              // MathUtils.distanceSq: unfused, e ascending
        err += t * t;
        p += t * t;
        nrm += x * x;
      }
    }
  }
  flush(j, p);
  for (int jj = j + 1; jj < m; jj++) flush(jj, 0.f);        // quantizers without coordinates (d < m)
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

struct GroupBase { const float *gcent; const int *bounds; int g; };

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
  const size_t lds = ix->wide ? (size_t)m * 128 : (size_t)ix->ng * 64 * ix->vec;
  GULON_UNSUPPORTED(lds + sizeof(float) * 64 * (RE_DT + 2) > 64 * 1024, "m = %d: one row block's codes do not fit in LDS", m);
  const int rb0 = from / 64, nrb = ceil_div(until, 64) - rb0;
  DevBuf<double> qpart((size_t)nrb * m), qsum((size_t)m);
  DevBuf<int> bad(1);
  StreamOrder so(ix, st);
  HIP_CHECK(hipMemsetAsync(bad.p, 0, sizeof(int), st));
  const bool v4 = ix->d % 4 == 0 && (uintptr_t)ds->x.p % 16 == 0;
#define RE(W, V) hipLaunchKernelGGL((row_errors_kernel<W, V>), dim3(nrb), dim3(64), lds, st, code_src(ix), ix->cents.p, \
                                    ix->d, ix->k, ds->x.p, ds->n, d_map, gb.gcent, gb.bounds, gb.g, from, until, rb0,   \
                                    d_err, d_norm, qpart.p, bad.p)
  if (ix->wide) { if (v4) RE(true, true); else RE(true, false); }
  else { if (v4) RE(false, true); else RE(false, false); }
#undef RE
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

void row_errors_dev(gulon_index *ix, std::mutex &mu, GroupBase gb, const gulon_dataset *ds, const int *d_map,
                    int map_len, int from, int until, float *d_err, float *d_norm, double *quantizer_error,
                    hipStream_t st) {
  check_row_error_args(ix, ds, d_map != nullptr, map_len, from, until, quantizer_error);
  std::lock_guard<std::mutex> lock(mu);
  run_row_errors(ix, ds, d_map, gb, from, until, d_err, d_norm, quantizer_error, st);
}

void row_errors_host(gulon_index *ix, std::mutex &mu, GroupBase gb, const gulon_dataset *ds, const int *row_map,
                     int map_len, int from, int until, float *row_error, float *row_norm_sq,
                     double *quantizer_error) {
  check_row_error_args(ix, ds, row_map != nullptr, map_len, from, until, quantizer_error);
  const size_t rows = (size_t)(until - from);
  GULON_REQUIRE(rows == 0 || row_error != nullptr, "row_error is null");
  std::lock_guard<std::mutex> lock(mu);
  DevBuf<int> dmap;
  DevBuf<float> derr(rows), dnorm(row_norm_sq ? rows : 0);
  if (row_map && map_len) dmap.upload(row_map, (size_t)map_len);
  try {
    run_row_errors(ix, ds, row_map ? dmap.p : nullptr, gb, from, until, derr.p, row_norm_sq ? dnorm.p : nullptr,
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

GroupBase group_base(const GroupedParts &gp) { return {gp.gcent, gp.bounds, gp.g}; }

}  // namespace
}  // namespace gulon

using namespace gulon;

GULON_API int32_t gulon_index_code_histogram(gulon_index *idx, int32_t from, int32_t until, int64_t *out) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    code_histogram(idx, idx->mu, from, until, out);
  });
}

GULON_API int32_t gulon_grouped_index_code_histogram(gulon_grouped_index *idx, int32_t from, int32_t until,
                                                     int64_t *out) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    const GroupedParts gp = grouped_parts(idx);
    code_histogram(gp.pq, *gp.mu, from, until, out);
  });
}

GULON_API int32_t gulon_index_row_errors(gulon_index *idx, const gulon_dataset *vectors, const int32_t *row_map,
                                         int32_t map_len, int32_t from, int32_t until, float *row_error,
                                         float *row_norm_sq, double *quantizer_error) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    row_errors_host(idx, idx->mu, GroupBase{nullptr, nullptr, 0}, vectors, row_map, map_len, from, until, row_error,
                    row_norm_sq, quantizer_error);
  });
}

GULON_API int32_t gulon_index_row_errors_dev(gulon_index *idx, const gulon_dataset *vectors, const int32_t *d_row_map,
                                             int32_t map_len, int32_t from, int32_t until, float *d_row_error,
                                             float *d_row_norm_sq, double *quantizer_error, void *stream) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    row_errors_dev(idx, idx->mu, GroupBase{nullptr, nullptr, 0}, vectors, d_row_map, map_len, from, until, d_row_error,
                   d_row_norm_sq, quantizer_error, (hipStream_t)stream);
  });
}

GULON_API int32_t gulon_grouped_index_row_errors(gulon_grouped_index *idx, const gulon_dataset *vectors,
                                                 const int32_t *row_map, int32_t map_len, int32_t from, int32_t until,
                                                 float *row_error, float *row_norm_sq, double *quantizer_error) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    const GroupedParts gp = grouped_parts(idx);
    row_errors_host(gp.pq, *gp.mu, group_base(gp), vectors, row_map, map_len, from, until, row_error, row_norm_sq,
                    quantizer_error);
  });
}

GULON_API int32_t gulon_grouped_index_row_errors_dev(gulon_grouped_index *idx, const gulon_dataset *vectors,
                                                     const int32_t *d_row_map, int32_t map_len, int32_t from,
                                                     int32_t until, float *d_row_error, float *d_row_norm_sq,
                                                     double *quantizer_error, void *stream) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    const GroupedParts gp = grouped_parts(idx);
    row_errors_dev(gp.pq, *gp.mu, group_base(gp), vectors, d_row_map, map_len, from, until, d_row_error, d_row_norm_sq,
                   quantizer_error, (hipStream_t)stream);
  });
}
