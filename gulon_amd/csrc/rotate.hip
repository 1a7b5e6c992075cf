// Rotated indexes (DESIGN.md "Rotated indexes"): an orthogonal rotation applied once to the data and once to each query,
// and the second moment a rotation is learned from.  Neither is a Scala method: the reference has no rotation, so the
// entry points below cite nothing in it; their arithmetic follows the project's convention instead.
//   rotate   out[i][c] = sum_j x[i][j] * R[j][c] (transpose: R[c][j]) -- binary32, s = 0; j ascending: s = s + (x * R),
//            product and sum each rounded, nothing fused                                          -- rotate_kernel
//   moment   out[p][q] = sum_r a[r][p] * b[r][q] in binary64.  The product of two binary32 values is exact in binary64,
//            so only the additions round.  Rows are cut into chunks of MOMENT_ROWS -- a constant of this file, never a
//            function of the device -- each chunk summed r ascending by one workgroup into a slab of partial sums, the
//            slabs added in ascending chunk order by a second kernel.  No floating-point atomics: the result is the same
//            bits on every run and every device                         -- moment_partial_kernel, moment_sum_kernel
//            The rows may come through a row map, r then a position in two lists of rows (moment_rows, moment.hpp;
//            alignment.hip's pair moment): the same kernels and the same chunk driver.
// Both use scratch of their own and touch no index handle.
#include "moment.hpp"

namespace gulon {
namespace {

// ---- rotate ----------------------------------------------------------------------------------------------------
// Lane = output column; a wave owns a strip of ROT_STRIP rows, a workgroup ROT_ROWS rows x ROT_COLS columns.  j is walked
// in slabs of ROT_SLAB: the slab of R (any d: it never has to fit LDS whole) and the workgroup's x tile are staged in
// LDS, the ROT_STRIP running sums stay in registers.  Per j a wave reads its column's R[j][c] once (ds_read_b32, leading
// dimension ROT_COLS + 1: conflict-free both for this read and for the transposed staging write, whose lanes run along
// j) and the strip's x values as wave-uniform broadcast reads, four j at a time (ds_read_b128).  x is read along its
// rows, R along its rows in either orientation, out is written one 256-byte row segment per wave: all coalesced.
// Rows and columns outside the matrix are staged as zeros and never stored; they meet no other row's or column's sum.
constexpr int ROT_THREADS = 256, ROT_WAVES = ROT_THREADS / 64;
constexpr int ROT_COLS = 64, ROT_STRIP = 16, ROT_ROWS = ROT_WAVES * ROT_STRIP, ROT_SLAB = 32, ROT_LD = ROT_COLS + 1;

template <bool TRANSPOSE>
__global__ __launch_bounds__(ROT_THREADS) void rotate_kernel(const float *__restrict__ x, long long n, int d,
                                                             const float *__restrict__ rot, float *__restrict__ out) {
  __shared__ float s_r[ROT_SLAB * ROT_LD];
  __shared__ __attribute__((aligned(16))) float s_x[ROT_ROWS * ROT_SLAB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long row0 = (long long)blockIdx.x * ROT_ROWS;
  const int c0 = blockIdx.y * ROT_COLS;
  float acc[ROT_STRIP];
#pragma unroll
  for (int t = 0; t < ROT_STRIP; t++) acc[t] = 0.0f;
  const float *xs = s_x + wave * ROT_STRIP * ROT_SLAB;
  for (int j0 = 0; j0 < d; j0 += ROT_SLAB) {
    const int js = min(ROT_SLAB, d - j0);
    __syncthreads();   // the previous slab has been read
    for (int e = tid; e < ROT_SLAB * ROT_COLS; e += ROT_THREADS) {
      // consecutive lanes run along a row of R: along c as stored, along j when transposed
      const int jj = TRANSPOSE ? e % ROT_SLAB : e / ROT_COLS, cc = TRANSPOSE ? e / ROT_SLAB : e % ROT_COLS;
      const int j = j0 + jj, c = c0 + cc;
      float v = 0.0f;
      if (j < d && c < d) v = TRANSPOSE ? rot[(size_t)c * d + j] : rot[(size_t)j * d + c];
      s_r[jj * ROT_LD + cc] = v;
    }
    for (int e = tid; e < ROT_ROWS * ROT_SLAB; e += ROT_THREADS) {
      const long long r = row0 + e / ROT_SLAB;
      const int j = j0 + e % ROT_SLAB;
      s_x[e] = (r < n && j < d) ? x[(size_t)r * d + j] : 0.0f;
    }
    __syncthreads();
    int jj = 0;
    for (; jj + 4 <= js; jj += 4) {
      const float r0 = s_r[(jj + 0) * ROT_LD + lane], r1 = s_r[(jj + 1) * ROT_LD + lane];
      const float r2 = s_r[(jj + 2) * ROT_LD + lane], r3 = s_r[(jj + 3) * ROT_LD + lane];
#pragma unroll
      for (int t = 0; t < ROT_STRIP; t++) {
        const f32x4 xv = *reinterpret_cast<const f32x4 *>(xs + t * ROT_SLAB + jj);
        acc[t] = acc[t] + xv.x * r0;
        acc[t] = acc[t] + xv.y * r1;
        acc[t] = acc[t] + xv.z * r2;
        acc[t] = acc[t] + xv.w * r3;
      }
    }
    for (; jj < js; jj++) {
      const float r = s_r[jj * ROT_LD + lane];
#pragma unroll
      for (int t = 0; t < ROT_STRIP; t++) acc[t] = acc[t] + xs[t * ROT_SLAB + jj] * r;
    }
  }
  const int c = c0 + lane;
  if (c < d) {
#pragma unroll
    for (int t = 0; t < ROT_STRIP; t++) {
      const long long r = row0 + wave * ROT_STRIP + t;
      if (r < n) out[(size_t)r * d + c] = acc[t];
    }
  }
}

// enqueue only: d_out = d_x * R on `st`
void rotate_launch(const float *d_x, long long n, int d, const float *d_rot, int transpose, float *d_out,
                   hipStream_t st) {
  if (n == 0) return;
  const dim3 grid((unsigned)ceil_div(n, ROT_ROWS), (unsigned)ceil_div(d, ROT_COLS));
  if (transpose) hipLaunchKernelGGL(rotate_kernel<true>, grid, dim3(ROT_THREADS), 0, st, d_x, n, d, d_rot, d_out);
  else hipLaunchKernelGGL(rotate_kernel<false>, grid, dim3(ROT_THREADS), 0, st, d_x, n, d, d_rot, d_out);
  HIP_CHECK(hipGetLastError());
}

constexpr long long ROT_MAX_ROWS = (long long)INT_MAX * ROT_ROWS;   // the row tiles are gridDim.x

// ---- moment ----------------------------------------------------------------------------------------------------
// A workgroup owns one chunk of MOMENT_ROWS rows and one MOM_TILE x MOM_TILE tile of the output (gridDim.y, gridDim.z
// walk the tiles, so any d_a, d_b work); a thread a 4 x 4 register tile of binary64 sums.  Row slabs of MOM_SLAB rows of
// a and b are staged in LDS as binary32 and widened where they are used; one staged row feeds 16 fused multiply-adds per
// thread from two ds_read_b128 (the 16 lanes of one a-column group read one address: a broadcast; the b reads of a wave
// cover one 256-byte row).  Fused or not is the same number: the product is exact.  Staged zeros outside the matrices
// add +0 and only ever meet a non-finite value in a tile entry that is not stored.
constexpr int MOMENT_ROWS = 4096;
constexpr long long MOMENT_MAX_ROWS = (long long)INT_MAX * MOMENT_ROWS;   // the chunk number is an int
constexpr int MOM_THREADS = 256, MOM_TILE = 64, MOM_SLAB = 16;
constexpr size_t MOM_SCRATCH_BYTES = (size_t)256 << 20;   // partial slabs held at a time; more chunks go in batches
constexpr int MOM_STEPS = MOM_SLAB / (MOM_THREADS / 64);   // rows of a slab one wave stages
static_assert(MOM_TILE == 64, "a wave stages one row segment: the row of a staged element is wave-uniform");

// The rows are those of a row map: position i of the chunk reads a[ra(i)] and b[rb(i)].  MAPPED false: ra(i) = rb(i) = i,
// the full-matrix moment.  MAPPED true: ra(i) = rows_a[i], rb(i) = rows_b[i], a negative row on either side stages zeros
// for both (the pair adds +0).  A wave stages one 256-byte segment of one row of a and of b per step, so the map is read
// once per wave and row (a uniform address: a scalar load).  A slab is staged in three passes over the wave's MOM_STEPS
// rows -- the map entries (read at a position clamped into the chunk, so none of the loads is conditional), the row
// segments into registers, the registers into LDS -- so that the 2 * MOM_STEPS gathered segments are in flight together
// instead of each waiting for the one before it.
template <bool MAPPED>
__global__ __launch_bounds__(MOM_THREADS) void moment_partial_kernel(const float *__restrict__ a, int da,
                                                                     const float *__restrict__ b, int db,
                                                                     const int *__restrict__ rows_a,
                                                                     const int *__restrict__ rows_b, long long n,
                                                                     int chunk0, double *__restrict__ partial) {
  __shared__ __attribute__((aligned(16))) float s_a[MOM_SLAB * MOM_TILE];
  __shared__ __attribute__((aligned(16))) float s_b[MOM_SLAB * MOM_TILE];
  const int tid = threadIdx.x, tp = tid >> 4, tq = tid & 15;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int p0 = blockIdx.y * MOM_TILE, q0 = blockIdx.z * MOM_TILE;
  const long long begin = (long long)(chunk0 + (int)blockIdx.x) * MOMENT_ROWS;
  const long long end = min(n, begin + MOMENT_ROWS);
  double acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc[i][j] = 0.0;
  for (long long r0 = begin; r0 < end; r0 += MOM_SLAB) {
    __syncthreads();
    long long ra[MOM_STEPS], rb[MOM_STEPS];   // -1: zeros
#pragma unroll
    for (int t = 0; t < MOM_STEPS; t++) {
      const long long i = r0 + wave + t * (MOM_THREADS / 64);
      if (MAPPED) {
        const long long ic = min(i, end - 1);   // r0 < end: a position of this chunk
        const int xa = rows_a[ic], xb = rows_b[ic];
        const bool live = i < end && xa >= 0 && xb >= 0;
        ra[t] = live ? xa : -1;
        rb[t] = live ? xb : -1;
      } else {
        ra[t] = rb[t] = i < end ? i : -1;
      }
    }
    float va[MOM_STEPS], vb[MOM_STEPS];
#pragma unroll
    for (int t = 0; t < MOM_STEPS; t++) {
      va[t] = (ra[t] >= 0 && p0 + lane < da) ? a[(size_t)ra[t] * da + p0 + lane] : 0.0f;
      vb[t] = (rb[t] >= 0 && q0 + lane < db) ? b[(size_t)rb[t] * db + q0 + lane] : 0.0f;
    }
#pragma unroll
    for (int t = 0; t < MOM_STEPS; t++) {
      const int e = (wave + t * (MOM_THREADS / 64)) * MOM_TILE + lane;
      s_a[e] = va[t];
      s_b[e] = vb[t];
    }
    __syncthreads();
#pragma unroll 4
    for (int rr = 0; rr < MOM_SLAB; rr++) {
      const f32x4 av = *reinterpret_cast<const f32x4 *>(s_a + rr * MOM_TILE + tp * 4);
      const f32x4 bv = *reinterpret_cast<const f32x4 *>(s_b + rr * MOM_TILE + tq * 4);
      const double ad[4] = {(double)av.x, (double)av.y, (double)av.z, (double)av.w};
      const double bd[4] = {(double)bv.x, (double)bv.y, (double)bv.z, (double)bv.w};
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = __builtin_fma(ad[i], bd[j], acc[i][j]);
    }
  }
  double *slab = partial + (size_t)blockIdx.x * da * db;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int p = p0 + tp * 4 + i;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int q = q0 + tq * 4 + j;
      if (p < da && q < db) slab[(size_t)p * db + q] = acc[i][j];
    }
  }
}

// out[e] = (first ? 0 : out[e]) + partial[0][e] + partial[1][e] + ..., one chain in ascending chunk order: batches of
// chunks continue the same chain, so the batch size changes nothing
__global__ void moment_sum_kernel(const double *__restrict__ partial, int chunks, size_t entries, int first,
                                  double *__restrict__ out) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= entries) return;
  double s = first ? 0.0 : out[e];
  for (int c = 0; c < chunks; c++) s = s + partial[(size_t)c * entries + e];
  out[e] = s;
}

void moment(const gulon_dataset *a, const gulon_dataset *b, double *out) {
  GULON_REQUIRE(a != nullptr && b != nullptr && out != nullptr, "null argument");
  GULON_REQUIRE(a->n == b->n, "the moment of %d rows with %d rows", a->n, b->n);
  moment_rows(a->x.p, a->d, b->x.p, b->d, nullptr, nullptr, a->n, out);
}

void check_rotate(long long n, int d) {
  GULON_REQUIRE(d >= 1, "bad dimension d=%d", d);
  GULON_REQUIRE(n >= 0 && n <= ROT_MAX_ROWS, "bad row count n=%lld", n);
}

}  // namespace

void moment_rows(const float *d_a, int da, const float *d_b, int db, const int *d_rows_a, const int *d_rows_b,
                 long long n, double *out) {
  GULON_REQUIRE(n >= 0 && n <= MOMENT_MAX_ROWS, "the number of rows must lie in [0, %lld], got %lld", MOMENT_MAX_ROWS, n);
  const size_t entries = (size_t)da * db;
  if (n == 0) {
    std::fill(out, out + entries, 0.0);
    return;
  }
  const int chunks = ceil_div(n, MOMENT_ROWS);
  const int batch = (int)std::min<size_t>((size_t)chunks, std::max<size_t>(MOM_SCRATCH_BYTES / (entries * sizeof(double)), 1));
  DevBuf<double> partial((size_t)batch * entries), sum(entries);
  const bool mapped = d_rows_a != nullptr;
  for (int c0 = 0; c0 < chunks; c0 += batch) {
    const int nc = std::min(batch, chunks - c0);
    const dim3 grid(nc, ceil_div(da, MOM_TILE), ceil_div(db, MOM_TILE));
    if (mapped)
      hipLaunchKernelGGL(moment_partial_kernel<true>, grid, dim3(MOM_THREADS), 0, 0, d_a, da, d_b, db, d_rows_a, d_rows_b,
                         n, c0, partial.p);
    else
      hipLaunchKernelGGL(moment_partial_kernel<false>, grid, dim3(MOM_THREADS), 0, 0, d_a, da, d_b, db, d_rows_a, d_rows_b,
                         n, c0, partial.p);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(moment_sum_kernel, dim3(ceil_div((long long)entries, 256)), dim3(256), 0, 0, partial.p, nc,
                       entries, c0 == 0 ? 1 : 0, sum.p);
    HIP_CHECK(hipGetLastError());
  }
  sum.download(out, entries);
  HIP_CHECK(hipDeviceSynchronize());
}

}  // namespace gulon

using namespace gulon;

GULON_API int32_t gulon_dataset_rotate(const gulon_dataset *ds, const float *rotation, int32_t transpose,
                                       gulon_dataset **out) {
  return guarded([&] {
    GULON_REQUIRE(out != nullptr, "out is null");
    *out = nullptr;
    GULON_REQUIRE(ds != nullptr && rotation != nullptr, "null argument");
    check_rotate(ds->n, ds->d);
    std::unique_ptr<gulon_dataset> g(new gulon_dataset());
    g->n = ds->n; g->d = ds->d;
    g->x.alloc(std::max<size_t>((size_t)ds->n * ds->d, 1));
    if (ds->n) {
      DevBuf<float> rot;
      rot.upload(rotation, (size_t)ds->d * ds->d);
      rotate_launch(ds->x.p, ds->n, ds->d, rot.p, transpose, g->x.p, nullptr);
      HIP_CHECK(hipDeviceSynchronize());
    }
    *out = g.release();
  });
}

GULON_API int32_t gulon_rotate_rows(const float *x, int32_t n, int32_t d, const float *rotation, int32_t transpose,
                                    float *out) {
  return guarded([&] {
    check_rotate(n, d);
    GULON_REQUIRE(rotation != nullptr && ((x != nullptr && out != nullptr) || n == 0), "null argument");
    if (n == 0) return;
    const size_t total = (size_t)n * d;
    DevBuf<float> dx, rot, dout(total);
    dx.upload(x, total);
    rot.upload(rotation, (size_t)d * d);
    rotate_launch(dx.p, n, d, rot.p, transpose, dout.p, nullptr);
    dout.download(out, total);
    HIP_CHECK(hipDeviceSynchronize());
  });
}

GULON_API int32_t gulon_rotate_rows_dev(const float *d_x, int64_t n, int32_t d, const float *d_rotation,
                                        int32_t transpose, float *d_out, void *stream) {
  return guarded([&] {
    check_rotate(n, d);
    GULON_REQUIRE(d_rotation != nullptr && ((d_x != nullptr && d_out != nullptr) || n == 0), "null argument");
    GULON_REQUIRE(d_x != d_out || n == 0, "the rotation is not done in place");
    rotate_launch(d_x, n, d, d_rotation, transpose, d_out, (hipStream_t)stream);
  });
}

GULON_API int32_t gulon_dataset_moment(const gulon_dataset *a, const gulon_dataset *b, double *out) {
  return guarded([&] { moment(a, b, out); });
}
