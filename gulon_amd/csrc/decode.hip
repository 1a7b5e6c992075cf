// Decoding rows of a device-resident PQIndex back into vectors, on the device:
//   ProductQuantizer.decode(EncodedVector) (ProductQuantizer.scala:37-50)  -- decode_rows_kernel
//   GroupedIndex.lookup (Index.scala:247-253)                               -- the same kernel with a group base
//   MathUtils.normalize (MathUtils.scala:100-120), fused behind a flag        -- for cosine query-by-row
//   ProductQuantizer.decode(EncodedMatrix) (ProductQuantizer.scala:58-78)  -- decode_range_kernel (bandwidth-bound)
// A decoded coordinate is a copy of a codebook entry (plus one fp32 add for the grouped lookup), so results are
// bit-exact by construction.  Codes are read in the layout the handle already keeps, through row_decode.hpp (shared with
// compose.hip, inspect.hip and fine.hip): decode_rows_kernel reads single codes (CodeSrc), decode_range_kernel a block
// staged in LDS (StagedCodes).  Neither clamps a code to the code book.
#include "normalize.hpp"
#include "row_decode.hpp"

namespace gulon {
namespace {

// One workgroup (one wavefront) per requested row.  gcent != nullptr: GroupedIndex.lookup, base = the centroid of
// the partition the reference's binarySearch over the raw offsets names, out = base + decode(row) (MathUtils.add,
// MathUtils.scala:63-71).  normalize: MathUtils.normalize of the result.  A row outside [0, n) gives an all-NaN
// vector and sets *err (nothing is read for it).
__global__ __launch_bounds__(64) void decode_rows_kernel(CodeSrc src, const float *__restrict__ cents, int n, int d, int k,
                                                         const int *__restrict__ rows, const float *__restrict__ gcent,
                                                         const int *__restrict__ offsets, int n_offsets, int normalize,
                                                         float *__restrict__ out, int *__restrict__ err) {
  extern __shared__ float xs[];   // [d]
  const int r = blockIdx.x, lane = threadIdx.x;
  const int row = rows[r];
  float *o = out + (size_t)r * d;
  if (row < 0 || row >= n) {
    for (int e = lane; e < d; e += 64) o[e] = __int_as_float(0x7FC00000);
    if (lane == 0 && err) *err = 1;
    return;
  }
  const SubvectorMap sv(d, src.m);
  const float *base = gcent ? lookup_base(gcent, offsets, n_offsets, row, d) : nullptr;
  for (int e = lane; e < d; e += 64) xs[e] = decoded_coordinate(src, sv, cents, k, row, e, base);
  if (!normalize) {
    for (int e = lane; e < d; e += 64) o[e] = xs[e];
    return;
  }
  __syncthreads();
  normalize_staged_row(xs, d, lane, 64, o);
}

// Rows [from, until) into out[(i - from) * d + e].  One workgroup per 64-row block: the block's codes are staged in LDS
// once (StagedCodes), then the block's slice of the output -- contiguous in row-major order -- is written with
// 16-byte stores, consecutive lanes on consecutive addresses (VEC4: d % 4 == 0, so a float4 never spans two rows and
// every row starts 16-byte aligned).  Centroids are read through the caches (k * d * 4 bytes).
constexpr int DR_THREADS = 256;
template <bool WIDE, bool VEC4>
__global__ __launch_bounds__(DR_THREADS) void decode_range_kernel(CodeSrc src, const float *__restrict__ cents, int d,
                                                                  int k, int from, int until, int rb0,
                                                                  float *__restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lcode[];
  const int rb = rb0 + blockIdx.x;
  const int tid = threadIdx.x;
  const int m = src.m;
  const StagedCodes<WIDE> staged{lcode, src.vec};
  staged.stage(src, rb, tid, DR_THREADS);
  __syncthreads();
  const int r_lo = max(rb * 64, from), r_hi = min(rb * 64 + 64, until);
  const SubvectorMap sv(d, m);
  auto value = [&](int l, int e) -> float {
    const int j = sv.quantizer(e), fr = sv.from(j), sj = sv.sdim(j);
    return cents[(size_t)k * fr + (size_t)staged.code(l, j) * sj + (e - fr)];
  };
  float *o = out + (size_t)(r_lo - from) * d;
  const int total = (r_hi - r_lo) * d;          // floats of this block's output
  const int l0 = r_lo - rb * 64;
  if (VEC4) {
    for (int f = tid * 4; f < total; f += DR_THREADS * 4) {
      const int l = l0 + f / d, e = f % d;
      f32x4 v;
      v.x = value(l, e); v.y = value(l, e + 1); v.z = value(l, e + 2); v.w = value(l, e + 3);
      *(gptr<f32x4>)as_global(o + f) = v;
    }
  } else {
    for (int f = tid; f < total; f += DR_THREADS) o[f] = value(l0 + f / d, f % d);
  }
}

void check_rows_host(const gulon_index *ix, const int32_t *rows, int b) {
  for (int r = 0; r < b; r++)
    GULON_REQUIRE(rows[r] >= 0 && rows[r] < ix->n, "row %d = %d outside [0, %d)", r, rows[r], ix->n);
}

}  // namespace

void ensure_row_err(gulon_index *ix) {
  if (ix->row_err.n) return;
  ix->row_err.alloc(1);
  HIP_CHECK(hipMemset(ix->row_err.p, 0, sizeof(int)));
  // the memset runs on the null stream, which the caller's (non-blocking) stream does not wait for: it must have landed
  // before a kernel on that stream can set the word.  Once per handle, and every handle has its word from the moment it
  // is made (gulon_index_create, make_context, build_view, the roots of update.hip): the wait below can last as long as
  // the work of ANOTHER stream that shares a hardware queue with the null stream, which a *_dev call documented not to
  // synchronise must not pay for.  The calls in the *_dev paths are the guard for a handle made any other way
  HIP_CHECK(hipStreamSynchronize(nullptr));
}

int take_row_err(gulon_index *ix) {
  int v = 0;
  if (ix->row_err.n == 0) return 0;
  HIP_CHECK(hipDeviceSynchronize());
  HIP_CHECK(hipMemcpy(&v, ix->row_err.p, sizeof(int), hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemset(ix->row_err.p, 0, sizeof(int)));
  HIP_CHECK(hipStreamSynchronize(nullptr));   // cleared before the next call's kernels, whatever their stream
  return v;
}

void launch_decode_rows(const gulon_index *ix, const int *d_rows, int b, const float *gcent, const int *offsets,
                        int n_offsets, bool normalize, float *d_out, int *d_err, hipStream_t st) {
  GULON_REQUIRE(b >= 0, "batch size must be non-negative");
  GULON_UNSUPPORTED((size_t)ix->d * sizeof(float) > 64 * 1024, "d = %d: a decoded row does not fit in LDS", ix->d);
  if (b == 0) return;
  GULON_REQUIRE(d_rows != nullptr && d_out != nullptr, "null argument");
  hipLaunchKernelGGL(decode_rows_kernel, dim3(b), dim3(64), (size_t)ix->d * sizeof(float), st, code_src(ix), ix->cents.p,
                     ix->n, ix->d, ix->k, d_rows, gcent, offsets, n_offsets, normalize ? 1 : 0, d_out, d_err);
  HIP_CHECK(hipGetLastError());
}

void launch_decode_range(const gulon_index *ix, int from, int until, float *d_out, hipStream_t st) {
  GULON_REQUIRE(0 <= from && from <= until && until <= ix->n, "expected: 0 <= from <= until <= length");
  if (from == until) return;
  const int rb0 = from / 64, nrb = ceil_div(until, 64) - rb0;
  const size_t lds = block_code_bytes(ix);
  GULON_UNSUPPORTED(lds > 64 * 1024, "m = %d: one row block's codes do not fit in LDS", ix->m);
  dispatch_flags(ix->wide, ix->d % 4 == 0, [&](auto wide, auto vec4) {
    hipLaunchKernelGGL((decode_range_kernel<wide.value, vec4.value>), dim3(nrb), dim3(DR_THREADS), lds, st, code_src(ix),
                       ix->cents.p, ix->d, ix->k, from, until, rb0, d_out);
  });
  HIP_CHECK(hipGetLastError());
}

void decode_rows_host(const gulon_index *ix, DevBuf<int> &rows_buf, DevBuf<float> &out_buf, const int32_t *rows, int b,
                      const float *gcent, const int *offsets, int n_offsets, bool normalize, float *out,
                      hipStream_t st) {
  GULON_REQUIRE(b >= 0, "batch size must be non-negative");
  GULON_REQUIRE(b == 0 || (rows != nullptr && out != nullptr), "null argument");
  check_rows_host(ix, rows, b);
  if (b == 0) return;
  rows_buf.upload(rows, (size_t)b, st);
  out_buf.ensure((size_t)b * ix->d);
  launch_decode_rows(ix, rows_buf.p, b, gcent, offsets, n_offsets, normalize, out_buf.p, nullptr, st);
  out_buf.download(out, (size_t)b * ix->d, st);
  HIP_CHECK(hipStreamSynchronize(st));
}

}  // namespace gulon

using namespace gulon;

GULON_API int32_t gulon_index_decode_rows(gulon_index *idx, const int32_t *rows, int32_t b, int32_t normalize,
                                          float *out) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    std::lock_guard<std::mutex> lock(idx->mu);
    idx->pend_b = -1;
    StreamOrder so(idx, nullptr);
    decode_rows_host(idx, idx->stage_rows, idx->stage_q, rows, b, nullptr, nullptr, 0, normalize != 0, out, nullptr);
    so.done();
  });
}

GULON_API int32_t gulon_index_decode_rows_dev(gulon_index *idx, const int32_t *d_rows, int32_t b, int32_t normalize,
                                              float *d_out, void *stream) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    std::lock_guard<std::mutex> lock(idx->mu);
    ensure_row_err(idx);
    launch_decode_rows(idx, d_rows, b, nullptr, nullptr, 0, normalize != 0, d_out, idx->row_err.p, (hipStream_t)stream);
  });
}

GULON_API int32_t gulon_index_decode_dataset(gulon_index *idx, int32_t from, int32_t until, gulon_dataset **out) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr && out != nullptr, "null argument");
    *out = nullptr;
    GULON_REQUIRE(0 <= from && from <= until && until <= idx->n, "expected: 0 <= from <= until <= length");
    std::lock_guard<std::mutex> lock(idx->mu);
    std::unique_ptr<gulon_dataset> ds(new gulon_dataset());
    ds->n = until - from; ds->d = idx->d;
    ds->x.alloc(std::max<size_t>((size_t)ds->n * ds->d, 1));
    StreamOrder so(idx, nullptr);
    launch_decode_range(idx, from, until, ds->x.p, nullptr);
    so.done();
    HIP_CHECK(hipStreamSynchronize(nullptr));
    *out = ds.release();
  });
}

GULON_API int32_t gulon_index_row_error(gulon_index *idx, int32_t *out) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr && out != nullptr, "null argument");
    std::lock_guard<std::mutex> lock(idx->mu);
    *out = take_row_err(idx);
  });
}
