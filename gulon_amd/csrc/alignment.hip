// Learning the map between two embedding spaces (alignment.py): the two device steps of MUSE's supervised
// recipe (Conneau et al. 2018, "Word translation without parallel data") that the rest of the library does not have yet.
// Neither is a Scala method: the reference aligns nothing.
//   pair moment   out[p][q] = sum_i a[rows_a[i]][p] * b[rows_b[i]][q] in binary64 over a list of row pairs of two
//                 datasets -- the matrix an orthogonal Procrustes solve takes its SVD of.  It is rotate.hip's moment with
//                 its staging step reading through a row map (moment_rows, moment.hpp): the same accumulate body, the
//                 same chunks of 4096 positions summed i ascending, the same ascending chain of chunk sums, no
//                 floating-point atomics.  A pair with a negative row on either side stages zeros and is not counted:
//                 the match list of a refinement round holds -1 for unmatched rows and never has to be compacted.
//                                                                              -- pair_used_kernel counts the live pairs
//   mutual rows   out[s] = fwd[s] if 0 <= fwd[s] < nt and bwd[fwd[s]] == s, else -1: the pairs that are each other's
//                 best match, elementwise, nothing compacted                                     -- mutual_rows_kernel
#include "moment.hpp"

namespace gulon {
namespace {

constexpr int AL_THREADS = 256;
constexpr int AL_MAX_BLOCKS = 1024;   // pair_used_kernel strides over longer lists

// *used += the positions whose two rows are both non-negative: integer atomics, one per wave, so the order is immaterial
__global__ __launch_bounds__(AL_THREADS) void pair_used_kernel(const int *__restrict__ rows_a,
                                                               const int *__restrict__ rows_b, long long n,
                                                               unsigned long long *__restrict__ used) {
  const long long stride = (long long)gridDim.x * AL_THREADS;
  unsigned long long mine = 0;
  for (long long i = (long long)blockIdx.x * AL_THREADS + threadIdx.x; i < n; i += stride)
    mine += (rows_a[i] >= 0 && rows_b[i] >= 0) ? 1 : 0;
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o, 64);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(used, mine);
}

__global__ __launch_bounds__(AL_THREADS) void mutual_rows_kernel(const int *__restrict__ fwd, int ns,
                                                                 const int *__restrict__ bwd, int nt,
                                                                 int *__restrict__ out) {
  const int s = blockIdx.x * AL_THREADS + threadIdx.x;
  if (s >= ns) return;
  const int t = fwd[s];
  out[s] = (t >= 0 && t < nt && bwd[t] == s) ? t : -1;
}

void check_mutual_args(const void *fwd, int ns, const void *bwd, int nt, const void *out) {
  GULON_REQUIRE(ns >= 0 && nt >= 0, "the numbers of rows must be non-negative, got %d and %d", ns, nt);
  GULON_REQUIRE(ns == 0 || (fwd != nullptr && out != nullptr), "null argument");
  GULON_REQUIRE(nt == 0 || bwd != nullptr, "null argument");
}

// enqueue only
void launch_mutual_rows(const int *d_fwd, int ns, const int *d_bwd, int nt, int *d_out, hipStream_t st) {
  if (ns == 0) return;
  hipLaunchKernelGGL(mutual_rows_kernel, dim3(ceil_div(ns, AL_THREADS)), dim3(AL_THREADS), 0, st, d_fwd, ns, d_bwd, nt,
                     d_out);
  HIP_CHECK(hipGetLastError());
}

void check_pair_moment_args(const gulon_dataset *a, const gulon_dataset *b, const void *rows_a, const void *rows_b,
                            long long n, const void *out, const void *out_used) {
  GULON_REQUIRE(a != nullptr && b != nullptr && out != nullptr && out_used != nullptr, "null argument");
  GULON_REQUIRE(n >= 0, "the number of pairs must be non-negative, got %lld", n);
  GULON_REQUIRE(n == 0 || (rows_a != nullptr && rows_b != nullptr), "null argument");
}

// Device lists, host results; null stream, returns after the results have arrived
void pair_moment(const gulon_dataset *a, const gulon_dataset *b, const int *d_rows_a, const int *d_rows_b, long long n,
                 double *out, int64_t *out_used) {
  static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the count is added as an unsigned word");
  *out_used = 0;
  if (n == 0) {
    moment_rows(a->x.p, a->d, b->x.p, b->d, nullptr, nullptr, 0, out);
    return;
  }
  DevBuf<unsigned long long> used(1);
  HIP_CHECK(hipMemsetAsync(used.p, 0, sizeof(unsigned long long), nullptr));
  const int blocks = (int)std::min<long long>(AL_MAX_BLOCKS, (n + AL_THREADS - 1) / AL_THREADS);
  hipLaunchKernelGGL(pair_used_kernel, dim3(blocks), dim3(AL_THREADS), 0, 0, d_rows_a, d_rows_b, n, used.p);
  HIP_CHECK(hipGetLastError());
  used.download((unsigned long long *)out_used, 1);
  moment_rows(a->x.p, a->d, b->x.p, b->d, d_rows_a, d_rows_b, n, out);   // waits for the null stream
}

}  // namespace
}  // namespace gulon

using namespace gulon;

GULON_API int32_t gulon_dataset_pair_moment(const gulon_dataset *a, const gulon_dataset *b, const int32_t *rows_a,
                                            const int32_t *rows_b, int64_t n, double *out, int64_t *out_used) {
  return guarded([&] {
    check_pair_moment_args(a, b, rows_a, rows_b, n, out, out_used);
    for (int64_t i = 0; i < n; i++)
      GULON_REQUIRE(rows_a[i] < a->n && rows_b[i] < b->n, "pair %lld = (%d, %d) beyond the %d and %d rows", (long long)i,
                    rows_a[i], rows_b[i], a->n, b->n);
    DevBuf<int> da, db;
    da.upload(rows_a, (size_t)n);
    db.upload(rows_b, (size_t)n);
    pair_moment(a, b, da.p, db.p, n, out, out_used);
  });
}

GULON_API int32_t gulon_dataset_pair_moment_dev(const gulon_dataset *a, const gulon_dataset *b, const int32_t *d_rows_a,
                                                const int32_t *d_rows_b, int64_t n, double *out, int64_t *out_used) {
  return guarded([&] {
    check_pair_moment_args(a, b, d_rows_a, d_rows_b, n, out, out_used);
    pair_moment(a, b, d_rows_a, d_rows_b, n, out, out_used);
  });
}

GULON_API int32_t gulon_mutual_rows(const int32_t *fwd, int32_t ns, const int32_t *bwd, int32_t nt, int32_t *out) {
  return guarded([&] {
    check_mutual_args(fwd, ns, bwd, nt, out);
    if (ns == 0) return;
    DevBuf<int> dfwd, dbwd, dout((size_t)ns);
    dfwd.upload(fwd, (size_t)ns);
    dbwd.upload(bwd, (size_t)nt);
    launch_mutual_rows(dfwd.p, ns, dbwd.p, nt, dout.p, nullptr);
    dout.download(out, (size_t)ns);
    HIP_CHECK(hipStreamSynchronize(nullptr));
  });
}

GULON_API int32_t gulon_mutual_rows_dev(const int32_t *d_fwd, int32_t ns, const int32_t *d_bwd, int32_t nt,
                                        int32_t *d_out, void *stream) {
  return guarded([&] {
    check_mutual_args(d_fwd, ns, d_bwd, nt, d_out);
    launch_mutual_rows(d_fwd, ns, d_bwd, nt, d_out, (hipStream_t)stream);
  });
}
