// Expressions over the rows of a dataset: compose.hip's composed vector with v_t = row row_t of the
// dataset in the place of Index.lookup -- the true vectors asked `king - man + woman`.  The accumulate and normalise
// steps are compose.hpp's compose_terms, shared with compose_rows_kernel: the same order of binary32 operations, which
// expressions.compose_reference restates.
#include "compose.hpp"

namespace gulon {
namespace {

template <int CPT>
__global__ __launch_bounds__(CR_THREADS) void dataset_compose_kernel(
    const float *__restrict__ X, int n, int d, const int *__restrict__ term_offsets, const int *__restrict__ term_rows,
    const float *__restrict__ term_weights, int normalize_terms, int normalize_query, float *__restrict__ out,
    int *__restrict__ err) {
  extern __shared__ float xs[];   // [d], and [d] more when terms are normalised
  const int b = blockIdx.x;
  const int t0 = term_offsets[b], t1 = term_offsets[b + 1];
  float *o = out + (size_t)b * d;
  if (terms_unusable(term_rows, t0, t1, n)) {   // (uniform over the workgroup: no barrier is skipped by a part of it)
    write_nan_vector(o, d, threadIdx.x, err);
    return;
  }
  compose_terms<CPT>(t0, t1, term_rows, term_weights, d, normalize_terms, normalize_query, xs, o, [&](int row) {
    const float *x = X + (size_t)row * d;
    return [x](int e) { return x[e]; };
  });
}

}  // namespace

void launch_dataset_compose(const gulon_dataset *ds, const int *d_off, const int *d_rows, const float *d_w, int b,
                            bool norm_terms, bool norm_query, float *d_out, int *d_err, hipStream_t st) {
  GULON_REQUIRE(b >= 0, "batch size must be non-negative");
  GULON_UNSUPPORTED((size_t)ds->d * sizeof(float) > 64 * 1024, "d = %d: a row does not fit in LDS", ds->d);
  if (b == 0) return;
  GULON_REQUIRE(d_off != nullptr && d_rows != nullptr && d_w != nullptr && d_out != nullptr, "null argument");
  const size_t lds = compose_lds_bytes(ds->d, norm_terms, norm_query);
#define DC(CPT) hipLaunchKernelGGL(dataset_compose_kernel<CPT>, dim3(b), dim3(CR_THREADS), lds, st, ds->x.p, ds->n, \
                                   ds->d, d_off, d_rows, d_w, norm_terms ? 1 : 0, norm_query ? 1 : 0, d_out, d_err)
  if (ds->d <= CR_THREADS) DC(1);
  else if (ds->d <= 4 * CR_THREADS) DC(4);
  else if (ds->d <= 16 * CR_THREADS) DC(16);
  else {
    if (lds > 64 * 1024)   // xs and ys of a row above 8192 coordinates: more than the default dynamic LDS of a launch
      HIP_CHECK(hipFuncSetAttribute((const void *)dataset_compose_kernel<64>,
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    DC(64);
  }
#undef DC
  HIP_CHECK(hipGetLastError());
}

}  // namespace gulon

using namespace gulon;

GULON_API int32_t gulon_dataset_compose_rows_dev(const gulon_dataset *ds, const int32_t *d_term_offsets,
                                                 const int32_t *d_term_rows, const float *d_term_weights, int32_t b,
                                                 int32_t normalize_terms, int32_t normalize_query, float *d_out,
                                                 int32_t *d_err, void *stream) {
  return guarded([&] {
    GULON_REQUIRE(ds != nullptr, "dataset is null");
    launch_dataset_compose(ds, d_term_offsets, d_term_rows, d_term_weights, b, normalize_terms != 0,
                           normalize_query != 0, d_out, d_err, (hipStream_t)stream);
  });
}

GULON_API int32_t gulon_dataset_compose_rows(const gulon_dataset *ds, const int32_t *term_offsets,
                                             const int32_t *term_rows, const float *term_weights, int32_t b,
                                             int32_t normalize_terms, int32_t normalize_query, float *out) {
  return guarded([&] {
    GULON_REQUIRE(ds != nullptr, "dataset is null");
    const int terms = check_terms_host(term_offsets, term_rows, term_weights, b, ds->n);
    GULON_UNSUPPORTED((size_t)ds->d * sizeof(float) > 64 * 1024, "d = %d: a row does not fit in LDS", ds->d);
    if (b == 0) return;
    GULON_REQUIRE(out != nullptr, "null argument");
    DevBuf<int> off, rows;
    DevBuf<float> w, q((size_t)b * ds->d);
    off.upload(term_offsets, (size_t)b + 1);
    rows.upload(term_rows, (size_t)terms);
    w.upload(term_weights, (size_t)terms);
    launch_dataset_compose(ds, off.p, rows.p, w.p, b, normalize_terms != 0, normalize_query != 0, q.p, nullptr, nullptr);
    q.download(out, (size_t)b * ds->d);
    HIP_CHECK(hipStreamSynchronize(nullptr));
  });
}
