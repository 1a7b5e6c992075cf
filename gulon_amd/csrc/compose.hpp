// What the expression calls share (DESIGN.md "Expression queries", 9u): the accumulate and normalise steps of a composed
// vector, whatever a term row is read from -- an index's decoded rows (compose.hip) or a dataset's rows
// (dataset_compose.hip) -- the kernel that drops the operands from an answer, and the host-side check of a CSR term list.
#pragma once
#include "normalize.hpp"

namespace gulon {

constexpr int CR_THREADS = 256;

// An expression without terms, or with a term row outside [0, n): uniform over the workgroup.
__device__ __forceinline__ bool terms_unusable(const int *__restrict__ term_rows, int t0, int t1, int n) {
  bool bad = t1 <= t0;
  for (int t = t0; t < t1; t++) {
    const int row = term_rows[t];
    bad = bad || row < 0 || row >= n;
  }
  return bad;
}

// ... comes back as an all-NaN vector and sets *err (nullable); nothing is read for it.
__device__ __forceinline__ void write_nan_vector(float *__restrict__ o, int d, int tid, int *__restrict__ err) {
  for (int e = tid; e < d; e += CR_THREADS) o[e] = __int_as_float(0x7FC00000);
  if (tid == 0 && err) *err = 1;
}

// One workgroup of CR_THREADS composes terms [t0, t1) into o[d]; thread t owns coordinates t, t + 256, ... (CPT of
// them: d <= 256 * CPT) and keeps their running sums in registers:
//   acc = w_0 * v_0[e];  acc = acc + (w_t * v_t[e])  for t = 1, 2, ... in list order,
// every product and every sum a binary32 operation of its own.  read_row(row) gives the reader of that row's
// coordinates, v = reader(e).  A term is staged in LDS only where it is normalised: xs[d] the row, ys = xs + d its
// normalised form (normalize_staged_row reads all of xs in every thread, so it cannot write in place).  The composed
// vector goes through xs for the final normalisation.  Every thread of the workgroup must call (barriers inside).
template <int CPT, class ReadRow>
__device__ __forceinline__ void compose_terms(int t0, int t1, const int *__restrict__ term_rows,
                                              const float *__restrict__ term_weights, int d, int normalize_terms,
                                              int normalize_query, float *xs, float *__restrict__ o, ReadRow read_row) {
  float *ys = xs + d;
  const int tid = threadIdx.x;
  float acc[CPT];
  for (int t = t0; t < t1; t++) {
    const float w = term_weights[t];
    const auto coordinate = read_row(term_rows[t]);
    float v[CPT];
#pragma unroll
    for (int i = 0; i < CPT; i++) {
      const int e = tid + i * CR_THREADS;
      v[i] = e < d ? coordinate(e) : 0.f;
    }
    if (normalize_terms) {
#pragma unroll
      for (int i = 0; i < CPT; i++) {
        const int e = tid + i * CR_THREADS;
        if (e < d) xs[e] = v[i];
      }
      __syncthreads();
      normalize_staged_row(xs, d, tid, CR_THREADS, ys);
#pragma unroll
      for (int i = 0; i < CPT; i++) {   // (its own writes: ys[tid], ys[tid + 256], ...)
        const int e = tid + i * CR_THREADS;
        if (e < d) v[i] = ys[e];
      }
      __syncthreads();   // every thread has summed xs before the next term overwrites it
    }
#pragma unroll
    for (int i = 0; i < CPT; i++) {
      const float p = __fmul_rn(w, v[i]);
      acc[i] = t == t0 ? p : __fadd_rn(acc[i], p);
    }
  }
  if (!normalize_query) {
#pragma unroll
    for (int i = 0; i < CPT; i++) {
      const int e = tid + i * CR_THREADS;
      if (e < d) o[e] = acc[i];
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < CPT; i++) {
    const int e = tid + i * CR_THREADS;
    if (e < d) xs[e] = acc[i];
  }
  __syncthreads();
  normalize_staged_row(xs, d, tid, CR_THREADS, o);
}

// dynamic LDS of a compose launch: xs, and ys where terms are normalised
inline size_t compose_lds_bytes(int d, bool norm_terms, bool norm_query) {
  return (size_t)d * sizeof(float) * (norm_terms ? 2 : norm_query ? 1 : 0);
}

// compose.hip: one wavefront per query drops the term rows from an answer of depth kin and keeps the first k_nn.
__global__ __launch_bounds__(64) void drop_rows_kernel(const int *__restrict__ in_idx, const float *__restrict__ in_dist,
                                                       const int *__restrict__ in_count, int kin, int k_nn,
                                                       const int *__restrict__ term_offsets,
                                                       const int *__restrict__ term_rows, int row_base,
                                                       int *__restrict__ out_idx, float *__restrict__ out_dist,
                                                       int *__restrict__ out_count);
void launch_drop(const int *in_idx, const float *in_dist, const int *in_count, int b, int kin, int k_nn,
                 const int *d_off, const int *d_rows, int row_base, int *out_idx, float *out_dist, int *out_count,
                 hipStream_t st);
// The host-pointer forms check everything before anything is launched; returns the number of terms.
int check_terms_host(const int32_t *off, const int32_t *rows, const float *w, int b, int n);
// dataset_compose.hip: expressions over the rows of a dataset -> d_out [b][d], on `st` (d_err nullable)
void launch_dataset_compose(const gulon_dataset *ds, const int *d_off, const int *d_rows, const float *d_w, int b,
                            bool norm_terms, bool norm_query, float *d_out, int *d_err, hipStream_t st);

}  // namespace gulon
