// Index views: a chosen subset of an index's rows as an index of its own, built on the device.
//
// A view of P over rows r_0 < r_1 < ... < r_{s-1} is the PQIndex over the EncodedMatrix whose columns are those rows, in
// that order: its code buffers are gathered from P's, it owns a copy of the codebooks, and it keeps the map p -> r_p so
// that the view-query entries can answer in P's row ids.  No scan kernel knows about views.
//
// A view gathers from one parent, in ascending order.  update.hip has the rest: gulon_index_merge gathers from two
// sources in any order into a root index, gulon_index_encode_dataset fills a code buffer from new vectors, and
// gulon_index_get_codes is the accessor for an index's plain code buffer (a view's included).
//
// Kernels
//   mask_to_rows_count    bit mask -> per word the prefix of its popcount inside its 64-word group, per group the sum
//   mask_to_rows_groups   exclusive scan over the group sums (one workgroup), and the total s
//   mask_to_rows_scatter  one wave per mask word, lane = bit: row r lands at prefix + popcount of the lower bits
//   gather_codes<VEC>     [n/64][ng][64][VEC] of the parent -> [ceil(s/64)][ng][64][VEC] of the view
//   gather_wcodes         the same for the wide layout [n/64][m][64] of uint16
//   compose_map_kernel    the map of a view of a view: rows of the root
//   map_rows_kernel       [count] positions -> row ids of the root, in place; negative entries (padding) kept
#include "scan.hpp"

namespace gulon {
namespace {

// word w of the mask with the bits at or above row n cleared
__device__ __forceinline__ unsigned long long mask_word(const unsigned long long *__restrict__ mask, int w, int n) {
  unsigned long long x = mask[w];
  const long long left = (long long)n - (long long)w * 64;   // >= 1 for every word the callers read
  if (left < 64) x &= (1ull << left) - 1ull;
  return x;
}

__device__ __forceinline__ int wave_inclusive_sum(int c, int lane) {
  int inc = c;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  return inc;
}

__global__ __launch_bounds__(64) void mask_to_rows_count(const unsigned long long *__restrict__ mask, int n, int nwords,
                                                         int *__restrict__ wprefix, int *__restrict__ gsum) {
  const int lane = threadIdx.x;
  const int w = blockIdx.x * 64 + lane;
  const int c = w < nwords ? __popcll(mask_word(mask, w, n)) : 0;
  const int inc = wave_inclusive_sum(c, lane);
  if (w < nwords) wprefix[w] = inc - c;
  if (lane == 63) gsum[blockIdx.x] = inc;
}

__global__ __launch_bounds__(1024) void mask_to_rows_groups(const int *__restrict__ gsum, int ngroups,
                                                            int *__restrict__ gprefix, int *__restrict__ total) {
  __shared__ int wsum[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int carry = 0;
  for (int base = 0; base < ngroups; base += 1024) {
    const int g = base + tid;
    const int c = g < ngroups ? gsum[g] : 0;
    const int inc = wave_inclusive_sum(c, lane);
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int before = 0, all = 0;
    for (int i = 0; i < 16; i++) {
      const int v = wsum[i];
      if (i < wave) before += v;
      all += v;
    }
    if (g < ngroups) gprefix[g] = carry + before + inc - c;
    carry += all;
    __syncthreads();
  }
  if (tid == 0) *total = carry;
}

__global__ __launch_bounds__(256) void mask_to_rows_scatter(const unsigned long long *__restrict__ mask, int n, int nwords,
                                                            const int *__restrict__ wprefix,
                                                            const int *__restrict__ gprefix, int s,
                                                            int *__restrict__ rows) {
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= nwords) return;
  const unsigned long long x = mask_word(mask, w, n);
  if (!((x >> lane) & 1ull)) return;
  const int pos = gprefix[w >> 6] + wprefix[w] + __popcll(x & ((1ull << lane) - 1ull));
  if (pos < s) rows[pos] = w * 64 + lane;   // (s: a mask rewritten between the count and the scatter stays in bounds)
}

// lanes past the view's last row get what relayout_codes gives padding rows: zero words
template <int VEC>
__global__ void gather_codes(const typename CodeWord<VEC>::type *__restrict__ src, const int *__restrict__ rows, int s,
                             int ng, typename CodeWord<VEC>::type *__restrict__ dst, long long total /* nblk*ng*64 */) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int lane = (int)(t & 63);
  const long long bg = t >> 6;
  const int g = (int)(bg % ng);
  const long long p = (bg / ng) * 64 + lane;
  typename CodeWord<VEC>::type w{};
  if (p < s) {
    const int r = rows[p];
    w = src[((size_t)(r >> 6) * ng + g) * 64 + (r & 63)];
  }
  dst[t] = w;
}

__global__ void gather_wcodes(const uint16_t *__restrict__ src, const int *__restrict__ rows, int s, int m,
                              uint16_t *__restrict__ dst, long long total /* nblk*m*64 */) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int lane = (int)(t & 63);
  const long long bj = t >> 6;
  const int j = (int)(bj % m);
  const long long p = (bj / m) * 64 + lane;
  uint16_t v = 0;
  if (p < s) {
    const int r = rows[p];
    v = src[((size_t)(r >> 6) * m + j) * 64 + (r & 63)];
  }
  dst[t] = v;
}

__global__ void compose_map_kernel(const int *__restrict__ outer, const int *__restrict__ rows, int s,
                                   int *__restrict__ out) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p < s) out[p] = outer[rows[p]];
}

__global__ void map_rows_kernel(const int *__restrict__ map, int s, int base, int *__restrict__ idx, long long count) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count) return;
  const int p = idx[t];
  if (p >= 0 && p < s) idx[t] = base + map[p];
}

// mask (device, ceil(n/64) words) -> ascending rows; synchronises once for s
int mask_to_rows(const unsigned long long *d_mask, int n, DevBuf<int> &rows) {
  if (n <= 0) return 0;
  const int nwords = ceil_div(n, 64), ngroups = ceil_div(nwords, 64);
  DevBuf<int> wprefix((size_t)nwords), gsum((size_t)ngroups), gprefix((size_t)ngroups), total(1);
  hipLaunchKernelGGL(mask_to_rows_count, dim3(ngroups), dim3(64), 0, 0, d_mask, n, nwords, wprefix.p, gsum.p);
  hipLaunchKernelGGL(mask_to_rows_groups, dim3(1), dim3(1024), 0, 0, gsum.p, ngroups, gprefix.p, total.p);
  HIP_CHECK(hipGetLastError());
  int s = 0;
  HIP_CHECK(hipMemcpy(&s, total.p, sizeof(int), hipMemcpyDeviceToHost));
  if (s > 0) {
    rows.alloc((size_t)s);
    hipLaunchKernelGGL(mask_to_rows_scatter, dim3(ceil_div(nwords, 4)), dim3(256), 0, 0, d_mask, n, nwords, wprefix.p,
                       gprefix.p, s, rows.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());   // the prefix buffers go out of scope
  }
  return s;
}

template <class T>
void copy_dev(DevBuf<T> &dst, const DevBuf<T> &src, size_t count) {
  dst.alloc(count);
  if (count) HIP_CHECK(hipMemcpy(dst.p, src.p, count * sizeof(T), hipMemcpyDeviceToDevice));
}

// The view of `P` over `rows` (device, s entries, ascending, each in [0, P->n)); takes the buffer over as the map.
gulon_index *build_view(const gulon_index *P, DevBuf<int> &&rows, int s) {
  std::unique_ptr<gulon_index> v(new gulon_index());
  v->tune = std::make_shared<ScanTuning>();   // the environment as it is now, as for gulon_index_create
  v->n = s; v->d = P->d; v->m = P->m; v->k = P->k; v->row_base = 0;
  v->vec = P->vec; v->ng = P->ng; v->m_pad = P->m_pad; v->nsub = P->nsub; v->w = P->w;
  v->wide = P->wide;
  v->cents_absmax = P->cents_absmax;
  copy_dev(v->cents, P->cents, (size_t)P->k * P->d);
  copy_dev(v->from, P->from, (size_t)P->m);
  copy_dev(v->sdim, P->sdim, (size_t)P->m);
  const size_t nblk = (size_t)ceil_div(s, 64);
  if (P->wide) {
    v->wcodes.alloc(std::max<size_t>(nblk * P->m * 64, 64));
    if (s > 0) {
      const long long total = (long long)nblk * P->m * 64;
      hipLaunchKernelGGL(gather_wcodes, dim3((unsigned)ceil_div(total, 256LL)), dim3(256), 0, 0, P->wcodes.p, rows.p, s,
                         P->m, v->wcodes.p, total);
      HIP_CHECK(hipGetLastError());
    }
  } else {
    v->codes.alloc(std::max<size_t>(nblk * P->ng * 64 * P->vec, 16));
    if (s > 0) {
      const long long total = (long long)nblk * P->ng * 64;
      if (P->vec == 16)
        hipLaunchKernelGGL(gather_codes<16>, dim3((unsigned)ceil_div(total, 256LL)), dim3(256), 0, 0,
                           (const uint4 *)P->codes.p, rows.p, s, P->ng, (uint4 *)v->codes.p, total);
      else
        hipLaunchKernelGGL(gather_codes<4>, dim3((unsigned)ceil_div(total, 256LL)), dim3(256), 0, 0,
                           (const uint32_t *)P->codes.p, rows.p, s, P->ng, (uint32_t *)v->codes.p, total);
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipDeviceSynchronize());
      build_filter_copy(v.get());   // ordered over the view's own windows: the parent's dealing means nothing here
    }
  }
  // the map names rows of the root
  v->is_view = true;
  v->view_base = P->is_view ? P->view_base : P->row_base;
  if (P->is_view && s > 0) {
    v->vmap.alloc((size_t)s);
    hipLaunchKernelGGL(compose_map_kernel, dim3(ceil_div(s, 256)), dim3(256), 0, 0, P->vmap.p, rows.p, s, v->vmap.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
  } else {
    HIP_CHECK(hipDeviceSynchronize());
    v->vmap = std::move(rows);
  }
  ensure_row_err(v.get());
  return v.release();
}

void require_view(const gulon_index *v) {
  GULON_REQUIRE(v != nullptr, "index is null");
  GULON_REQUIRE(v->is_view, "the index is not a view");
}

}  // namespace

void launch_map_rows(const gulon_index *view, int *d_idx, long long count, hipStream_t st) {
  if (count <= 0 || view->n <= 0) return;
  hipLaunchKernelGGL(map_rows_kernel, dim3((unsigned)ceil_div(count, 256LL)), dim3(256), 0, st, view->vmap.p, view->n,
                     view->view_base, d_idx, count);
  HIP_CHECK(hipGetLastError());
}

}  // namespace gulon

using namespace gulon;

GULON_API int32_t gulon_index_select_rows(gulon_index *idx, const int32_t *rows, int32_t s, gulon_index **out) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr && out != nullptr, "null argument");
    *out = nullptr;
    GULON_REQUIRE(s >= 0 && (rows != nullptr || s == 0), "bad row list");
    for (int p = 0; p < s; p++) {
      GULON_REQUIRE(rows[p] >= 0 && rows[p] < idx->n, "rows[%d] = %d outside [0, %d)", p, rows[p], idx->n);
      GULON_REQUIRE(p == 0 || rows[p] > rows[p - 1], "rows[%d] = %d does not ascend strictly (rows[%d] = %d)", p, rows[p],
                    p - 1, rows[p - 1]);
    }
    DevBuf<int> d_rows;
    if (s > 0) {
      d_rows.upload(rows, (size_t)s);
      HIP_CHECK(hipDeviceSynchronize());
    }
    *out = build_view(idx, std::move(d_rows), s);
  });
}

GULON_API int32_t gulon_index_select_mask_dev(gulon_index *idx, const uint64_t *d_mask, gulon_index **out) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr && out != nullptr, "null argument");
    *out = nullptr;
    GULON_REQUIRE(d_mask != nullptr || idx->n == 0, "mask is null");
    DevBuf<int> d_rows;
    const int s = mask_to_rows((const unsigned long long *)d_mask, idx->n, d_rows);
    *out = build_view(idx, std::move(d_rows), s);
  });
}

GULON_API int32_t gulon_index_select_mask(gulon_index *idx, const uint64_t *mask, gulon_index **out) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr && out != nullptr, "null argument");
    *out = nullptr;
    GULON_REQUIRE(mask != nullptr || idx->n == 0, "mask is null");
    DevBuf<unsigned long long> d_mask;
    if (idx->n > 0) {
      d_mask.upload((const unsigned long long *)mask, (size_t)ceil_div(idx->n, 64));
      HIP_CHECK(hipDeviceSynchronize());
    }
    DevBuf<int> d_rows;
    const int s = mask_to_rows(d_mask.p, idx->n, d_rows);
    *out = build_view(idx, std::move(d_rows), s);
  });
}

GULON_API int32_t gulon_index_view_size(gulon_index *view, int32_t *s) {
  return guarded([&] {
    require_view(view);
    GULON_REQUIRE(s != nullptr, "null argument");
    *s = view->n;
  });
}

GULON_API int32_t gulon_index_view_rows(gulon_index *view, int32_t *rows_out) {
  return guarded([&] {
    require_view(view);
    if (view->n == 0) return;
    GULON_REQUIRE(rows_out != nullptr, "null argument");
    HIP_CHECK(hipMemcpy(rows_out, view->vmap.p, sizeof(int) * (size_t)view->n, hipMemcpyDeviceToHost));
  });
}

GULON_API int32_t gulon_index_view_rows_dev(gulon_index *view, const int32_t **d_rows) {
  return guarded([&] {
    require_view(view);
    GULON_REQUIRE(d_rows != nullptr, "null argument");
    *d_rows = view->vmap.p;
  });
}

GULON_API int32_t gulon_index_view_batch_query_dev(gulon_index *view, const float *d_queries, int32_t b, int32_t k_nn,
                                                   int32_t from, int32_t until, int32_t *d_out_idx, float *d_out_dist,
                                                   int32_t *d_out_count, int32_t *d_out_flags, void *stream) {
  return guarded([&] {
    require_view(view);
    batch_query_dev_on(view, d_queries, b, k_nn, from, until, d_out_idx, d_out_dist, d_out_count, d_out_flags,
                       (hipStream_t)stream, true);
  });
}

GULON_API int32_t gulon_index_view_batch_query(gulon_index *view, const float *queries, int32_t b, int32_t k_nn,
                                               int32_t from, int32_t until, int32_t *out_idx, float *out_dist,
                                               int32_t *out_count, int32_t *out_flags) {
  return guarded([&] {
    require_view(view);
    batch_query_host_on(view, queries, b, k_nn, from, until, out_idx, out_dist, out_count, out_flags, true);
  });
}

GULON_API int32_t gulon_index_view_map_rows_dev(gulon_index *view, int32_t *d_idx, int64_t count, void *stream) {
  return guarded([&] {
    require_view(view);
    GULON_REQUIRE(count >= 0 && (d_idx != nullptr || count == 0), "bad id array");
    launch_map_rows(view, d_idx, count, (hipStream_t)stream);   // reads the map only: no workspace, no ordering needed
  });
}
