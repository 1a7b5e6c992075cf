// Index updates: new root indexes built on the device from an index's own quantizer and from the code buffers of
// existing indexes, and the accessor that reads codes back.
//
// The reference has no mutation.  An updated index is the PQIndex the reference would hold over the merged
// EncodedMatrix: new columns are ProductQuantizer.encode of the new vectors by the index's own quantizer
// (gulon_index_encode_dataset), and the columns of two indexes are combined in any order (gulon_index_merge).  Both give
// ordinary root indexes -- no map, row_base 0 -- that own all they read.
//
// Kernels
//   store_codes<VEC>      [m][n] int assignments -> [n/64][ng][64][VEC], zero words in the ragged last block
//   store_wcodes          the same for the wide layout [n/64][m][64] of uint16
//   merge_codes<VEC>      gather_codes (subset.hip) from two sources: take[p] >= 0 row take[p] of a, else row -1 - take[p] of b
//   merge_wcodes          the same for the wide layout
//   unblock_codes         rows [from, until) of [n/64][ng][64][VEC] -> [m][until - from] uint16 (EncodedMatrix.indices)
//   unblock_wcodes        the same for the wide layout
#include "kmeans.hpp"
#include "scan.hpp"

namespace gulon {
namespace {

template <int VEC> struct CodePack;
template <> struct CodePack<4> {
  static __device__ __forceinline__ uint32_t make(const uint32_t *x) { return x[0]; }
};
template <> struct CodePack<16> {
  static __device__ __forceinline__ uint4 make(const uint32_t *x) { return make_uint4(x[0], x[1], x[2], x[3]); }
};

template <int VEC>
__global__ void store_codes(const int *__restrict__ assign /*[m][n]*/, int n, int m, int ng,
                            typename CodeWord<VEC>::type *__restrict__ dst, long long total /* nblk*ng*64 */) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int lane = (int)(t & 63);
  const long long bg = t >> 6;
  const int g = (int)(bg % ng);
  const long long row = (bg / ng) * 64 + lane;
  uint32_t x[VEC / 4];
#pragma unroll
  for (int q = 0; q < VEC / 4; q++) {
    uint32_t v = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) {
      const int j = g * VEC + q * 4 + b;
      const uint32_t c = (row < n && j < m) ? (uint32_t)assign[(size_t)j * n + row] & 0xFFu : 0u;   // Coder8: idx.toByte
      v |= c << (8 * b);
    }
    x[q] = v;
  }
  dst[t] = CodePack<VEC>::make(x);
}

__global__ void store_wcodes(const int *__restrict__ assign /*[m][n]*/, int n, int m, uint16_t *__restrict__ dst,
                             long long total /* nblk*m*64 */) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int lane = (int)(t & 63);
  const long long bj = t >> 6;
  const int j = (int)(bj % m);
  const long long row = (bj / m) * 64 + lane;
  dst[t] = row < n ? (uint16_t)assign[(size_t)j * n + row] : (uint16_t)0;
}

// lanes past the last row get what relayout_codes gives padding rows: zero words
template <int VEC>
__global__ void merge_codes(const typename CodeWord<VEC>::type *__restrict__ a,
                            const typename CodeWord<VEC>::type *__restrict__ b, const int *__restrict__ take, int s,
                            int ng, typename CodeWord<VEC>::type *__restrict__ dst, long long total /* nblk*ng*64 */) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int lane = (int)(t & 63);
  const long long bg = t >> 6;
  const int g = (int)(bg % ng);
  const long long p = (bg / ng) * 64 + lane;
  typename CodeWord<VEC>::type w{};
  if (p < s) {
    const int e = take[p];
    const int r = e >= 0 ? e : -1 - e;
    const typename CodeWord<VEC>::type *src = e >= 0 ? a : b;
    w = src[((size_t)(r >> 6) * ng + g) * 64 + (r & 63)];
  }
  dst[t] = w;
}

__global__ void merge_wcodes(const uint16_t *__restrict__ a, const uint16_t *__restrict__ b,
                             const int *__restrict__ take, int s, int m, uint16_t *__restrict__ dst,
                             long long total /* nblk*m*64 */) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int lane = (int)(t & 63);
  const long long bj = t >> 6;
  const int j = (int)(bj % m);
  const long long p = (bj / m) * 64 + lane;
  uint16_t v = 0;
  if (p < s) {
    const int e = take[p];
    const int r = e >= 0 ? e : -1 - e;
    const uint16_t *src = e >= 0 ? a : b;
    v = src[((size_t)(r >> 6) * m + j) * 64 + (r & 63)];
  }
  dst[t] = v;
}

__global__ void unblock_codes(const uint8_t *__restrict__ src, int vec, int ng, int from, int count,
                              uint16_t *__restrict__ out /*[m][count]*/, long long total /* m*count */) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int j = (int)(t / count);
  const int r = from + (int)(t - (long long)j * count);
  out[t] = src[(((size_t)(r >> 6) * ng + j / vec) * 64 + (r & 63)) * vec + j % vec];
}

__global__ void unblock_wcodes(const uint16_t *__restrict__ src, int m, int from, int count,
                               uint16_t *__restrict__ out /*[m][count]*/, long long total /* m*count */) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int j = (int)(t / count);
  const int r = from + (int)(t - (long long)j * count);
  out[t] = src[((size_t)(r >> 6) * m + j) * 64 + (r & 63)];
}

template <class T>
void copy_dev(DevBuf<T> &dst, const DevBuf<T> &src, size_t count) {
  dst.alloc(count);
  if (count) HIP_CHECK(hipMemcpy(dst.p, src.p, count * sizeof(T), hipMemcpyDeviceToDevice));
}

unsigned grid_of(long long total) { return (unsigned)ceil_div(total, 256LL); }

// A root index of `n` rows with P's shape and its own copy of P's quantizer; the code buffer allocated, not written.
std::unique_ptr<gulon_index> new_root_like(const gulon_index *P, int n) {
  std::unique_ptr<gulon_index> r(new gulon_index());
  r->tune = std::make_shared<ScanTuning>();   // the environment as it is now, as for gulon_index_create
  r->n = n; r->d = P->d; r->m = P->m; r->k = P->k; r->row_base = 0;
  r->vec = P->vec; r->ng = P->ng; r->m_pad = P->m_pad; r->nsub = P->nsub; r->w = P->w;
  r->wide = P->wide;
  r->cents_absmax = P->cents_absmax;
  copy_dev(r->cents, P->cents, (size_t)P->k * P->d);
  copy_dev(r->from, P->from, (size_t)P->m);
  copy_dev(r->sdim, P->sdim, (size_t)P->m);
  const size_t nblk = (size_t)ceil_div(n, 64);
  if (P->wide) r->wcodes.alloc(std::max<size_t>(nblk * P->m * 64, 64));
  else r->codes.alloc(std::max<size_t>(nblk * P->ng * 64 * P->vec, 16));
  return r;
}

// after the code buffer is written: the filter's copy, where the shape calls for one
void finish_root(gulon_index *r) {
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  if (!r->wide && r->n > 0) build_filter_copy(r);
}

bool same_codebooks(const gulon_index *a, const gulon_index *b) {
  if (a->cents.p == b->cents.p) return true;   // contexts of one index
  const size_t count = (size_t)a->k * a->d;
  std::vector<float> ha(count), hb(count);
  HIP_CHECK(hipMemcpy(ha.data(), a->cents.p, count * sizeof(float), hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(hb.data(), b->cents.p, count * sizeof(float), hipMemcpyDeviceToHost));
  return memcmp(ha.data(), hb.data(), count * sizeof(float)) == 0;
}

}  // namespace
}  // namespace gulon

using namespace gulon;

GULON_API int32_t gulon_index_encode_dataset(gulon_index *idx, const gulon_dataset *ds, gulon_index **out) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr && ds != nullptr && out != nullptr, "null argument");
    *out = nullptr;
    GULON_REQUIRE(ds->d == idx->d, "the vectors have %d dimensions, the index %d", ds->d, idx->d);
    const int n = ds->n, m = idx->m, k = idx->k;
    std::unique_ptr<gulon_index> r = new_root_like(idx, n);
    if (n > 0) {
      const size_t nblk = (size_t)ceil_div(n, 64);
      if (k == 1) {                              // Coder0: every index is 0
        HIP_CHECK(hipMemset(r->codes.p, 0, nblk * r->ng * 64 * r->vec));
      } else {
        std::vector<int> from, until;
        subvectors(idx->d, m, from, until);
        KmeansWorkspace ws;
        PackedSlice packed;
        DevBuf<float> dc;
        DevBuf<int> da((size_t)m * n);           // [m][n]: one quantizer's assignments per pass
        for (int j = 0; j < m; j++) {
          const int s = until[j] - from[j];
          dc.alloc((size_t)k * s);               // the quantizer's block of the index's codebooks, aligned as an upload is
          HIP_CHECK(hipMemcpy(dc.p, idx->cents.p + (size_t)k * from[j], sizeof(float) * (size_t)k * s,
                              hipMemcpyDeviceToDevice));
          pq_assign_quantizer(ws, packed, ds->x.p, n, ds->d, from[j], s, dc.p, k, da.p + (size_t)j * n);
        }
        if (r->wide) {
          const long long total = (long long)nblk * m * 64;
          hipLaunchKernelGGL(store_wcodes, dim3(grid_of(total)), dim3(256), 0, 0, da.p, n, m, r->wcodes.p, total);
        } else {
          const long long total = (long long)nblk * r->ng * 64;
          if (r->vec == 16)
            hipLaunchKernelGGL(store_codes<16>, dim3(grid_of(total)), dim3(256), 0, 0, da.p, n, m, r->ng,
                               (uint4 *)r->codes.p, total);
          else
            hipLaunchKernelGGL(store_codes<4>, dim3(grid_of(total)), dim3(256), 0, 0, da.p, n, m, r->ng,
                               (uint32_t *)r->codes.p, total);
        }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());       // the assignments go out of scope
      }
    }
    finish_root(r.get());
    ensure_row_err(r.get());
    *out = r.release();
  });
}

GULON_API int32_t gulon_index_merge(gulon_index *a, gulon_index *b, const int32_t *take, int32_t s, gulon_index **out) {
  return guarded([&] {
    GULON_REQUIRE(a != nullptr && out != nullptr, "null argument");
    *out = nullptr;
    GULON_REQUIRE(s >= 0 && (take != nullptr || s == 0), "bad take list");
    if (b != nullptr) {
      GULON_REQUIRE(a->d == b->d && a->m == b->m && a->k == b->k,
                    "the indexes differ in shape: d=%d m=%d k=%d and d=%d m=%d k=%d", a->d, a->m, a->k, b->d, b->m, b->k);
    }
    for (int p = 0; p < s; p++) {
      const int e = take[p];
      if (e >= 0) {
        GULON_REQUIRE(e < a->n, "take[%d] = %d outside [0, %d) of the first index", p, e, a->n);
      } else {
        GULON_REQUIRE(b != nullptr, "take[%d] = %d names a row of the second index, which is null", p, e);
        GULON_REQUIRE(-1 - e < b->n, "take[%d] = %d (row %d) outside [0, %d) of the second index", p, e, -1 - e, b->n);
      }
    }
    if (b != nullptr) GULON_REQUIRE(same_codebooks(a, b), "the indexes differ in their codebooks");
    std::unique_ptr<gulon_index> r = new_root_like(a, s);
    if (s > 0) {
      DevBuf<int> d_take;
      d_take.upload(take, (size_t)s);
      const size_t nblk = (size_t)ceil_div(s, 64);
      const gulon_index *bb = b != nullptr ? b : a;   // never read when b is null: every entry is >= 0
      if (r->wide) {
        const long long total = (long long)nblk * r->m * 64;
        hipLaunchKernelGGL(merge_wcodes, dim3(grid_of(total)), dim3(256), 0, 0, a->wcodes.p, bb->wcodes.p, d_take.p, s,
                           r->m, r->wcodes.p, total);
      } else {
        const long long total = (long long)nblk * r->ng * 64;
        if (r->vec == 16)
          hipLaunchKernelGGL(merge_codes<16>, dim3(grid_of(total)), dim3(256), 0, 0, (const uint4 *)a->codes.p,
                             (const uint4 *)bb->codes.p, d_take.p, s, r->ng, (uint4 *)r->codes.p, total);
        else
          hipLaunchKernelGGL(merge_codes<4>, dim3(grid_of(total)), dim3(256), 0, 0, (const uint32_t *)a->codes.p,
                             (const uint32_t *)bb->codes.p, d_take.p, s, r->ng, (uint32_t *)r->codes.p, total);
      }
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipDeviceSynchronize());         // the take list goes out of scope
    }
    finish_root(r.get());
    ensure_row_err(r.get());
    *out = r.release();
  });
}

GULON_API int32_t gulon_index_get_codes(gulon_index *idx, int32_t from, int32_t until, uint16_t *out) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    GULON_REQUIRE(0 <= from && from <= until && until <= idx->n, "rows [%d, %d) outside [0, %d)", from, until, idx->n);
    const int count = until - from;
    if (count == 0) return;
    GULON_REQUIRE(out != nullptr, "null argument");
    const long long total = (long long)idx->m * count;
    DevBuf<uint16_t> plain((size_t)total);
    if (idx->wide)
      hipLaunchKernelGGL(unblock_wcodes, dim3(grid_of(total)), dim3(256), 0, 0, idx->wcodes.p, idx->m, from, count,
                         plain.p, total);
    else
      hipLaunchKernelGGL(unblock_codes, dim3(grid_of(total)), dim3(256), 0, 0, idx->codes.p, idx->vec, idx->ng, from,
                         count, plain.p, total);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpy(out, plain.p, sizeof(uint16_t) * (size_t)total, hipMemcpyDeviceToHost));
  });
}
