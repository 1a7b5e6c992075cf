// Offset queries on the grouped index.  Per query q and per row r of the groups q searches:
//   d   the distance the grouped handle's ordinary query returns between q and r: the residual q - centroid(group) by
//       MathUtils.subtract, Index.prepareQuery on it, the row's entries summed quantizer 0 first from 0.f, unfused;
//   t   = d + offsets[r], one binary32 addition, offsets indexed by grouped row position;
// a row is a candidate if and only if t is finite and r is not exclude[q]; the answer is the candidates by (t ascending,
// row ascending), the first k_nn.  Rows of groups the query does not search are never candidates.
//
//   grouped_offset_scan   gq_group_scan's geometry (grouped.hip): a workgroup is four (query, searched-group slot) pairs,
//                         one wave each; the pair's residual and [m_pad][256] table in LDS (group_pair_table: each
//                         quantizer's codebook slice staged once for the four pairs, dead slots help); the group's
//                         rows 64 at a time with the code-word prefetch ring, one offset load per row, t into the
//                         pair's WaveList in registers (wave_offer), which orders by (key ascending, row ascending);
//                         the pair's keff entries to its slot's list, padded with (+inf, INT_MAX) -- a dead slot's
//                         list is all padding
//   launch_merge          the `stride` lists of a query -> the first k_nn, -1 / +inf after the last.  A candidate's key
//                         is finite, so it is never confused with the padding.
#include "grouped_offset.hpp"
#include "table_scan.hpp"   // finite_key

namespace gulon {
namespace {

// gq_group_scan's constants (grouped.hip), which the launch's LDS (group_scan_lds) is sized by
constexpr int GO_WAVES = 4;    // (query, group) pairs per workgroup: they share the staged codebook slices
constexpr int GO_RPT = 8;      // centroid components prefetched per thread (sub-vectors up to 8 wide are fully overlapped)
constexpr int GO_PD = 4;       // quantizers whose codebooks are in flight

// The residual and table of a pair: gq_group_scan's build, arithmetic and all, as a local copy (lifting it
// into a function both kernels call left gq_group_scan's register and LDS figures alone but its literal route measured
// 0.7 % slower, so that kernel stays as it is and the duplication is follow-up).  Every thread of the workgroup calls (it
// holds barriers); `live` is wave-uniform and says whether this wave has a pair: query row `qrow` [d] against group
// centroid `gc` [d].  On return gtab holds the pair's table, entries beyond k and padding quantizers 0, and every wave is
// done with the slice.
__device__ __forceinline__ void group_pair_table(bool live, const float *__restrict__ qrow, const float *__restrict__ gc,
                                                 int m, int m_pad, int k, int d, const float *__restrict__ pq_cents,
                                                 const int *__restrict__ from, const int *__restrict__ sdim, float *gtab,
                                                 float *res, float *slice, int tid, int lane) {
  __syncthreads();
  if (live)
    for (int e = lane; e < d; e += 64) res[e] = qrow[e] - gc[e];   // MathUtils.subtract
  // Index.prepareQuery on the residual: T[j][c'] = sum_e (r[from_j+e] - cent_j[c'][e])^2, e ascending, unfused.
  // The codebook of quantizer j (k * s_j contiguous floats) is staged once for the four pairs.
  // The codebooks of the next GO_PD quantizers are in flight in registers (GO_RPT floats per thread
  // each) while this one is used: at two workgroups per CU a single global round trip costs more
  // than a quantizer's 256 x s table entries (LDS holds one slice at a time).
  static_assert(64 * GO_WAVES == 256, "thread = centroid staging assumes 256 threads");
  float pre[GO_PD][GO_RPT];
  // thread = centroid (k <= 256 threads): component x of its centroid, no index arithmetic
  auto fetch = [&](int j, float (&dst)[GO_RPT]) {
    const int fr = j < m ? from[j] : 0, sj = j < m ? sdim[j] : 0;
    const float *cent = pq_cents + (size_t)k * fr + (size_t)tid * sj;
#pragma unroll
    for (int u = 0; u < GO_RPT; u++) dst[u] = (tid < k && u < sj) ? cent[u] : 0.f;
  };
#pragma unroll
  for (int p = 0; p < GO_PD; p++) fetch(p, pre[p]);
  for (int j0 = 0; j0 < m_pad; j0 += GO_PD) {            // m_pad is a multiple of 4
#pragma unroll
    for (int p = 0; p < GO_PD; p++) {
      const int j = j0 + p;
      const int fr = j < m ? from[j] : 0, sj = j < m ? sdim[j] : 0;
      float *sl = slice;
      __syncthreads();                                   // slice j-1 is no longer read
      // stored transposed, [x][centroid]: the lanes of a wave then read consecutive addresses
#pragma unroll
      for (int u = 0; u < GO_RPT; u++)
        if (u < sj) sl[u * 256 + tid] = pre[p][u];
      for (int x = GO_RPT; x < sj; x++)                  // long sub-vectors: the rest straight from memory
        sl[x * 256 + tid] = tid < k ? pq_cents[(size_t)k * fr + (size_t)tid * sj + x] : 0.f;
      if (j + GO_PD < m_pad) fetch(j + GO_PD, pre[p]);
      __syncthreads();                                   // slice j complete
      if (live) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};             // centroids lane, lane + 64, lane + 128, lane + 192
        for (int x = 0; x < sj; x++) {
          const float rx = res[fr + x];
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const float dd = rx - sl[x * 256 + lane + 64 * i];
            acc[i] += dd * dd;
          }
        }
#pragma unroll
        for (int i = 0; i < 4; i++) gtab[j * 256 + lane + 64 * i] = lane + 64 * i < k ? acc[i] : 0.f;
      }
    }
  }
  __syncthreads();
}

template <int VEC>
__global__ __launch_bounds__(64 * GO_WAVES) void grouped_offset_scan(
    const uint8_t *__restrict__ codes, int ng, int m, int m_pad, int k, int d, const float *__restrict__ pq_cents,
    const int *__restrict__ from, const int *__restrict__ sdim, const float *__restrict__ gcent,
    const int *__restrict__ bounds, const float *__restrict__ Q, const int *__restrict__ nn, int nn_stride,
    const int *__restrict__ nn_cnt, int stride, const float *__restrict__ offsets, const int *__restrict__ exclude,
    int keff, float *__restrict__ part_v, int *__restrict__ part_i) {
  using Word = typename CodeWord<VEC>::type;
  // per wave: m_pad * 256 table entries + d residual components; then one codebook slice
  extern __shared__ float go_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int t = blockIdx.x * GO_WAVES + wave;            // searched-group slot of this wave
  const int q = blockIdx.y;
  float *gtab = go_lds + (size_t)wave * (m_pad * 256 + d);
  float *res = gtab + m_pad * 256;
  float *slice = go_lds + (size_t)GO_WAVES * (m_pad * 256 + d);
  const bool live = t < nn_cnt[q];                       // wave-uniform; dead waves still help staging
  const int c = live ? nn[(size_t)q * nn_stride + t] : 0;
  group_pair_table(live, Q + (size_t)q * d, gcent + (size_t)c * d, m, m_pad, k, d, pq_cents, from, sdim, gtab, res, slice,
                   tid, lane);
  WaveList wl;
  wl.init();
  if (live) {
    int cnt = 0;
    const int ex = exclude != nullptr ? exclude[q] : -1;
    const int row_from = bounds[c], row_until = bounds[c + 1];
    const Word *cw = reinterpret_cast<const Word *>(codes);
    // the first code words of the next GO_PD row blocks stay in flight
    const int rb_first = row_from / 64, rb_end = (row_until + 63) / 64;
    Word wq[GO_PD];
#pragma unroll
    for (int p = 0; p < GO_PD; p++) wq[p] = rb_first + p < rb_end ? cw[((size_t)(rb_first + p) * ng) * 64 + lane] : Word{};
    for (int rb0 = rb_first; rb0 < rb_end; rb0 += GO_PD) {
#pragma unroll
      for (int p = 0; p < GO_PD; p++) {
        const int rb = rb0 + p;
        if (rb >= rb_end) break;
        const int row = rb * 64 + lane;
        const bool in = row >= row_from && row < row_until;
        const float off = in ? offsets[row] : 0.f;
        float acc = 0.f;                 // PQIndex.distances: j ascending, unfused fp32
        const Word w0 = wq[p];
        if (rb + GO_PD < rb_end) wq[p] = cw[((size_t)(rb + GO_PD) * ng) * 64 + lane];
        for (int gi = 0; gi < ng; gi++) {
          const Word w = gi == 0 ? w0 : cw[((size_t)rb * ng + gi) * 64 + lane];
          const float *tj = gtab + gi * VEC * 256;
#pragma unroll
          for (int b = 0; b < VEC; b++) acc += tj[b * 256 + code_byte<VEC>(w, b)];
        }
        const float key = __fadd_rn(acc, off);
        const bool valid = in && finite_key(key) && row != ex;
        wave_offer(wl, cnt, key, valid, __ballot(valid), rb * 64, keff, lane);
      }
    }
  }
  if (t < stride && lane < keff) {   // (a dead slot: the padding wl.init() left)
    const size_t o = ((size_t)q * stride + t) * keff + lane;
    part_v[o] = wl.v;
    part_i[o] = wl.i;
  }
}

}  // namespace

void launch_grouped_offset(const GroupedOffsetPass &p, GroupedOffsetWork &x, int k_nn, const float *d_offsets,
                           const int *d_exclude, int *out_idx, float *out_key, int *out_count, hipStream_t st) {
  if (p.nb <= 0) return;
  GULON_REQUIRE(p.d_q != nullptr && d_offsets != nullptr && out_idx != nullptr && out_key != nullptr, "null argument");
  const gulon_index *ix = p.pq;
  const int keff = k_nn + 1;
  x.pv.ensure((size_t)p.nb * p.stride * keff); x.pi.ensure((size_t)p.nb * p.stride * keff);
  auto kern = ix->vec == 16 ? grouped_offset_scan<16> : grouped_offset_scan<4>;
  HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)p.lds_bytes));
  hipLaunchKernelGGL(kern, dim3(ceil_div(p.stride, GO_WAVES), p.nb), dim3(64 * GO_WAVES), p.lds_bytes, st, ix->codes.p,
                     ix->ng, ix->m, ix->m_pad, ix->k, ix->d, ix->cents.p, ix->from.p, ix->sdim.p, p.gcent, p.bounds, p.d_q,
                     p.nn, p.nn_stride, p.nn_cnt, p.stride, d_offsets, d_exclude, keff, x.pv.p, x.pi.p);
  HIP_CHECK(hipGetLastError());
  launch_merge(x.pv.p, x.pi.p, p.stride, (long long)keff, (long long)p.stride * keff, p.nb, k_nn,
               QueryOut::final_lists(out_idx, out_key, out_count, nullptr), st);
}

}  // namespace gulon
