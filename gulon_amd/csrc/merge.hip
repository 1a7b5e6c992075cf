// Merging sorted (distance, row id) lists: merge_lists, the per-query merge of partial lists (chunks, or GPUs) every
// top-k user ends with; the large-K peeling rounds (64 entries per scan round); and the pairwise merge tree of shards'
// lists beyond 63 entries (merge2_long).
#include "scan.hpp"

namespace gulon {

// ---------------------------------------------------------------------------
// merge `lists` sorted partial lists per query; one wave per query.
// in: element (l, q, e) at  l*stride_l + q*stride_q + e.
// FINAL: write idx/dist/count/flags [B][K]; else write a (K+1)-list [B][keff].
// ---------------------------------------------------------------------------
template <bool FINAL>
__global__ __launch_bounds__(64) void merge_lists(const float *__restrict__ in_v, const int *__restrict__ in_i,
                                                  int lists, long long stride_l, long long stride_q,
                                                  int B, int K, int keff, int *__restrict__ out_idx,
                                                  float *__restrict__ out_dist, int *__restrict__ out_count,
                                                  int *__restrict__ out_flags, float *__restrict__ out_pv,
                                                  int *__restrict__ out_pi, const int *__restrict__ tile_enable,
                                                  int qt) {
  const int q = blockIdx.x;
  const int lane = threadIdx.x;
  if (q >= B) return;
  if (tile_enable && tile_enable[q / qt] == 0) return;
  WaveList wl;
  wl.init();
  const int total = lists * keff;
  for (int base = 0; base < total; base += 64) {
    int e = base + lane;
    float cv = INFINITY;
    int cr = INT_MAX;
    if (e < total) {
      int l = e / keff, x = e - l * keff;
      size_t o = (size_t)l * stride_l + (size_t)q * stride_q + x;
      cv = in_v[o];
      cr = in_i[o];
    }
    unsigned long long mk = __ballot(cr != INT_MAX && wl.accepts(cv, cr));
    while (mk) {
      int l = __ffsll((long long)mk) - 1;
      mk &= mk - 1;
      float v = readlane_f(cv, l);
      int r = readlane_i(cr, l);
      if (wl.accepts(v, r)) wl.insert(v, r, keff, lane);
    }
  }
  if (FINAL) {
    int live = __popcll(__ballot(lane < K && wl.i != INT_MAX));
    if (lane < K) {
      bool ok = wl.i != INT_MAX;
      out_idx[(size_t)q * K + lane] = ok ? wl.i : -1;
      out_dist[(size_t)q * K + lane] = ok ? wl.v : INFINITY;
    }
    float nv = __shfl_down(wl.v, 1);
    int ni = __shfl_down(wl.i, 1);
    bool tie = wl.i != INT_MAX && ni != INT_MAX && wl.v == nv && lane + 1 < keff;
    unsigned long long tm = __ballot(tie);
    if (lane == 0) {
      if (out_count) out_count[q] = live;
      if (out_flags) {
        int f = 0;
        if (K >= 1 && ((tm >> (K - 1)) & 1ull)) f |= GULON_FLAG_BOUNDARY_TIE;
        if (K >= 2 && (tm & ((1ull << (K - 1)) - 1ull))) f |= GULON_FLAG_INTERIOR_TIE;
        out_flags[q] = f;
      }
    }
  } else {
    if (lane < keff) {
      out_pv[(size_t)q * keff + lane] = wl.v;
      out_pi[(size_t)q * keff + lane] = wl.i;
    }
  }
}


void launch_merge(const float *in_v, const int *in_i, int lists, long long stride_l, long long stride_q, int B, int K,
                  const QueryOut &out, hipStream_t st) {
  if (B <= 0) return;
  hipLaunchKernelGGL(out.final_out() ? merge_lists<true> : merge_lists<false>, dim3(B), dim3(64), 0, st, in_v, in_i,
                     lists, stride_l, stride_q, B, K, K + 1, out.idx, out.dist, out.count, out.flags, out.part_v,
                     out.part_i, (const int *)nullptr, 1);
  HIP_CHECK(hipGetLastError());
}

void launch_merge_enabled(const float *in_v, const int *in_i, int lists, long long stride_l, long long stride_q, int B,
                          int K, float *out_pv, int *out_pi, const int *tile_enable, int qt, hipStream_t st) {
  if (B <= 0) return;
  hipLaunchKernelGGL(merge_lists<false>, dim3(B), dim3(64), 0, st, in_v, in_i, lists, stride_l, stride_q, B, K, K + 1,
                     (int *)nullptr, (float *)nullptr, (int *)nullptr, (int *)nullptr, out_pv, out_pi, tile_enable, qt);
  HIP_CHECK(hipGetLastError());
}

// ---- large K: peel the result 64 entries at a time (each round = one scan restricted to the
// ---- entries after the previous round's last one) -------------------------------------
__global__ __launch_bounds__(64) void peel_update(const float *__restrict__ tv, const int *__restrict__ ti, int round,
                                                  int cap, float *__restrict__ pv, int *__restrict__ pi,
                                                  float *__restrict__ lbv, int *__restrict__ lbi) {
  const int q = blockIdx.x, lane = threadIdx.x;
  const float v = tv[(size_t)q * 64 + lane];
  const int i = ti[(size_t)q * 64 + lane];
  pv[(size_t)q * cap + round * 64 + lane] = v;
  pi[(size_t)q * cap + round * 64 + lane] = i;
  if (lane == 63) {
    if (i != INT_MAX) { lbv[q] = v; lbi[q] = i; }
    else { lbv[q] = INFINITY; lbi[q] = INT_MAX; }   // list exhausted: nothing is eligible any more
  }
}

__global__ void peel_finalize(const float *__restrict__ pv, const int *__restrict__ pi, int B, int cap, int K,
                              int *__restrict__ out_idx, float *__restrict__ out_dist, int *__restrict__ out_count,
                              int *__restrict__ out_flags) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= B) return;
  const float *v = pv + (size_t)q * cap;
  const int *id = pi + (size_t)q * cap;
  int live = 0, flags = 0;
  for (int e = 0; e < K; e++) {
    const bool ok = id[e] != INT_MAX;
    out_idx[(size_t)q * K + e] = ok ? id[e] : -1;
    out_dist[(size_t)q * K + e] = ok ? v[e] : INFINITY;
    live += ok ? 1 : 0;
    if (ok && e + 1 < cap && id[e + 1] != INT_MAX && v[e] == v[e + 1])
      flags |= (e == K - 1) ? GULON_FLAG_BOUNDARY_TIE : GULON_FLAG_INTERIOR_TIE;
  }
  if (out_count) out_count[q] = live;
  if (out_flags) out_flags[q] = flags;
}

// the peeled list as a partial (K+1)-list for the multi-GPU merge: [B][cap] -> [B][K+1]
__global__ void peel_export(const float *__restrict__ pv, const int *__restrict__ pi, int B, int cap, int keff,
                            float *__restrict__ out_v, int *__restrict__ out_i) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)B * keff) return;
  const int q = (int)(t / keff), e = (int)(t - (long long)q * keff);
  out_v[t] = pv[(size_t)q * cap + e];
  out_i[t] = pi[(size_t)q * cap + e];
}

// Merge of two ascending (distance, row id) lists of `len` entries per query (padded with (+inf, INT_MAX)) into
// the `len` smallest, ascending: every entry's position = its own index + its rank in the other list (row ids
// are distinct across lists, so the order is strict).  b == nullptr: a copies through.
__global__ __launch_bounds__(256) void merge2_long(const float *__restrict__ av, const int *__restrict__ ai,
                                                   const float *__restrict__ bv, const int *__restrict__ bi, int len,
                                                   float *__restrict__ ov, int *__restrict__ oi) {
  const int q = blockIdx.x;
  const float *A = av + (size_t)q * len, *Bv = bv ? bv + (size_t)q * len : nullptr;
  const int *Ai = ai + (size_t)q * len, *Bi = bi ? bi + (size_t)q * len : nullptr;
  float *O = ov + (size_t)q * len;
  int *Oi = oi + (size_t)q * len;
  auto less = [](float v0, int i0, float v1, int i1) { return v0 < v1 || (v0 == v1 && i0 < i1); };
  for (int e = threadIdx.x; e < len; e += blockDim.x) {
    if (!Bv) { O[e] = A[e]; Oi[e] = Ai[e]; continue; }
    {   // A[e]: entries of B before it
      const float v = A[e]; const int id = Ai[e];
      int lo = 0, hi = len;
      while (lo < hi) { const int mid = (lo + hi) >> 1; if (less(Bv[mid], Bi[mid], v, id)) lo = mid + 1; else hi = mid; }
      const int pos = e + lo;
      if (pos < len && id != INT_MAX) { O[pos] = v; Oi[pos] = id; }
    }
    {   // B[e]: entries of A before it
      const float v = Bv[e]; const int id = Bi[e];
      int lo = 0, hi = len;
      while (lo < hi) { const int mid = (lo + hi) >> 1; if (less(A[mid], Ai[mid], v, id)) lo = mid + 1; else hi = mid; }
      const int pos = e + lo;
      if (pos < len && id != INT_MAX) { O[pos] = v; Oi[pos] = id; }
    }
  }
}
__global__ void fill_list(float *__restrict__ v, int *__restrict__ i, long long n) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) { v[t] = INFINITY; i[t] = INT_MAX; }
}

void launch_fill_list(float *v, int *i, long long n, hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(fill_list, dim3((unsigned)ceil_div(n, 256LL)), dim3(256), 0, st, v, i, n);
  HIP_CHECK(hipGetLastError());
}

// `lists` partial (K+1)-lists per query (element (l, q, e) at l*stride_l + q*keff + e) -> final [B][K] + count + flags,
// for K beyond the 63 a wavefront list holds: a tree of pairwise merges through device scratch
void launch_merge_long(const float *in_v, const int *in_i, int lists, long long stride_l, int B, int K, int *out_idx,
                       float *out_dist, int *out_count, int *out_flags, hipStream_t st) {
  const int keff = K + 1;
  const size_t per = (size_t)B * keff;
  int width = lists;                       // lists alive in the current round
  DevBuf<float> va, vb;
  DevBuf<int> ia, ib;
  const size_t half = (size_t)((lists + 1) / 2);
  va.alloc(std::max<size_t>(half * per, 1)); ia.alloc(std::max<size_t>(half * per, 1));
  vb.alloc(std::max<size_t>(((half + 1) / 2) * per, 1)); ib.alloc(std::max<size_t>(((half + 1) / 2) * per, 1));
  const float *cv = in_v;
  const int *ci = in_i;
  long long cs = stride_l;
  bool to_a = true;
  while (width > 1) {   // (a single list: straight to the finaliser)
    const int next = (width + 1) / 2;
    float *ov = to_a ? va.p : vb.p;
    int *oi = to_a ? ia.p : ib.p;
    launch_fill_list(ov, oi, (long long)next * per, st);
    for (int p = 0; p < next; p++) {
      const bool pair = 2 * p + 1 < width;
      hipLaunchKernelGGL(merge2_long, dim3(B), dim3(256), 0, st, cv + (size_t)(2 * p) * cs, ci + (size_t)(2 * p) * cs,
                         pair ? cv + (size_t)(2 * p + 1) * cs : nullptr, pair ? ci + (size_t)(2 * p + 1) * cs : nullptr, keff,
                         ov + (size_t)p * per, oi + (size_t)p * per);
    }
    HIP_CHECK(hipGetLastError());
    cv = ov; ci = oi; cs = (long long)per;
    width = next;
    to_a = !to_a;
  }
  launch_peel_finalize(cv, ci, B, keff, K, out_idx, out_dist, out_count, out_flags, st);
  HIP_CHECK(hipStreamSynchronize(st));   // the scratch lists above go out of scope
}

void launch_peel_update(const float *tv, const int *ti, int B, int round, int cap, float *pv, int *pi, float *lbv,
                        int *lbi, hipStream_t st) {
  hipLaunchKernelGGL(peel_update, dim3(B), dim3(64), 0, st, tv, ti, round, cap, pv, pi, lbv, lbi);
  HIP_CHECK(hipGetLastError());
}
void launch_peel_finalize(const float *pv, const int *pi, int B, int cap, int K, int *out_idx, float *out_dist,
                          int *out_count, int *out_flags, hipStream_t st) {
  hipLaunchKernelGGL(peel_finalize, dim3(ceil_div(B, 64)), dim3(64), 0, st, pv, pi, B, cap, K, out_idx, out_dist,
                     out_count, out_flags);
  HIP_CHECK(hipGetLastError());
}

PeelRounds::PeelRounds(gulon_index *ix_, int B_, int bound_slots, int tv_slots, int K_, hipStream_t st_)
    : ix(ix_), B(B_), K(K_), rounds(ceil_div(K_ + 1, 64)), cap(rounds * 64), st(st_) {
  ix->peel_v.ensure((size_t)B * cap); ix->peel_i.ensure((size_t)B * cap);
  ix->peel_tv.ensure((size_t)tv_slots * 64); ix->peel_ti.ensure((size_t)tv_slots * 64);
  ix->peel_lbv.ensure((size_t)bound_slots); ix->peel_lbi.ensure((size_t)bound_slots);
  HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)ix->peel_lbv.p, 0xBF800000 /* -1.0f */, (size_t)bound_slots, st));
  HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)ix->peel_lbi.p, 0xFFFFFFFF /* -1 */, (size_t)bound_slots, st));
}

PeelRounds::Bounds PeelRounds::bounds(int q0) const { return {ix->peel_lbv.p + q0, ix->peel_lbi.p + q0}; }

void PeelRounds::append(int r, int q0, int nq, int lists) {
  launch_merge(ix->part_v.p, ix->part_i.p, lists, 64LL, (long long)lists * 64, nq, 63,
               QueryOut::partial_lists(ix->peel_tv.p, ix->peel_ti.p), st);
  launch_peel_update(ix->peel_tv.p, ix->peel_ti.p, nq, r, cap, ix->peel_v.p + (size_t)q0 * cap,
                     ix->peel_i.p + (size_t)q0 * cap, ix->peel_lbv.p + q0, ix->peel_lbi.p + q0, st);
}

void PeelRounds::finish(const QueryOut &out) {
  if (out.final_out()) {
    launch_peel_finalize(ix->peel_v.p, ix->peel_i.p, B, cap, K, out.idx, out.dist, out.count, out.flags, st);
    return;
  }
  // a shard of a large-K query: its K+1 smallest as a partial list (merged by gulon_topk_merge_dev)
  hipLaunchKernelGGL(peel_export, dim3((unsigned)ceil_div((long long)B * (K + 1), 256LL)), dim3(256), 0, st,
                     ix->peel_v.p, ix->peel_i.p, B, cap, K + 1, out.part_v, out.part_i);
  HIP_CHECK(hipGetLastError());
}

}  // namespace gulon

using namespace gulon;

GULON_API int32_t gulon_topk_merge_dev(const float *d_part_dist, const int32_t *d_part_idx, int32_t lists,
                                       int64_t list_stride, int32_t b, int32_t k_nn, int32_t *d_out_idx,
                                       float *d_out_dist, int32_t *d_out_count, int32_t *d_out_flags, void *stream) {
  return guarded([&] {
    GULON_REQUIRE(lists >= 1 && b >= 0 && k_nn >= 1, "bad merge shape");
    GULON_UNSUPPORTED(k_nn + 1 > GULON_MAX_K_PEELED, "k_nn = %d > %d", k_nn, GULON_MAX_K_PEELED - 1);
    int keff = k_nn + 1;
    GULON_REQUIRE(list_stride == 0 || list_stride >= (long long)b * keff, "list_stride too small");
    if (b == 0) return;
    if (k_nn > GULON_MAX_K) {   // beyond a wavefront list: pairwise merges through scratch (synchronises the stream)
      launch_merge_long(d_part_dist, d_part_idx, lists, list_stride ? (long long)list_stride : (long long)b * keff, b, k_nn,
                        d_out_idx, d_out_dist, d_out_count, d_out_flags, (hipStream_t)stream);
      return;
    }
    launch_merge(d_part_dist, d_part_idx, lists, list_stride ? (long long)list_stride : (long long)b * keff,
                 (long long)keff, b, k_nn, QueryOut::final_lists(d_out_idx, d_out_dist, d_out_count, d_out_flags),
                 (hipStream_t)stream);
  });
}

GULON_API int32_t gulon_topk_merge(const float *part_dist, const int32_t *part_idx, int32_t lists, int32_t b,
                                   int32_t k_nn, int32_t *out_idx, float *out_dist, int32_t *out_count,
                                   int32_t *out_flags) {
  return guarded([&] {
    GULON_REQUIRE(lists >= 1 && b >= 0 && k_nn >= 1, "bad merge shape");
    GULON_UNSUPPORTED(k_nn > GULON_MAX_K, "k_nn = %d > GULON_MAX_K = %d", k_nn, GULON_MAX_K);
    if (b == 0) return;
    size_t np = (size_t)lists * b * (k_nn + 1), bk = (size_t)b * k_nn;
    DevBuf<float> pv; DevBuf<int> pi; DevBuf<int> oi(bk), oc(b), of(b); DevBuf<float> od(bk);
    pv.upload(part_dist, np); pi.upload(part_idx, np);
    int keff = k_nn + 1;
    launch_merge(pv.p, pi.p, lists, (long long)b * keff, (long long)keff, b, k_nn,
                 QueryOut::final_lists(oi.p, od.p, oc.p, of.p), nullptr);
    oi.download(out_idx, bk); od.download(out_dist, bk);
    if (out_count) oc.download(out_count, b);
    if (out_flags) of.download(out_flags, b);
    HIP_CHECK(hipDeviceSynchronize());
  });
}
