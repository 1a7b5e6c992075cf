// Index.exactNearestNeighbours (Index.scala:209-229) with MathUtils.distanceSq
// (MathUtils.scala:85-95): brute-force squared L2, sequential unfused fp32, then the
// same wavefront top-k as the ADC scan.  Used for BASELINE config 1 and for the
// recall ground truth (Tests.scala:89-97).
#include "exact.hpp"   // the distance tile and the declaration of the driver

namespace gulon {

// exact.hpp has the layout of Qt
__global__ void transpose_queries(const float *__restrict__ Q, int B, int d, int ntiles, float *__restrict__ Qt) {
  long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long total = (long long)ntiles * d * KNN_QT;
  if (t >= total) return;
  int u = (int)(t % KNN_QT);
  int dim = (int)((t / KNN_QT) % d);
  int tile = (int)(t / ((long long)KNN_QT * d));
  int q = tile * KNN_QT + u;
  Qt[t] = q < B ? Q[(size_t)q * d + dim] : 0.f;
}

__global__ __launch_bounds__(KNN_THREADS) void knn_kernel(const float *__restrict__ X, int n, int d,
                                                          const float *__restrict__ Qt, int row_from, int row_until,
                                                          int rows_per_chunk, int nchunks, int keff,
                                                          float *__restrict__ part_v, int *__restrict__ part_i,
                                                          const float *__restrict__ lbv, const int *__restrict__ lbi) {
  constexpr int NW = KNN_THREADS / 64;
  __shared__ float xs[KNN_THREADS * (KNN_DT + 1)];
  __shared__ float sv[KNN_QT * NW * 64];
  __shared__ int si[KNN_QT * NW * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tile = blockIdx.x, chunk = blockIdx.y;
  const float *qt = Qt + (size_t)tile * d * KNN_QT;

  WaveList wl[KNN_QT];
  int cnt[KNN_QT];
#pragma unroll
  for (int q = 0; q < KNN_QT; q++) { wl[q].init(); cnt[q] = 0; }

  // large-K peeling: only entries after (lbq, lbiq) in (distance, row id) order are eligible
  const bool peel = lbv != nullptr;
  float lbq[KNN_QT];
  int lbiq[KNN_QT];
#pragma unroll
  for (int q = 0; q < KNN_QT; q++) {
    lbq[q] = peel ? lbv[tile * KNN_QT + q] : -1.f;
    lbiq[q] = peel ? lbi[tile * KNN_QT + q] : -1;
  }

  const int r0 = (row_from / KNN_THREADS) * KNN_THREADS + chunk * rows_per_chunk;
  const int r1 = min(row_until, r0 + rows_per_chunk);
  for (int base = r0; base < r1; base += KNN_THREADS) {
    float acc[KNN_QT];
    exact_tile(X, n, d, qt, xs, tid, [&](int r) { return base + r; }, acc);
    const int row = base + tid;
    const bool valid = row >= row_from && row < row_until;
    unsigned long long vmask = __ballot(valid);
#pragma unroll
    for (int q = 0; q < KNN_QT; q++)
      wave_offer(wl[q], cnt[q], acc[q], valid, vmask, base + wave * 64, keff, lane, [&](float cv, int cr) {
        return !peel || cv > lbq[q] || (cv == lbq[q] && cr > lbiq[q]);
      });
  }
  __syncthreads();
  merge_wave_lists<KNN_QT, NW>(wl, sv, si, keff, lane, wave, [&](int q, const WaveList &out) {
    if (lane < keff) {
      size_t o = ((size_t)(tile * KNN_QT + q) * nchunks + chunk) * keff + lane;
      part_v[o] = out.v;
      part_i[o] = out.i;
    }
  });
}

// exact.hpp: the single-pass / peeled driver of gulon_exact_knn and of the exact index
void exact_knn_dev(const gulon_dataset *ds, int from, int until, const float *d_q, int b, int K, KnnScratch &s, int *oi,
                   float *od, int *oc, int *of, hipStream_t st) {
  const bool peeled = K > GULON_MAX_K;
  const int keff = peeled ? 64 : K + 1, d = ds->d;
  const int ntiles = ceil_div(b, KNN_QT), Bp = ntiles * KNN_QT;
  const RowChunks ch = knn_row_chunks(from, until, ntiles);
  const int nchunks = ch.nchunks, rows_per_chunk = ch.groups_per_chunk * KNN_THREADS;
  s.qt.ensure((size_t)ntiles * d * KNN_QT);
  s.pv.ensure((size_t)Bp * nchunks * keff);
  s.pi.ensure((size_t)Bp * nchunks * keff);
  const long long tq = (long long)ntiles * d * KNN_QT;
  hipLaunchKernelGGL(transpose_queries, dim3(ceil_div(tq, 256)), dim3(256), 0, st, d_q, b, d, ntiles, s.qt.p);
  if (peeled) {
    const int rounds = ceil_div(K + 1, 64), cap = rounds * 64;
    s.accv.ensure((size_t)b * cap); s.acci.ensure((size_t)b * cap);
    s.tv.ensure((size_t)b * 64); s.ti.ensure((size_t)b * 64);
    s.lbv.ensure(Bp); s.lbi.ensure(Bp);
    HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)s.lbv.p, 0xBF800000 /* -1.0f */, (size_t)Bp, st));
    HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)s.lbi.p, 0xFFFFFFFF, (size_t)Bp, st));
    for (int r = 0; r < rounds; r++) {
      hipLaunchKernelGGL(knn_kernel, dim3(ntiles, nchunks), dim3(KNN_THREADS), 0, st, ds->x.p, ds->n, d, s.qt.p, from,
                         until, rows_per_chunk, nchunks, 64, s.pv.p, s.pi.p, s.lbv.p, s.lbi.p);
      HIP_CHECK(hipGetLastError());
      launch_merge(s.pv.p, s.pi.p, nchunks, 64LL, (long long)nchunks * 64, b, 63,
                   QueryOut::partial_lists(s.tv.p, s.ti.p), st);
      launch_peel_update(s.tv.p, s.ti.p, b, r, cap, s.accv.p, s.acci.p, s.lbv.p, s.lbi.p, st);
    }
    launch_peel_finalize(s.accv.p, s.acci.p, b, cap, K, oi, od, oc, of, st);
  } else {
    hipLaunchKernelGGL(knn_kernel, dim3(ntiles, nchunks), dim3(KNN_THREADS), 0, st, ds->x.p, ds->n, d, s.qt.p, from,
                       until, rows_per_chunk, nchunks, keff, s.pv.p, s.pi.p, (const float *)nullptr,
                       (const int *)nullptr);
    HIP_CHECK(hipGetLastError());
    launch_merge(s.pv.p, s.pi.p, nchunks, (long long)keff, (long long)nchunks * keff, b, K,
                 QueryOut::final_lists(oi, od, oc, of), st);
  }
}

}  // namespace gulon

using namespace gulon;

GULON_API int32_t gulon_exact_knn(const gulon_dataset *ds, int32_t from, int32_t until, const float *queries,
                                  int32_t b, int32_t k_nn, int32_t *out_idx, float *out_dist, int32_t *out_count,
                                  int32_t *out_flags) {
  return guarded([&] {
    GULON_REQUIRE(ds != nullptr, "dataset is null");
    GULON_REQUIRE(from <= until, "invalid range: expected from=%d <= until=%d", from, until);          // Index.scala:213
    GULON_REQUIRE(until <= ds->n, "invalid range: expected until=%d <= vectors.length=%d", until, ds->n);  // :214
    GULON_REQUIRE(from >= 0 && b >= 0 && k_nn >= 0, "bad arguments");
    GULON_UNSUPPORTED(k_nn > GULON_MAX_K_PEELED, "k_nn = %d > %d", k_nn, GULON_MAX_K_PEELED);
    if (b == 0) return;
    const int K = k_nn;
    size_t bk = (size_t)b * K;
    if (K == 0 || from == until) {
      for (size_t i = 0; i < bk; i++) { out_idx[i] = -1; out_dist[i] = INFINITY; }
      for (int q = 0; q < b; q++) { if (out_count) out_count[q] = 0; if (out_flags) out_flags[q] = 0; }
      return;
    }
    KnnScratch scratch;
    DevBuf<float> dq, od(bk);
    DevBuf<int> oi(bk), oc(b), of(b);
    dq.upload(queries, (size_t)b * ds->d);
    exact_knn_dev(ds, from, until, dq.p, b, K, scratch, oi.p, od.p, oc.p, of.p, nullptr);
    oi.download(out_idx, bk); od.download(out_dist, bk);
    if (out_count) oc.download(out_count, b);
    if (out_flags) of.download(out_flags, b);
    HIP_CHECK(hipDeviceSynchronize());
  });
}
