// The exact index: Index.exactNearestNeighbours (Index.scala:209-229) with MathUtils.distanceSq (MathUtils.scala:85-95)
// behind a handle, device-resident, and for k_nn > GULON_MAX_K in ONE pass over the rows instead of the peeled path's
// ceil((k_nn + 1) / 64).
//
//   sample   exact_pass<true>   exact distances of S rows spread evenly over [from, until) -> [B][S]
//   bound    exact_tau          tau_q = the (k_nn + 1)-th smallest of them: the distance of a real row, so an upper bound
//                               of the true (k_nn + 1)-th distance
//   main     exact_pass<false>  one read of [from, until), distances by exact_tile; every row with distance <= tau_q is
//                               appended to the query's queue as (distance bits << 32) | row
//   select   exact_select       per query: radix-select the (k_nn + 1)-th key, keep the keys up to it, sort, write
//
// The answer of a query whose distances are all finite is the (distance, row id) order of gulon_exact_knn, whatever the
// order of its queue.  A query whose queue overflowed is answered by the peeled path (knn.hip's exact_knn_dev) in a
// compacted sub-batch; a query that met a NaN / +inf distance by the same path in
// a batch of one, which is what gulon_exact_knn gives it when asked alone.
//
// Expression queries: dataset_compose.hip composes the term rows of the dataset, the handle answers the
// composed vectors at k_nn + extra by the path above, compose.hip's drop_rows_kernel removes the term rows.
//
// Multiplicative analogy queries: gulon_exact_index_query_cosmul[_dev] hand the handle's range and its
// CosmulWork to cosmul.hip, under the handle's mutex and stream order.
//
// Offset queries: gulon_exact_index_query_offset[_dev] hand the range and the handle's OffsetWork to
// offset.hip in the same way.
#include "compose.hpp"
#include "cosmul.hpp"
#include "exact.hpp"
#include "logsumexp.hpp"
#include "offset.hpp"
#include "rank.hpp"
#include "select.hpp"

#include <cstdlib>

namespace gulon {
namespace {

constexpr int SEL_THREADS = 1024;                     // exact_select's workgroup
constexpr size_t EXACT_SCRATCH_BYTES = size_t(1) << 30;   // sample distances + queues of one sub-batch of queries
constexpr int EXACT_SAMPLE_MAX = 1 << 22;             // most sample rows chosen automatically

// Slot j of a pass is row `from + j` (main) or the j-th of S rows spread evenly over the range (sample).
template <bool SAMPLE>
__device__ __forceinline__ int slot_row(int from, int range, int S, int j) {
  return SAMPLE ? from + (int)((long long)j * range / S) : from + j;
}

// Distances of 16 queries to 256 slots per step (exact_tile), written out (sample) or queued when at or below tau.
template <bool SAMPLE>
__global__ __launch_bounds__(KNN_THREADS) void exact_pass(const float *__restrict__ X, int d, const float *__restrict__ Qt,
                                                          int B, int from, int range, int S, int slots_per_chunk,
                                                          float *__restrict__ sample_out,
                                                          const float *__restrict__ tau, unsigned long long *__restrict__ queue,
                                                          int cap, unsigned *__restrict__ cnt, int *__restrict__ overflow,
                                                          int *__restrict__ nonfinite) {
  __shared__ float xs[KNN_THREADS * (KNN_DT + 1)];
  __shared__ int rowid[KNN_THREADS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int tile = blockIdx.x, chunk = blockIdx.y;
  const float *qt = Qt + (size_t)tile * d * KNN_QT;
  const int total = SAMPLE ? S : range;
  const int s0 = chunk * slots_per_chunk;
  const int s1 = min(total, s0 + slots_per_chunk);

  float tq[KNN_QT];
  if (!SAMPLE) {
#pragma unroll
    for (int q = 0; q < KNN_QT; q++) tq[q] = tau[tile * KNN_QT + q];
  }

  for (int base = s0; base < s1; base += KNN_THREADS) {
    float acc[KNN_QT];
    __syncthreads();   // the previous step's readers of rowid are done
    rowid[tid] = base + tid < s1 ? slot_row<SAMPLE>(from, range, S, base + tid) : -1;
    exact_tile(X, from + range, d, qt, xs, tid, [&](int r) { return rowid[r]; }, acc);
    const int slot = base + tid;
    const bool valid = slot < s1;
    if (SAMPLE) {
#pragma unroll
      for (int q = 0; q < KNN_QT; q++) {
        const int qg = tile * KNN_QT + q;
        if (valid && qg < B) sample_out[(size_t)qg * S + slot] = acc[q];
      }
    } else {
      const unsigned row = (unsigned)(from + slot);
      const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
      for (int q = 0; q < KNN_QT; q++) {
        const int qg = tile * KNN_QT + q;
        const unsigned long long bad = __ballot(valid && !(acc[q] < INFINITY));   // NaN or +inf
        if (bad && lane == 0) nonfinite[qg] = 1;
        const bool keep = valid && acc[q] <= tq[q];
        const unsigned long long mk = __ballot(keep);
        if (mk) {
          const int first = __ffsll((long long)mk) - 1, add = __popcll(mk);
          unsigned pos = 0;
          if (lane == first) pos = atomicAdd(&cnt[qg], (unsigned)add);
          pos = (unsigned)readlane_i((int)pos, first);
          if (pos + (unsigned)add <= (unsigned)cap) {
            if (keep)
              queue[(size_t)qg * cap + pos + __popcll(mk & below)] =
                  ((unsigned long long)__float_as_uint(acc[q]) << 32) | row;
          } else if (lane == first) {
            overflow[qg] = 1;
          }
        }
      }
    }
  }
}

// tau[q] = the want-th smallest of the query's S sample distances (q < B), -1 for the padding queries of the last tile
// (nothing is at or below it).  NaN distances sort last (ordered_key); a query that has one is flagged by the main pass.
__global__ __launch_bounds__(256) void exact_tau(const float *__restrict__ sample, int S, int want, int B,
                                                 float *__restrict__ tau) {
  __shared__ unsigned hsub[256 * 8], hist[256];
  __shared__ RadixSelectState state;
  const int q = blockIdx.x, tid = threadIdx.x;
  if (q >= B) {   // (uniform per workgroup)
    if (tid == 0) tau[q] = -1.f;
    return;
  }
  const float *s = sample + (size_t)q * S;
  const unsigned key = block_radix_select<256>(
      [&](auto f) __attribute__((always_inline)) {
        for (int e = tid; e < S; e += 256) f(ordered_key(s[e]));
      },
      (unsigned)want, hsub, hist, state);
  if (tid == 0) tau[q] = ordered_float(key);
}

// no sample: every finite distance is queued
__global__ void exact_tau_all(int B, int Bp, float *__restrict__ tau) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q < Bp) tau[q] = q < B ? INFINITY : -1.f;
}

// One workgroup per query over its queue of c keys: the want = min(K + 1, c) smallest, ascending, then rows, distances,
// count and tie flags as launch_peel_finalize writes them.  Keys are distinct (one per row), so the want-th key is
// found by two radix selects -- the distance word, then the row word among the keys that share it -- and exactly
// `want` keys are at or below it.  Dynamic LDS only (a 16-byte aligned base): keys [P], then the select's scratch.
__global__ __launch_bounds__(SEL_THREADS) void exact_select(const unsigned long long *__restrict__ queue, int cap,
                                                            const unsigned *__restrict__ cnt,
                                                            const int *__restrict__ overflow,
                                                            const int *__restrict__ nonfinite, int K, int P,
                                                            int *__restrict__ out_idx, float *__restrict__ out_dist,
                                                            int *__restrict__ out_count, int *__restrict__ out_flags) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long sel_lds[];
  unsigned long long *sk = sel_lds;                        // [P]
  unsigned *hsub = reinterpret_cast<unsigned *>(sk + P);   // [256 * 8]
  unsigned *hist = hsub + 256 * 8;                         // [256]
  RadixSelectState &state = *reinterpret_cast<RadixSelectState *>(hist + 256);
  unsigned *nkept = hist + 256 + 4, *tie = nkept + 1;
  const int q = blockIdx.x, tid = threadIdx.x;
  if (overflow[q] | nonfinite[q]) return;   // answered by the fallback (uniform per workgroup)
  const unsigned c = cnt[q];
  const unsigned long long *Q = queue + (size_t)q * cap;
  const unsigned want = min((unsigned)K + 1u, c);
  if (tid == 0) { *nkept = 0u; *tie = 0u; }
  for (int e = tid; e < P; e += SEL_THREADS) sk[e] = ~0ull;
  if (want > 0) {
    const unsigned T = block_radix_select<SEL_THREADS>(
        [&](auto f) __attribute__((always_inline)) {
          for (unsigned e = tid; e < c; e += SEL_THREADS) f((unsigned)(Q[e] >> 32));
        },
        want, hsub, hist, state);
    const unsigned rank = state.remaining;   // of the wanted key among those whose distance word is T
    __syncthreads();                         // (the next select rewrites `state`)
    const unsigned R = block_radix_select<SEL_THREADS>(
        [&](auto f) __attribute__((always_inline)) {
          for (unsigned e = tid; e < c; e += SEL_THREADS) {
            const unsigned long long k = Q[e];
            if ((unsigned)(k >> 32) == T) f((unsigned)k);
          }
        },
        rank, hsub, hist, state);
    const unsigned long long cut = ((unsigned long long)T << 32) | R;
    for (unsigned e = tid; e < c; e += SEL_THREADS) {
      const unsigned long long k = Q[e];
      if (k <= cut) {
        const unsigned pos = atomicAdd(nkept, 1u);
        if (pos < (unsigned)P) sk[pos] = k;
      }
    }
  }
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j >= 1; j >>= 1) {
      for (int t = tid; t < P / 2; t += SEL_THREADS) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const unsigned long long a = sk[i], b = sk[l];
        const bool up = (i & k) == 0;
        if ((a > b) == up) { sk[i] = b; sk[l] = a; }
      }
      __syncthreads();
    }
  unsigned flags = 0;
  for (int e = tid; e < K; e += SEL_THREADS) {
    const bool ok = (unsigned)e < want;
    const unsigned long long k = ok ? sk[e] : 0ull;
    out_idx[(size_t)q * K + e] = ok ? (int)(unsigned)k : -1;
    out_dist[(size_t)q * K + e] = ok ? __uint_as_float((unsigned)(k >> 32)) : INFINITY;
    if (ok && (unsigned)e + 1u < want && (unsigned)(sk[e + 1] >> 32) == (unsigned)(k >> 32))
      flags |= (e == K - 1) ? GULON_FLAG_BOUNDARY_TIE : GULON_FLAG_INTERIOR_TIE;
  }
  if (flags) atomicOr(tie, flags);
  __syncthreads();
  if (tid == 0) {
    if (out_count) out_count[q] = (int)min((unsigned)K, want);
    if (out_flags) out_flags[q] = (int)*tie;
  }
}

// small k_nn: can one of the query's distances to rows of magnitude <= absmax overflow, or is it NaN?  Conservative:
// d * (absmax + max |q_e|)^2 below 3e38 keeps every partial sum finite.
__global__ void exact_screen(const float *__restrict__ Q, int B, int d, float absmax, int *__restrict__ nonfinite) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= B) return;
  float m = 0.f;
  bool bad = !(absmax < INFINITY);
  for (int e = 0; e < d; e++) {
    const float a = fabsf(Q[(size_t)q * d + e]);
    bad = bad || !(a < INFINITY);
    m = fmaxf(m, a);
  }
  const double s = (double)absmax + (double)m;
  nonfinite[q] = (bad || !((double)d * s * s < 3.0e38)) ? 1 : 0;
}

__global__ void exact_fill_empty(long long bk, int B, int *__restrict__ out_idx, float *__restrict__ out_dist,
                                 int *__restrict__ out_count, int *__restrict__ out_flags) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < bk) { out_idx[t] = -1; out_dist[t] = INFINITY; }
  if (t < B) {
    if (out_count) out_count[t] = 0;
    if (out_flags) out_flags[t] = 0;
  }
}

// out[t] = X[rows[t]] (a row outside [0, n): NaN, which the non-finite path then answers)
__global__ void exact_gather_rows(const float *__restrict__ X, int n, int d, const int *__restrict__ rows, int b,
                                  float *__restrict__ out) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)b * d) return;
  const int r = rows[t / d];
  out[t] = (r >= 0 && r < n) ? X[(size_t)r * d + t % d] : NAN;
}

// the fallback's sub-batch: out[f] = Q[ids[f]], and its answers back to the rows of the batch
__global__ void exact_gather_queries(const float *__restrict__ Q, int d, const int *__restrict__ ids, int F,
                                     float *__restrict__ out) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)F * d) return;
  out[t] = Q[(size_t)ids[t / d] * d + t % d];
}
__global__ void exact_scatter_answers(const int *__restrict__ ids, int F, int K, const int *__restrict__ ci,
                                      const float *__restrict__ cd, const int *__restrict__ cc,
                                      const int *__restrict__ cf, int *__restrict__ out_idx,
                                      float *__restrict__ out_dist, int *__restrict__ out_count,
                                      int *__restrict__ out_flags) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)F * K) return;
  const int f = (int)(t / K), e = (int)(t % K), q = ids[f];
  out_idx[(size_t)q * K + e] = ci[t];
  out_dist[(size_t)q * K + e] = cd[t];
  if (e == 0) {
    if (out_count) out_count[q] = cc[f];
    if (out_flags) out_flags[q] = cf[f];
  }
}

}  // namespace
}  // namespace gulon

using namespace gulon;

struct gulon_exact_index {
  const gulon_dataset *ds = nullptr;   // not owned: the dataset outlives the handle
  int from = 0, until = 0;
  float absmax = 0.f;                  // max |x| over the range, +inf if any value is NaN / inf
  int knob_sample = 0;                 // GULON_EXACT_SAMPLE: sample rows S (0: by k_nn, the range and the capacity)
  int knob_cap = 32768;                // GULON_EXACT_QUEUE_CAP: queue entries per query
  int64_t stats[6] = {0, 0, 0, 0, 0, 0};
  // scratch, grown on demand under `mu`
  DevBuf<float> qt, sample, tau;
  DevBuf<unsigned long long> queue;
  DevBuf<unsigned> cnt;
  DevBuf<int> overflow, nonfinite, ids, count_tmp, flags_tmp;
  DevBuf<float> fq, fd;
  DevBuf<int> fi, fc, ff;
  KnnScratch knn;                      // the single-pass / peeled path of knn.hip
  // the host-pointer forms
  DevBuf<float> stage_q, stage_od;
  DevBuf<int> stage_rows, stage_oi, stage_oc, stage_of;
  ExprWork expr;                       // the expression queries' term lists, composed vectors and answers at k_nn + extra
  CosmulWork cosmul;                   // the multiplicative analogy queries (cosmul.hip)
  OffsetWork offset;                   // the offset queries (offset.hip)
  RankWork rank;                       // the rank queries (rank.hip)
  LseWork lse;                         // the log-sum-exp queries (logsumexp.hip)
  std::vector<int> h_cnt, h_ovf, h_nf, h_ids;
  hipEvent_t order_ev = nullptr;
  hipStream_t order_st = nullptr;
  bool order_set = false;
  std::mutex mu;
  ~gulon_exact_index() {
    if (order_ev) (void)hipEventDestroy(order_ev);
  }
};

namespace {

bool set_knob(gulon_exact_index *h, const char *key, int v) {
  if (!strcmp(key, "GULON_EXACT_SAMPLE")) { h->knob_sample = v < 0 ? 0 : v; return true; }
  if (!strcmp(key, "GULON_EXACT_QUEUE_CAP")) { h->knob_cap = v < 16 ? 16 : v > (1 << 22) ? (1 << 22) : v; return true; }
  return false;
}

// Batches on different streams are ordered on the device: a batch waits for the event the last one recorded.
void order_wait(gulon_exact_index *h, hipStream_t st) {
  if (h->order_set && h->order_st != st) HIP_CHECK(hipStreamWaitEvent(st, h->order_ev, 0));
}
void order_record(gulon_exact_index *h, hipStream_t st) {
  if (!h->order_ev) HIP_CHECK(hipEventCreateWithFlags(&h->order_ev, hipEventDisableTiming));
  HIP_CHECK(hipEventRecord(h->order_ev, st));
  h->order_st = st;
  h->order_set = true;
}

// gulon_exact_knn's answer for b queries at d_q: the single-pass / peeled driver of knn.hip on the handle's range
void legacy_dev(gulon_exact_index *h, const float *d_q, int b, int K, int *oi, float *od, int *oc, int *of,
                hipStream_t st) {
  exact_knn_dev(h->ds, h->from, h->until, d_q, b, K, h->knn, oi, od, oc, of, st);
}

// k_nn <= GULON_MAX_K: knn_kernel's single pass.  It has no test for non-finite distances, so exact_screen flags the
// queries that may meet one; those go one at a time, the others in the runs between them.
void small_k_dev(gulon_exact_index *h, const float *dQ, int B, int K, int *oi, float *od, int *oc, int *of,
                 hipStream_t st) {
  const int d = h->ds->d;
  h->nonfinite.ensure(B);
  hipLaunchKernelGGL(exact_screen, dim3(ceil_div(B, 256)), dim3(256), 0, st, dQ, B, d, h->absmax, h->nonfinite.p);
  HIP_CHECK(hipGetLastError());
  h->h_nf.resize(B);
  h->nonfinite.download(h->h_nf.data(), B, st);
  HIP_CHECK(hipStreamSynchronize(st));
  int q = 0;
  while (q < B) {
    int e = q + 1;
    if (!h->h_nf[q]) while (e < B && !h->h_nf[e]) e++;
    legacy_dev(h, dQ + (size_t)q * d, e - q, K, oi + (size_t)q * K, od + (size_t)q * K, oc + q, of + q, st);
    if (h->h_nf[q]) h->stats[2]++; else h->stats[0] += e - q;
    q = e;
  }
}

void large_k_dev(gulon_exact_index *h, const float *dQ, int B, int K, int *oi, float *od, int *oc, int *of,
                 hipStream_t st) {
  const gulon_dataset *ds = h->ds;
  const int d = ds->d, from = h->from, range = h->until - h->from, cap = h->knob_cap;
  // the sample: none for a range the queue holds; else S rows, by default twice as many as make the expected fill
  // (k_nn + 1) * range / S equal to the capacity
  const bool sampled = range > cap;
  int S = 0;
  if (sampled) {
    long long s = h->knob_sample > 0 ? h->knob_sample
                                     : std::min<long long>(ceil_div(2LL * (K + 1) * range, cap), EXACT_SAMPLE_MAX);
    s = std::max<long long>(s, K + 1);
    S = (int)std::min<long long>(s, range);
  }
  const int want_tau = std::min(K + 1, S);
  int P = 2;
  while (P < std::min(K + 1, std::min(range, cap))) P <<= 1;
  const size_t sel_lds = (size_t)P * 8 + (256 * 8 + 256 + 8) * sizeof(unsigned);
  static std::mutex attr_mu;
  static size_t attr_set[16] = {0};
  {
    int dev = 0;
    HIP_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> g(attr_mu);
    if (dev < 0 || dev >= 16 || attr_set[dev] < sel_lds) {
      HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(exact_select),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)sel_lds));
      if (dev >= 0 && dev < 16) attr_set[dev] = sel_lds;
    }
  }
  // queries per sub-batch: whole tiles whose sample distances and queues fit the scratch budget
  const size_t per_query = (size_t)S * 4 + (size_t)cap * 8;
  int sub = (int)std::min<size_t>(EXACT_SCRATCH_BYTES / per_query, (size_t)1 << 20) / KNN_QT * KNN_QT;
  sub = std::max(sub, KNN_QT);
  sub = std::min(sub, ceil_div(B, KNN_QT) * KNN_QT);
  const int Bp = ceil_div(B, KNN_QT) * KNN_QT;
  h->qt.ensure((size_t)sub * d);
  h->sample.ensure((size_t)sub * S);
  h->queue.ensure((size_t)sub * cap);
  h->tau.ensure(sub);
  h->cnt.ensure(Bp); h->overflow.ensure(Bp); h->nonfinite.ensure(Bp);
  HIP_CHECK(hipMemsetAsync(h->cnt.p, 0, sizeof(unsigned) * Bp, st));
  HIP_CHECK(hipMemsetAsync(h->overflow.p, 0, sizeof(int) * Bp, st));
  HIP_CHECK(hipMemsetAsync(h->nonfinite.p, 0, sizeof(int) * Bp, st));
  const int cus = device_cus();
  for (int q0 = 0; q0 < B; q0 += sub) {
    const int b = std::min(sub, B - q0), ntiles = ceil_div(b, KNN_QT), bp = ntiles * KNN_QT;
    const float *dq = dQ + (size_t)q0 * d;
    const long long tq = (long long)ntiles * d * KNN_QT;
    hipLaunchKernelGGL(transpose_queries, dim3(ceil_div(tq, 256)), dim3(256), 0, st, dq, b, d, ntiles, h->qt.p);
    auto shape = [&](int total, int &per_chunk, int &nchunks) {   // about 64 workgroups per compute unit
      const RowChunks c = split_groups(row_groups(0, total), ceil_div((long long)cus * 64, ntiles));
      per_chunk = c.groups_per_chunk * KNN_THREADS;
      nchunks = c.nchunks;
    };
    int per_chunk = 0, nchunks = 0;
    if (sampled) {
      shape(S, per_chunk, nchunks);
      hipLaunchKernelGGL(exact_pass<true>, dim3(ntiles, nchunks), dim3(KNN_THREADS), 0, st, ds->x.p, d, h->qt.p, b, from,
                         range, S, per_chunk, h->sample.p, (const float *)nullptr, (unsigned long long *)nullptr, 0,
                         (unsigned *)nullptr, (int *)nullptr, (int *)nullptr);
      hipLaunchKernelGGL(exact_tau, dim3(bp), dim3(256), 0, st, h->sample.p, S, want_tau, b, h->tau.p);
    } else {
      hipLaunchKernelGGL(exact_tau_all, dim3(ceil_div(bp, 256)), dim3(256), 0, st, b, bp, h->tau.p);
    }
    shape(range, per_chunk, nchunks);
    hipLaunchKernelGGL(exact_pass<false>, dim3(ntiles, nchunks), dim3(KNN_THREADS), 0, st, ds->x.p, d, h->qt.p, b, from,
                       range, 0, per_chunk, (float *)nullptr, h->tau.p, h->queue.p, cap, h->cnt.p + q0, h->overflow.p + q0,
                       h->nonfinite.p + q0);
    hipLaunchKernelGGL(exact_select, dim3(b), dim3(SEL_THREADS), sel_lds, st, h->queue.p, cap, h->cnt.p + q0,
                       h->overflow.p + q0, h->nonfinite.p + q0, K, P, oi + (size_t)q0 * K, od + (size_t)q0 * K, oc + q0,
                       of + q0);
    HIP_CHECK(hipGetLastError());
  }
  // what the device flagged decides the rest of the batch: one small read
  h->h_cnt.resize(B); h->h_ovf.resize(B); h->h_nf.resize(B);
  h->cnt.download((unsigned *)h->h_cnt.data(), B, st);
  h->overflow.download(h->h_ovf.data(), B, st);
  h->nonfinite.download(h->h_nf.data(), B, st);
  HIP_CHECK(hipStreamSynchronize(st));
  h->h_ids.clear();
  int64_t fill = 0;
  for (int q = 0; q < B; q++) {
    fill = std::max<int64_t>(fill, (unsigned)h->h_cnt[q]);
    if (h->h_nf[q]) h->stats[2]++;
    else if (h->h_ovf[q]) h->h_ids.push_back(q);
    else h->stats[0]++;
  }
  h->stats[1] = (int64_t)h->h_ids.size();
  h->stats[3] = S; h->stats[4] = cap; h->stats[5] = fill;
  const int F = (int)h->h_ids.size();
  if (F > 0) {   // overflowed queues: the peeled path over the compacted sub-batch
    h->ids.upload(h->h_ids.data(), F, st);
    h->fq.ensure((size_t)F * d);
    h->fi.ensure((size_t)F * K); h->fd.ensure((size_t)F * K); h->fc.ensure(F); h->ff.ensure(F);
    hipLaunchKernelGGL(exact_gather_queries, dim3(ceil_div((long long)F * d, 256)), dim3(256), 0, st, dQ, d, h->ids.p, F,
                       h->fq.p);
    legacy_dev(h, h->fq.p, F, K, h->fi.p, h->fd.p, h->fc.p, h->ff.p, st);
    hipLaunchKernelGGL(exact_scatter_answers, dim3(ceil_div((long long)F * K, 256)), dim3(256), 0, st, h->ids.p, F, K,
                       h->fi.p, h->fd.p, h->fc.p, h->ff.p, oi, od, oc, of);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(st));   // (h_ids is read by the upload)
  }
  for (int q = 0; q < B; q++)   // a NaN / +inf distance: the answer of a batch of one
    if (h->h_nf[q]) legacy_dev(h, dQ + (size_t)q * d, 1, K, oi + (size_t)q * K, od + (size_t)q * K, oc + q, of + q, st);
}

// the body of every query form: device pointers, outputs [B][K] / [B] (count and flags may be null)
void exact_query_dev(gulon_exact_index *h, const float *dQ, int B, int K, int *oi, float *od, int *oc, int *of,
                     hipStream_t st) {
  GULON_REQUIRE(B >= 0 && K >= 0, "bad arguments");
  GULON_UNSUPPORTED(K > GULON_MAX_K_PEELED, "k_nn = %d > %d", K, GULON_MAX_K_PEELED);
  for (auto &s : h->stats) s = 0;
  h->stats[4] = h->knob_cap;
  if (B == 0) return;
  order_wait(h, st);
  if (!oc) { h->count_tmp.ensure(B); oc = h->count_tmp.p; }
  if (!of) { h->flags_tmp.ensure(B); of = h->flags_tmp.p; }
  const long long bk = (long long)B * K;
  if (K == 0 || h->from == h->until) {
    hipLaunchKernelGGL(exact_fill_empty, dim3(ceil_div(std::max<long long>(bk, B), 256)), dim3(256), 0, st, bk, B, oi, od,
                       oc, of);
    HIP_CHECK(hipGetLastError());
    h->stats[0] = B;
  } else if (K <= GULON_MAX_K) {
    small_k_dev(h, dQ, B, K, oi, od, oc, of, st);
  } else {
    large_k_dev(h, dQ, B, K, oi, od, oc, of, st);
  }
  order_record(h, st);
}

// Expression queries: compose over the dataset's rows -> the handle's own answer at k_nn + extra -> the
// term rows dropped, all on `st`.  The ids the handle returns are dataset rows, as the term rows are: row_base 0.
void exact_terms_dev(gulon_exact_index *h, const int *d_off, const int *d_rows, const float *d_w, int b, int k_nn,
                     int extra, bool nt, bool nq, int *oi, float *od, int *oc, int *of, hipStream_t st) {
  GULON_REQUIRE(b >= 0 && k_nn >= 0 && extra >= 0, "k, extra and batch size must be non-negative");
  GULON_UNSUPPORTED((long long)k_nn + extra > GULON_MAX_K_PEELED, "k_nn + extra = %lld > %d", (long long)k_nn + extra,
                    GULON_MAX_K_PEELED);
  if (b == 0) { for (auto &s : h->stats) s = 0; return; }
  ExprWork &x = h->expr;
  const int kin = k_nn + extra;
  x.q.ensure((size_t)b * h->ds->d);
  x.oi.ensure((size_t)b * kin + 1);
  x.od.ensure((size_t)b * kin + 1);
  x.oc.ensure((size_t)b);
  order_wait(h, st);   // the workspace may still be read by the last batch, on another stream
  launch_dataset_compose(h->ds, d_off, d_rows, d_w, b, nt, nq, x.q.p, nullptr, st);
  exact_query_dev(h, x.q.p, b, kin, x.oi.p, x.od.p, x.oc.p, of, st);
  launch_drop(x.oi.p, x.od.p, x.oc.p, b, kin, k_nn, d_off, d_rows, 0, oi, od, oc, st);
  order_record(h, st);
}

void exact_query_host(gulon_exact_index *h, const float *dQ, int b, int K, int32_t *out_idx, float *out_dist,
                      int32_t *out_count, int32_t *out_flags) {
  const size_t bk = (size_t)b * K;
  h->stage_oi.ensure(std::max<size_t>(bk, 1)); h->stage_od.ensure(std::max<size_t>(bk, 1));
  h->stage_oc.ensure(b); h->stage_of.ensure(b);
  exact_query_dev(h, dQ, b, K, h->stage_oi.p, h->stage_od.p, h->stage_oc.p, h->stage_of.p, nullptr);
  h->stage_oi.download(out_idx, bk); h->stage_od.download(out_dist, bk);
  if (out_count) h->stage_oc.download(out_count, b);
  if (out_flags) h->stage_of.download(out_flags, b);
  HIP_CHECK(hipDeviceSynchronize());
}

void gather_rows(gulon_exact_index *h, const int *d_rows, int b, hipStream_t st) {
  const int d = h->ds->d;
  h->stage_q.ensure((size_t)b * d);
  hipLaunchKernelGGL(exact_gather_rows, dim3(ceil_div((long long)b * d, 256)), dim3(256), 0, st, h->ds->x.p, h->ds->n, d,
                     d_rows, b, h->stage_q.p);
  HIP_CHECK(hipGetLastError());
}

}  // namespace

GULON_API int32_t gulon_exact_index_create(const gulon_dataset *ds, int32_t from, int32_t until, gulon_exact_index **out) {
  return guarded([&] {
    GULON_REQUIRE(ds != nullptr && out != nullptr, "dataset or out is null");
    GULON_REQUIRE(from <= until, "invalid range: expected from=%d <= until=%d", from, until);
    GULON_REQUIRE(until <= ds->n, "invalid range: expected until=%d <= vectors.length=%d", until, ds->n);
    GULON_REQUIRE(from >= 0, "invalid range: from=%d < 0", from);
    auto h = std::make_unique<gulon_exact_index>();
    h->ds = ds; h->from = from; h->until = until;
    if (const char *e = getenv("GULON_EXACT_SAMPLE")) set_knob(h.get(), "GULON_EXACT_SAMPLE", atoi(e));
    if (const char *e = getenv("GULON_EXACT_QUEUE_CAP")) set_knob(h.get(), "GULON_EXACT_QUEUE_CAP", atoi(e));
    h->absmax = centroid_absmax(ds->x.p + (size_t)from * ds->d, (long long)(until - from) * ds->d);
    *out = h.release();
  });
}

GULON_API int32_t gulon_exact_index_destroy(gulon_exact_index *idx) {
  return guarded([&] {
    if (idx) (void)hipDeviceSynchronize();
    delete idx;
  });
}

GULON_API int32_t gulon_exact_index_batch_query_dev(gulon_exact_index *idx, const float *d_queries, int32_t b,
                                                    int32_t k_nn, int32_t *d_out_idx, float *d_out_dist,
                                                    int32_t *d_out_count, int32_t *d_out_flags, void *stream) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    std::lock_guard<std::mutex> g(idx->mu);
    exact_query_dev(idx, d_queries, b, k_nn, d_out_idx, d_out_dist, d_out_count, d_out_flags, (hipStream_t)stream);
  });
}

GULON_API int32_t gulon_exact_index_batch_query(gulon_exact_index *idx, const float *queries, int32_t b, int32_t k_nn,
                                                int32_t *out_idx, float *out_dist, int32_t *out_count,
                                                int32_t *out_flags) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    GULON_REQUIRE(b >= 0 && k_nn >= 0, "bad arguments");
    std::lock_guard<std::mutex> g(idx->mu);
    if (b == 0) { for (auto &s : idx->stats) s = 0; return; }
    idx->stage_q.upload(queries, (size_t)b * idx->ds->d);
    exact_query_host(idx, idx->stage_q.p, b, k_nn, out_idx, out_dist, out_count, out_flags);
  });
}

GULON_API int32_t gulon_exact_index_query_rows_dev(gulon_exact_index *idx, const int32_t *d_rows, int32_t b,
                                                   int32_t k_nn, int32_t *d_out_idx, float *d_out_dist,
                                                   int32_t *d_out_count, int32_t *d_out_flags, void *stream) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    GULON_REQUIRE(b >= 0 && k_nn >= 0, "bad arguments");
    std::lock_guard<std::mutex> g(idx->mu);
    if (b > 0) gather_rows(idx, d_rows, b, (hipStream_t)stream);
    exact_query_dev(idx, idx->stage_q.p, b, k_nn, d_out_idx, d_out_dist, d_out_count, d_out_flags, (hipStream_t)stream);
  });
}

GULON_API int32_t gulon_exact_index_query_rows(gulon_exact_index *idx, const int32_t *rows, int32_t b, int32_t k_nn,
                                               int32_t *out_idx, float *out_dist, int32_t *out_count,
                                               int32_t *out_flags) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    GULON_REQUIRE(b >= 0 && k_nn >= 0, "bad arguments");
    for (int r = 0; r < b; r++)
      GULON_REQUIRE(rows[r] >= 0 && rows[r] < idx->ds->n, "row %d = %d outside [0, %d)", r, rows[r], idx->ds->n);
    std::lock_guard<std::mutex> g(idx->mu);
    if (b == 0) { for (auto &s : idx->stats) s = 0; return; }
    idx->stage_rows.upload(rows, b);
    gather_rows(idx, idx->stage_rows.p, b, nullptr);
    exact_query_host(idx, idx->stage_q.p, b, k_nn, out_idx, out_dist, out_count, out_flags);
  });
}

GULON_API int32_t gulon_exact_index_query_terms_dev(gulon_exact_index *idx, const int32_t *d_term_offsets,
                                                    const int32_t *d_term_rows, const float *d_term_weights, int32_t b,
                                                    int32_t k_nn, int32_t extra, int32_t normalize_terms,
                                                    int32_t normalize_query, int32_t *d_out_idx, float *d_out_dist,
                                                    int32_t *d_out_count, int32_t *d_out_flags, void *stream) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    std::lock_guard<std::mutex> g(idx->mu);
    exact_terms_dev(idx, d_term_offsets, d_term_rows, d_term_weights, b, k_nn, extra, normalize_terms != 0,
                    normalize_query != 0, d_out_idx, d_out_dist, d_out_count, d_out_flags, (hipStream_t)stream);
  });
}

GULON_API int32_t gulon_exact_index_query_terms(gulon_exact_index *idx, const int32_t *term_offsets,
                                                const int32_t *term_rows, const float *term_weights, int32_t b,
                                                int32_t k_nn, int32_t extra, int32_t normalize_terms,
                                                int32_t normalize_query, int32_t *out_idx, float *out_dist,
                                                int32_t *out_count, int32_t *out_flags) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    GULON_REQUIRE(b >= 0 && k_nn >= 0 && extra >= 0, "k, extra and batch size must be non-negative");
    const int terms = check_terms_host(term_offsets, term_rows, term_weights, b, idx->ds->n);
    std::lock_guard<std::mutex> g(idx->mu);
    ExprWork &x = idx->expr;
    const hipStream_t st = nullptr;
    const size_t bk = (size_t)b * (size_t)k_nn;
    if (b > 0) {
      x.off.upload(term_offsets, (size_t)b + 1, st);
      x.rows.upload(term_rows, (size_t)terms, st);
      x.w.upload(term_weights, (size_t)terms, st);
    }
    x.fi.ensure(bk + 1); x.fd.ensure(bk + 1); x.fc.ensure((size_t)b + 1); x.ff.ensure((size_t)b + 1);
    exact_terms_dev(idx, x.off.p, x.rows.p, x.w.p, b, k_nn, extra, normalize_terms != 0, normalize_query != 0, x.fi.p,
                    x.fd.p, x.fc.p, x.ff.p, st);
    if (bk) { x.fi.download(out_idx, bk, st); x.fd.download(out_dist, bk, st); }
    if (b > 0 && out_count) x.fc.download(out_count, (size_t)b, st);
    if (b > 0 && out_flags) x.ff.download(out_flags, (size_t)b, st);
    HIP_CHECK(hipStreamSynchronize(st));
  });
}

// Multiplicative analogy queries: cosmul.hip scores rows [from, until) of the dataset against the term
// rows, which are dataset rows as the returned ids are.
GULON_API int32_t gulon_exact_index_query_cosmul_dev(gulon_exact_index *idx, const int32_t *d_term_offsets,
                                                     const int32_t *d_term_rows, const float *d_term_weights, int32_t b,
                                                     int32_t k_nn, int32_t normalize, int32_t *d_out_idx,
                                                     float *d_out_score, int32_t *d_out_count, int32_t *d_err,
                                                     void *stream) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    std::lock_guard<std::mutex> g(idx->mu);
    const hipStream_t st = (hipStream_t)stream;
    order_wait(idx, st);
    launch_cosmul_exact(idx->ds, idx->from, idx->until, idx->cosmul, d_term_offsets, d_term_rows, d_term_weights, b,
                        k_nn, normalize != 0, d_out_idx, d_out_score, d_out_count, d_err, st);
    if (b > 0) order_record(idx, st);
  });
}

GULON_API int32_t gulon_exact_index_query_cosmul(gulon_exact_index *idx, const int32_t *term_offsets,
                                                 const int32_t *term_rows, const float *term_weights, int32_t b,
                                                 int32_t k_nn, int32_t normalize, int32_t *out_idx, float *out_score,
                                                 int32_t *out_count) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    const int terms = check_cosmul_host(term_offsets, term_rows, term_weights, b, idx->ds->n, k_nn, nullptr);
    if (b == 0) return;
    std::lock_guard<std::mutex> g(idx->mu);
    CosmulWork &x = idx->cosmul;
    const hipStream_t st = nullptr;
    const size_t bk = (size_t)b * (size_t)k_nn;
    x.off.upload(term_offsets, (size_t)b + 1, st);
    x.rows.upload(term_rows, (size_t)terms, st);
    x.w.upload(term_weights, (size_t)terms, st);
    x.fi.ensure(bk + 1); x.fd.ensure(bk + 1); x.fc.ensure((size_t)b);
    order_wait(idx, st);
    launch_cosmul_exact(idx->ds, idx->from, idx->until, x, x.off.p, x.rows.p, x.w.p, b, k_nn, normalize != 0,
                        x.fi.p, x.fd.p, x.fc.p, nullptr, st);
    order_record(idx, st);
    if (bk) { x.fi.download(out_idx, bk, st); x.fd.download(out_score, bk, st); }
    if (out_count) x.fc.download(out_count, (size_t)b, st);
    HIP_CHECK(hipStreamSynchronize(st));
  });
}

// Offset queries: offset.hip ranks rows [from, until) of the dataset by distance + row_offsets[row]; the
// offsets and the excluded rows are indexed by dataset row, as the returned ids are.
GULON_API int32_t gulon_exact_index_query_offset_dev(gulon_exact_index *idx, const float *d_queries, int32_t b,
                                                     int32_t k_nn, const float *d_row_offsets, const int32_t *d_exclude,
                                                     int32_t *d_out_idx, float *d_out_key, int32_t *d_out_count,
                                                     void *stream) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    std::lock_guard<std::mutex> g(idx->mu);
    const hipStream_t st = (hipStream_t)stream;
    order_wait(idx, st);
    launch_offset_exact(idx->ds, idx->from, idx->until, idx->offset, d_queries, b, k_nn, d_row_offsets, d_exclude,
                        d_out_idx, d_out_key, d_out_count, st);
    if (b > 0) order_record(idx, st);
  });
}

GULON_API int32_t gulon_exact_index_query_offset(gulon_exact_index *idx, const float *queries, int32_t b, int32_t k_nn,
                                                 const float *row_offsets, const int32_t *exclude, int32_t *out_idx,
                                                 float *out_key, int32_t *out_count) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    check_offset_host(row_offsets, idx->ds->n, exclude, b, k_nn, 0);
    if (b == 0) return;
    GULON_REQUIRE(queries != nullptr && out_idx != nullptr && out_key != nullptr, "null argument");
    std::lock_guard<std::mutex> g(idx->mu);
    OffsetWork &x = idx->offset;
    const hipStream_t st = nullptr;
    const size_t bk = (size_t)b * (size_t)k_nn;
    order_wait(idx, st);   // the workspace may still be read by the last batch, on another stream
    x.q.upload(queries, (size_t)b * idx->ds->d, st);
    x.off.upload(row_offsets, (size_t)idx->ds->n, st);
    x.off.ensure(1);
    if (exclude) x.ex.upload(exclude, (size_t)b, st);
    x.fi.ensure(bk); x.fd.ensure(bk); x.fc.ensure((size_t)b);
    launch_offset_exact(idx->ds, idx->from, idx->until, x, x.q.p, b, k_nn, x.off.p, exclude ? x.ex.p : nullptr, x.fi.p,
                        x.fd.p, x.fc.p, st);
    order_record(idx, st);
    x.fi.download(out_idx, bk, st); x.fd.download(out_key, bk, st);
    if (out_count) x.fc.download(out_count, (size_t)b, st);
    HIP_CHECK(hipStreamSynchronize(st));
  });
}

// Rank queries: rank.hip counts the rows of [from, until) that the offset query above would put before the
// best row of each query's gold list; offsets, excluded rows and gold rows are dataset rows.  Host pointers, the null
// stream.
GULON_API int32_t gulon_exact_index_query_rank(gulon_exact_index *idx, const float *queries, int32_t b,
                                               const float *row_offsets, const int32_t *exclude,
                                               const int32_t *gold_offsets, const int32_t *gold_rows, int32_t *out_rank,
                                               int32_t *out_row, float *out_key, int32_t *out_total) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    GULON_REQUIRE(b >= 0, "batch size must be non-negative");
    if (b == 0) return;
    const int gold = check_rank_host(row_offsets, idx->ds->n, exclude, gold_offsets, gold_rows, b, 0);
    GULON_REQUIRE(queries != nullptr && out_rank != nullptr && out_row != nullptr && out_key != nullptr, "null argument");
    std::lock_guard<std::mutex> g(idx->mu);
    RankWork &x = idx->rank;
    const hipStream_t st = nullptr;
    order_wait(idx, st);   // the workspace may still be read by the last batch, on another stream
    x.q.upload(queries, (size_t)b * idx->ds->d, st);
    if (row_offsets) x.off.upload(row_offsets, (size_t)idx->ds->n, st);
    if (exclude) x.ex.upload(exclude, (size_t)b, st);
    x.goff.upload(gold_offsets, (size_t)b + 1, st);
    x.grows.upload(gold_rows, (size_t)gold, st);
    x.grows.ensure(1);
    x.frank.ensure((size_t)b); x.frow.ensure((size_t)b); x.fk.ensure((size_t)b); x.ftotal.ensure((size_t)b);
    launch_rank_exact(idx->ds, idx->from, idx->until, x, x.q.p, b, row_offsets ? x.off.p : nullptr,
                      exclude ? x.ex.p : nullptr, x.goff.p, x.grows.p, gold, x.frank.p, x.frow.p, x.fk.p, x.ftotal.p, st);
    order_record(idx, st);
    x.frank.download(out_rank, (size_t)b, st); x.frow.download(out_row, (size_t)b, st);
    x.fk.download(out_key, (size_t)b, st);
    if (out_total) x.ftotal.download(out_total, (size_t)b, st);
    HIP_CHECK(hipStreamSynchronize(st));
  });
}

// Log-sum-exp queries: logsumexp.hip sums exp(-(beta / 2) * distance) over the rows of [from, until) per
// query, in binary64 and in a fixed order, and takes the log; the excluded rows are dataset rows.  Host pointers, the
// null stream.
GULON_API int32_t gulon_exact_index_query_logsumexp(gulon_exact_index *idx, const float *queries, int32_t b, float beta,
                                                    const int32_t *exclude, double *out_lse, int32_t *out_terms) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    GULON_REQUIRE(b >= 0, "batch size must be non-negative");
    GULON_REQUIRE(std::isfinite(beta) && beta > 0.f, "beta = %g: expected a finite value > 0", (double)beta);
    check_rows_host(nullptr, true, idx->ds->n, exclude, b, 0);
    if (b == 0) return;
    GULON_REQUIRE(queries != nullptr && out_lse != nullptr, "null argument");
    std::lock_guard<std::mutex> g(idx->mu);
    LseWork &x = idx->lse;
    const hipStream_t st = nullptr;
    order_wait(idx, st);   // the workspace may still be read by the last batch, on another stream
    x.q.upload(queries, (size_t)b * idx->ds->d, st);
    if (exclude) x.ex.upload(exclude, (size_t)b, st);
    x.fl.ensure((size_t)b); x.ft.ensure((size_t)b);
    launch_logsumexp_exact(idx->ds, idx->from, idx->until, x, x.q.p, b, -0.5 * (double)beta, exclude ? x.ex.p : nullptr,
                           x.fl.p, x.ft.p, st);
    order_record(idx, st);
    x.fl.download(out_lse, (size_t)b, st);
    if (out_terms) x.ft.download(out_terms, (size_t)b, st);
    HIP_CHECK(hipStreamSynchronize(st));
  });
}

#ifdef GULON_TEST_HOOKS
// Which launch geometry gulon_exact_index_query_cosmul[_dev] takes for b questions on this handle's range
// (tests/test_gpu_cosmul_paths.py): out = {questions per pass, row chunks of the first pass, 256-row groups per chunk}, by
// the launcher's own cosmul_exact_shape.  Here because the handle's range is: host code, nothing is launched.
GULON_API int32_t gulon_selftest_cosmul_exact_shape(const gulon_exact_index *idx, int32_t b, int32_t out[3]) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr && out != nullptr && b >= 1, "bad arguments");
    const CosmulShape s = cosmul_exact_shape(idx->from, idx->until, b);
    out[0] = s.per_pass; out[1] = s.nchunks; out[2] = s.per_chunk;
  });
}
#endif

GULON_API int32_t gulon_exact_index_tuning(gulon_exact_index *idx, const char *key, int32_t value) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr && key != nullptr, "index or key is null");
    std::lock_guard<std::mutex> g(idx->mu);
    GULON_REQUIRE(set_knob(idx, key, value), "unknown tuning key %s", key);
  });
}

GULON_API int32_t gulon_exact_index_stats(gulon_exact_index *idx, int64_t *out) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr && out != nullptr, "index or out is null");
    std::lock_guard<std::mutex> g(idx->mu);
    for (int i = 0; i < 6; i++) out[i] = idx->stats[i];
  });
}
