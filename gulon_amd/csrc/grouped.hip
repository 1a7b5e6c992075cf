// GroupedIndex (Index.scala:231-308): coarse groups + product-quantized residuals.
//
//   query(k, q):  nn = searchSpace(q)                       nearest coarse centroids (TopKHeap + deleteAll)
//                 for c in nn:  residual = q - centroid(c)   MathUtils.subtract
//                               heap.merge(vectorIndex.query(k, residual, from(c), until(c)))
//                 Result.fromHeap(heap)
//
// The per-group heaps are merged with TopKHeap.merge, i.e. update() of the other heap's slots in
// ARRAY order, so under distance ties the answer depends on the literal heaps.  Kernels:
//   gq_cdist            query x centroid distances (MathUtils.distanceSq order), centroids transposed
//   gq_nearest_groups   LimitGroups(<= 63): literal TopKHeap in registers (lane = slot) + deleteAll
//   gq_select_groups    LimitGroups(> 63) of many groups: radix select of the limit-th distance, sort of the selected
//   gq_sorted_groups    LimitVectors / the other limits: (distance, id) bitonic sort, cut by rows or count
//   gq_literal_groups   the reference's heap for queries whose groups hang on equal centroid distances
//   gq_approx_scan      (or the by-group filter of grouped_filter.hip) the 64 rows of a query's searched groups
//                       with the smallest approximate distance, from one table per query ...
//   gq_rerank           ... re-scored with the reference's arithmetic and certified; a query that is not
//                       certified, has equal distances among its K+1 best or saw a NaN is appended to a list ...
//   gq_group_scan + gq_merge   ... and redone literally.  Workgroup = 4 (query, searched group) pairs, one
//                       wave each: the residual's m x k table in LDS (Index.prepareQuery arithmetic; each
//                       quantizer's codebook staged once per workgroup, transposed), then the group's rows
//                       64 at a time (PQIndex.distances order) through the reference's TopKHeap, fed in row
//                       order, stored in array order; TopKHeap.merge of the group heaps in search order +
//                       Result.fromHeap.  Ids and order therefore equal the reference's also under ties.
//                       Every query takes this way for k_nn > 63, on an index without rows and with
//                       GULON_GROUPED_LITERAL=1; gq_group_scan_wide does the same over 16-bit codes.
// Offset queries: gulon_grouped_index_query_offset runs coarse_stage per pass and hands its groups and the
// handle's GroupedOffsetWork to grouped_offset.hip.
#include "scan.hpp"

#include "grouped_filter.hpp"
#include "grouped_offset.hpp"
#include "offset.hpp"
#include "select.hpp"
#include "topk_heap.hpp"
using gulon::DevBuf;

struct gulon_grouped_index {
  gulon_index *pq = nullptr;       // residual codes + residual codebooks (row-blocked layout of scan.hip)
  int32_t n = 0, d = 0, g = 0;
  DevBuf<float> gcent, gcent_t;    // [g][d] centroids of the non-empty groups, and the [d][g] transpose
  DevBuf<int> bounds;              // [g+1] first row of every group, then n
  // scratch (grown on demand under mu)
  DevBuf<float> q_dev, cdist, hv, od;
  DevBuf<int> nn, nn_cnt, hk, hs, oi, oc, qlist, qcount, sel_ok, lit_flag;
  DevBuf<int> rows_dev;            // row ids of the host-pointer lookup / query-by-row calls
  DevBuf<float> lq;                // decoded queries of gulon_grouped_index_query_rows_dev
  DevBuf<float> wide_tables;       // k > 256: residual tables, one slot per workgroup of gq_group_scan_wide
  // approximate pre-selection (gq_approx_scan): |g + decode(codes_i)|^2 per row, its maximum, per-query tables, lists
  DevBuf<float> xnorm, ptab, apv, amv;
  DevBuf<int> api, ami, anan;
  gulon::GroupedOffsetWork offset;   // offset queries (grouped_offset.hip)
  gulon::GroupFilter gfilter;     // the same pre-selection batched by group with 8-bit bound tables (grouped_filter.hip)
  float xnmax = 0.f;
  int n_empty = 0;                 // groups without rows (the reference's leading empty group, WordVectors.scala:38-39)
  std::mutex mu;
  ~gulon_grouped_index() { if (pq) gulon_index_destroy(pq); }
};

namespace gulon {
namespace {

// ---- coarse search: distances of every query to every group centroid -------------------------
// MathUtils.distanceSq(centroid, query): sum of (q_e - c_e)^2, e ascending, unfused.
// gcent_t is the [d][g] transpose: consecutive threads (centroids) read consecutive addresses.
// A thread takes one centroid and CD_Q queries: the centroid's coordinates are read once for all of them (one query
// per thread re-read the 5 MB of centroids per query: 5 GB through L2 per batch, 0.33 ms at 10 001 groups).
constexpr int CD_Q = 8;
__global__ __launch_bounds__(256) void gq_cdist(const float *__restrict__ gcent_t, int g, int d,
                                                const float *__restrict__ Q, int B, float *__restrict__ out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x, q0 = blockIdx.y * CD_Q;
  if (c >= g) return;
  const int nq = min(CD_Q, B - q0);
  float sum[CD_Q];
#pragma unroll
  for (int i = 0; i < CD_Q; i++) sum[i] = 0.f;
  for (int e = 0; e < d; e++) {
    const float ce = gcent_t[(size_t)e * g + c];
#pragma unroll
    for (int i = 0; i < CD_Q; i++) {
      const float dx = Q[(size_t)(q0 + min(i, nq - 1)) * d + e] - ce;     // (wave-uniform address: a scalar load)
      sum[i] += dx * dx;
    }
  }
#pragma unroll
  for (int i = 0; i < CD_Q; i++)
    if (i < nq) out[(size_t)(q0 + i) * g + c] = sum[i];
}

// LimitGroups(limit <= 63): literal exactNearestNeighbours(centroids, query, limit).deleteAll()
__global__ __launch_bounds__(64) void gq_nearest_groups(const float *__restrict__ cdist, int g, int limit,
                                                        int *__restrict__ nn /*[B][stride]*/, int stride,
                                                        int *__restrict__ nn_cnt) {
  const int q = blockIdx.x, lane = threadIdx.x;
  RegHeap h(limit, lane);
  const float *dq = cdist + (size_t)q * g;
  for (int base = 0; base < g; base += 64) {
    const bool have = base + lane < g;
    const float dv = have ? dq[base + lane] : 0.f;
    // centroids in index order through heap.update; the ballot only skips those the heap would reject
    unsigned long long mk = __ballot(have && h.would_insert(dv));
    while (mk) {
      const int l = __ffsll((long long)mk) - 1;
      mk &= mk - 1;
      const float x = readlane_f(dv, l);
      if (h.would_insert(x)) h.update(base + l, x);
    }
  }
  const int live = h.size;
  h.drain([&](int i, int kk, float) { if (lane == 0) nn[(size_t)q * stride + i] = kk; });   // deleteAll()
  if (lane == 0) nn_cnt[q] = live;
}

// LimitVectors(limit) (and LimitGroups beyond 63): all centroids in ascending (distance, id)
// order -- the reference's heap order wherever no two centroid distances are equal -- cut after
// enough groups to cover `limit` rows (or after `limit` groups).  One workgroup per query, bitonic
// sort in LDS.
__global__ __launch_bounds__(256) void gq_sorted_groups(const float *__restrict__ cdist, int g, int n2,
                                                        const int *__restrict__ bounds, int by_vectors, int limit,
                                                        int *__restrict__ nn, int stride, int *__restrict__ nn_cnt,
                                                        const int *__restrict__ done, int *__restrict__ lit) {
  extern __shared__ float gs_lds[];
  if (done && done[blockIdx.x]) return;   // gq_select_groups already answered this query
  float *sv = gs_lds;
  int *si = reinterpret_cast<int *>(gs_lds + n2);
  __shared__ int s_lit;
  const int q = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) s_lit = 0;
  __syncthreads();
  for (int e = tid; e < n2; e += 256) {
    float v = e < g ? cdist[(size_t)q * g + e] : INFINITY;
    if (v != v) s_lit = 2;            // a NaN distance: only the literal heap knows what the reference does with it
    sv[e] = v != v ? INFINITY : v;    // NaN distances order last
    si[e] = e < g ? e : INT_MAX;
  }
  __syncthreads();
  for (int k = 2; k <= n2; k <<= 1)
    for (int j = k >> 1; j >= 1; j >>= 1) {
      for (int i = tid; i < n2; i += 256) {
        const int l = i ^ j;
        if (l > i) {
          const float a = sv[i], b = sv[l];
          const int ai = si[i], bi = si[l];
          const bool gt = a > b || (a == b && ai > bi);
          if (gt == ((i & k) == 0)) { sv[i] = b; sv[l] = a; si[i] = bi; si[l] = ai; }
        }
      }
      __syncthreads();
    }
  if (tid == 0) {
    int i = 0;
    if (by_vectors) {
      int count = 0;
      while (i < g && count < limit) { const int c = si[i]; count += bounds[c + 1] - bounds[c]; i++; }
    } else {
      i = min(limit, g);
    }
    nn_cnt[q] = i;
  }
  __syncthreads();
  const int cnt = nn_cnt[q];
  for (int e = tid; e < cnt; e += 256) nn[(size_t)q * stride + e] = si[e];
  // (distance, id) order is the reference's heap order only while the entries that decide the answer -- the
  // searched ones and the first one left out -- have pairwise different distances; otherwise gq_literal_groups
  // redoes this query (equal centroid distances are common: the reference's leading empty group repeats a centroid)
  // level 2: the searched SET hangs on the heap's order -- redone before the scan: the tie sits AT the cut (or a NaN is
  // around), or, cutting by rows, between the LAST TWO searched groups: the cut is cumulative, so with the larger twin
  // first the heap reaches `limit` rows one group earlier and never opens the other (a tie class further inside adds
  // the same rows in either order); level 1: only the ORDER of searched groups does, which matters solely
  // to queries whose RESULT is later redone literally (TopKHeap.merge runs in search order) -- those are redone then
  for (int e = tid; e + 1 < min(cnt + 1, g); e += 256)
    if (sv[e] == sv[e + 1]) atomicMax(&s_lit, e + 1 == cnt || (by_vectors && e + 2 == cnt) ? 2 : 1);
  __syncthreads();
  if (tid == 0) lit[q] = s_lit;
}

// LimitGroups(limit) for limit > 63 (the CLI's default is 5 % of the groups): only the `limit` nearest
// centroids are needed, so instead of sorting all g distances the limit-th smallest key is found
// by a 4-pass radix select on the float bits (distances are >= +0: unsigned order), everything at or
// below it is compacted (limit + ties entries) and only that is sorted by (distance, id).
// ok[q] = 0 if more than `cap` entries tie at the threshold (the caller then sorts everything).
// KR > 0: the query's g <= 256 KR keys are read ONCE and kept in registers through the four counting passes and the
// compaction (the kernel is one workgroup's latency -- all B of them are resident at once: five trips through the
// 40 KB of a query's distances and a 256-step serial walk over the bins per pass were most of its 134 us); KR = 0: any g,
// from memory.
template <int KR>
__global__ __launch_bounds__(256) void gq_select_groups(const float *__restrict__ cdist, int g, int limit, int cap,
                                                        int *__restrict__ nn, int stride,
                                                        int *__restrict__ nn_cnt, int *__restrict__ ok,
                                                        int *__restrict__ lit) {
  extern __shared__ float sel_lds[];
  float *sv = sel_lds;                                     // [cap]
  int *si = reinterpret_cast<int *>(sel_lds + cap);        // [cap]
  __shared__ unsigned hist[256], hsub[256 * 8];
  __shared__ RadixSelectState s_sel;
  __shared__ int s_count, s_lit;
  const int q = blockIdx.x, tid = threadIdx.x;
  const float *dq = cdist + (size_t)q * g;
  auto keyof = [&](int c) { const float v = dq[c]; return v != v ? 0x7F800000u : __float_as_uint(v); };   // NaN orders last
  const int want = min(limit, g);
  if (tid == 0) { s_count = 0; s_lit = 0; }
  constexpr int KRN = KR > 0 ? KR : 1;
  unsigned kreg[KRN];                                      // key of centroid tid + 256 r (0xFFFFFFFF: none)
  bool any_nan = false;
  if (KR > 0) {
#pragma unroll
    for (int r = 0; r < KRN; r++) {
      const int c = tid + 256 * r;
      const float v = c < g ? dq[c] : 0.f;
      any_nan = any_nan || v != v;
      kreg[r] = c < g ? (v != v ? 0x7F800000u : __float_as_uint(v)) : 0xFFFFFFFFu;
    }
  }
  __syncthreads();
  auto each = [&](auto f) __attribute__((always_inline)) {   // f(key, centroid) for every key of this thread
    if (KR > 0) {
#pragma unroll
      for (int r = 0; r < KRN; r++)
        if (kreg[r] != 0xFFFFFFFFu) f(kreg[r], tid + 256 * r);
    } else {
      for (int c = tid; c < g; c += 256) f(keyof(c), c);
    }
  };
  auto keys = [&](auto f) __attribute__((always_inline)) { each([&](unsigned key, int) __attribute__((always_inline)) { f(key); }); };
  const unsigned thr = block_radix_select<256>(keys, (unsigned)want, hsub, hist, s_sel);   // key of the want-th smallest distance
  if (KR > 0 && any_nan) s_lit = 2;                        // NaN distance: literal heap (gq_literal_groups)
  each([&](unsigned key, int c) __attribute__((always_inline)) {
    if (KR == 0 && dq[c] != dq[c]) s_lit = 2;
    if (key <= thr) {
      const int p = atomicAdd(&s_count, 1);
      if (p < cap) { sv[p] = __uint_as_float(key); si[p] = c; }
    }
  });
  __syncthreads();
  const int cnt = s_count;
  if (cnt > cap) {                                         // a huge tie at the threshold
    if (tid == 0) ok[q] = 0;
    return;
  }
  int n2 = 64;
  while (n2 < cnt) n2 <<= 1;
  for (int e = cnt + tid; e < n2; e += 256) { sv[e] = INFINITY; si[e] = INT_MAX; }
  __syncthreads();
  for (int k = 2; k <= n2; k <<= 1)
    for (int j = k >> 1; j >= 1; j >>= 1) {
      for (int i = tid; i < n2; i += 256) {
        const int l = i ^ j;
        if (l > i) {
          const float a = sv[i], b = sv[l];
          const int ai = si[i], bi = si[l];
          const bool gt = a > b || (a == b && ai > bi);
          if (gt == ((i & k) == 0)) { sv[i] = b; sv[l] = a; si[i] = bi; si[l] = ai; }
        }
      }
      __syncthreads();
    }
  for (int e = tid; e < want; e += 256) nn[(size_t)q * stride + e] = si[e];
  // equal distances among the searched groups or at the cut (every entry at the threshold was compacted, so a tie
  // there shows as cnt > want): the reference's heap order decides, not (distance, id) -- gq_literal_groups
  for (int e = tid; e + 1 < min(want + 1, cnt); e += 256)
    if (sv[e] == sv[e + 1]) atomicMax(&s_lit, e + 1 == want ? 2 : 1);   // levels: see gq_sorted_groups
  __syncthreads();
  if (tid == 0) { nn_cnt[q] = want; ok[q] = 1; lit[q] = s_lit; }
}

// exactNearestNeighbours(centroids, query, cap).deleteAll() (Index.scala:209-229, :287,:290) LITERALLY, for the
// queries gq_sorted_groups / gq_select_groups flagged: a TopKHeap of capacity `cap` (LimitGroups: the limit;
// LimitVectors: all g groups) in LDS, fed the centroid distances in index order, drained in place like heapsort
// (deleteAll fills its result from the back: slot `size` is free the moment delete() returns).  One wavefront per
// query (LdsHeap: every lane runs the same scalar heap code, lane 0 stores) and only the scan for centroids the heap
// would take is spread over the lanes.
__global__ __launch_bounds__(64) void gq_literal_groups(const float *__restrict__ cdist, int g, int cap,
                                                        const int *__restrict__ bounds, int by_vectors, int limit,
                                                        const int *__restrict__ lit, int level, const int *__restrict__ qlist,
                                                        const int *__restrict__ qcount, int *__restrict__ nn, int stride,
                                                        int *__restrict__ nn_cnt) {
  extern __shared__ float lg_lds[];
  const int lane = threadIdx.x;
  // level 2: every query whose searched set hangs on a tie (grid = B); level 1: the listed queries (redone literally)
  // whose group ORDER does (grid = a few workgroups walking qlist)
  const int nq = qlist ? *qcount : (int)gridDim.x;
  for (int fy = blockIdx.x; fy < nq; fy += gridDim.x) {
  const int q = qlist ? qlist[fy] : fy;
  if (lit[q] != level) continue;
  LdsHeap h(lg_lds, reinterpret_cast<int *>(lg_lds + cap), cap, lane);   // [cap] values, then [cap] keys
  const float *dq = cdist + (size_t)q * g;
  bool has_nan = false;
  for (int c = lane; c < g; c += 64) has_nan = has_nan || dq[c] != dq[c];
  has_nan = __any(has_nan);
  for (int base = 0; base < g; base += 64) {
    const bool have = base + lane < g;
    const float dv = have ? dq[base + lane] : 0.f;
    // with a NaN around the heap is not ordered and every centroid goes through update; otherwise its root only falls
    unsigned long long mk = __ballot(have && (has_nan || h.size < cap || h.val(0) > dv));
    while (mk) {
      const int l = __ffsll((long long)mk) - 1;
      mk &= mk - 1;
      h.update(base + l, readlane_f(dv, l));
    }
  }
  const int live = h.size;
  h.drain([&](int j, int kk, float x) { h.put(j, kk, x); });    // deleteAll(), in place: slot j is outside the heap now
  int cnt = live;
  if (by_vectors) {                                             // searchSpace, Index.scala:289-298
    int i = 0, count = 0;
    while (i < live && count < limit) { const int c = h.key(i); count += bounds[c + 1] - bounds[c]; i++; }
    cnt = i;
  }
  cnt = min(cnt, stride);
  for (int e = lane; e < cnt; e += 64) nn[(size_t)q * stride + e] = h.key(e);
  if (lane == 0) nn_cnt[q] = cnt;
  }
}

// ---- one searched group of one query -------------------------------------------------------------
// The group's literal TopKHeap, fed in row order and stored in array order: K entries per pair in hk/hv, the
// heap's size in hs.  With a query list (qlist/qcount on the device) only the listed queries are processed --
// the ones gq_rerank flagged.
constexpr int GQ_WAVES = 4;    // (query, group) pairs per workgroup: they share the staged codebook slices
constexpr int GQ_RPT = 8;      // centroid components prefetched per thread (sub-vectors up to 8 wide are fully overlapped)
constexpr int GQ_PD = 4;       // quantizers whose codebooks are in flight
template <int VEC, bool BIG = false /* k_nn > 63: the literal heap in LDS */>
__global__ __launch_bounds__(64 * GQ_WAVES) void gq_group_scan(const uint8_t *__restrict__ codes, int ng, int m, int m_pad, int k,
                                                    int d, const float *__restrict__ pq_cents,
                                                    const int *__restrict__ from, const int *__restrict__ sdim,
                                                    const float *__restrict__ gcent, const int *__restrict__ bounds,
                                                    const float *__restrict__ Q, const int *__restrict__ nn,
                                                    int nn_stride, const int *__restrict__ nn_cnt, int stride, int K,
                                                    int *__restrict__ hk, float *__restrict__ hv,
                                                    int *__restrict__ hs, const int *__restrict__ qlist,
                                                    const int *__restrict__ qcount, int slice_floats) {
  using Word = typename CodeWord<VEC>::type;
  // per wave: m_pad * 256 table entries + d residual components; then one codebook slice (k * smax floats)
  extern __shared__ float gq_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t = blockIdx.x * GQ_WAVES + wave;           // searched-group slot of this wave
  float *gtab = gq_lds + (size_t)wave * (m_pad * 256 + d);
  float *res = gtab + m_pad * 256;
  float *slice = gq_lds + (size_t)GQ_WAVES * (m_pad * 256 + d);
  const int nq = qlist ? *qcount : (int)gridDim.y;
  for (int fy = blockIdx.y; fy < nq; fy += gridDim.y) {
  const int q = qlist ? qlist[fy] : fy;
  const bool live = t < nn_cnt[q];                       // wave-uniform; dead waves still help staging
  const int c = live ? nn[(size_t)q * nn_stride + t] : 0;
  __syncthreads();
  if (live)
    for (int e = lane; e < d; e += 64) res[e] = Q[(size_t)q * d + e] - gcent[(size_t)c * d + e];   // MathUtils.subtract
  // Index.prepareQuery on the residual: T[j][c'] = sum_e (r[from_j+e] - cent_j[c'][e])^2, e ascending, unfused.
  // The codebook of quantizer j (k * s_j contiguous floats) is staged once for the four pairs.
  // The codebooks of the next GQ_PD quantizers are in flight in registers (GQ_RPT floats per thread
  // each) while this one is used: at two workgroups per CU a single global round trip costs more
  // than a quantizer's 256 x s table entries (LDS holds one slice at a time).
  static_assert(64 * GQ_WAVES == 256, "thread = centroid staging assumes 256 threads");
  float pre[GQ_PD][GQ_RPT];
  // thread = centroid (k <= 256 = GQ_THREADS): component x of its centroid, no index arithmetic
  auto fetch = [&](int j, float (&dst)[GQ_RPT]) {
    const int fr = j < m ? from[j] : 0, sj = j < m ? sdim[j] : 0;
    const float *cent = pq_cents + (size_t)k * fr + (size_t)tid * sj;
#pragma unroll
    for (int u = 0; u < GQ_RPT; u++) dst[u] = (tid < k && u < sj) ? cent[u] : 0.f;
  };
#pragma unroll
  for (int p = 0; p < GQ_PD; p++) fetch(p, pre[p]);
  for (int j0 = 0; j0 < m_pad; j0 += GQ_PD) {            // m_pad is a multiple of 4
#pragma unroll
    for (int p = 0; p < GQ_PD; p++) {
      const int j = j0 + p;
      const int fr = j < m ? from[j] : 0, sj = j < m ? sdim[j] : 0;
      float *sl = slice;
      __syncthreads();                                   // slice j-1 is no longer read
      // stored transposed, [x][centroid]: the lanes of a wave then read consecutive addresses
#pragma unroll
      for (int u = 0; u < GQ_RPT; u++)
        if (u < sj) sl[u * 256 + tid] = pre[p][u];
      for (int x = GQ_RPT; x < sj; x++)                  // long sub-vectors: the rest straight from memory
        sl[x * 256 + tid] = tid < k ? pq_cents[(size_t)k * fr + (size_t)tid * sj + x] : 0.f;
      if (j + GQ_PD < m_pad) fetch(j + GQ_PD, pre[p]);
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
  if (!live) continue;
  const int row_from = bounds[c], row_until = bounds[c + 1];
  // (BIG: the heaps sit behind the tables and the codebook slice)
  float *bigv = gq_lds + (size_t)GQ_WAVES * (m_pad * 256 + d) + slice_floats + (size_t)wave * (BIG ? K : 0);
  int *bigk = reinterpret_cast<int *>(gq_lds + (size_t)GQ_WAVES * (m_pad * 256 + d) + slice_floats + (size_t)GQ_WAVES * (BIG ? K : 0)) +
              (size_t)wave * (BIG ? K : 0);
  typename std::conditional<BIG, LdsHeap, RegHeap>::type h = [&] {
    if constexpr (BIG) return LdsHeap(bigv, bigk, K, lane);
    else return RegHeap(K, lane);
  }();
  const Word *cw = reinterpret_cast<const Word *>(codes);
  // the first code words of the next GQ_PD row blocks stay in flight
  const int rb_first = row_from / 64, rb_end = (row_until + 63) / 64;
  Word wq[GQ_PD];
#pragma unroll
  for (int p = 0; p < GQ_PD; p++) wq[p] = rb_first + p < rb_end ? cw[((size_t)(rb_first + p) * ng) * 64 + lane] : Word{};
  for (int rb0 = rb_first; rb0 < rb_end; rb0 += GQ_PD) {
#pragma unroll
  for (int p = 0; p < GQ_PD; p++) {
    const int rb = rb0 + p;
    if (rb >= rb_end) break;
    float acc = 0.f;                 // PQIndex.distances: j ascending, unfused fp32
    const Word w0 = wq[p];
    if (rb + GQ_PD < rb_end) wq[p] = cw[((size_t)(rb + GQ_PD) * ng) * 64 + lane];
    for (int gi = 0; gi < ng; gi++) {
      const Word w = gi == 0 ? w0 : cw[((size_t)rb * ng + gi) * 64 + lane];
      const float *tj = gtab + gi * VEC * 256;
#pragma unroll
      for (int b = 0; b < VEC; b++) acc += tj[b * 256 + code_byte<VEC>(w, b)];
    }
    const int row = rb * 64 + lane;
    const bool valid = row >= row_from && row < row_until;
    // rows in ascending order through heap.update; the ballot only skips rows the heap would
    // reject anyway (full and root <= value -- NaN compares false and is rejected like there)
    unsigned long long mk = __ballot(valid && (h.size < K || h.val(0) > acc));
    while (mk) {
      const int l = __ffsll((long long)mk) - 1;
      mk &= mk - 1;
      const float x = readlane_f(acc, l);
      if (h.would_insert(x)) h.update(rb * 64 + l, x);
    }
  }
  }
  const size_t o = ((size_t)q * stride + t) * K;
  if constexpr (BIG) {
    for (int i = lane; i < h.size; i += 64) { hk[o + i] = h.key(i); hv[o + i] = h.val(i); }
  } else {
    if (lane < h.size) { hk[o + lane] = h.k; hv[o + lane] = h.v; }
  }
  if (lane == 0) hs[(size_t)q * stride + t] = h.size;
  }
}

// ---- one searched group of one query over 16-bit codes (k > 256: Coder.BytePlus, wide.hip) ----------------
// The residual's table is m * k floats (64 KiB at k = 1024, 4 MiB at k = 65 536): it is built in a slot of
// global scratch (one slot per workgroup, which walks the (query, group) pairs), and the group's rows go through
// the LITERAL TopKHeap in row order -- the same heaps, stored in array order, as gq_group_scan's, so
// that gq_merge folds them exactly as GroupedIndex.query does (Index.scala:265-282).  Generality over speed.
// BIG (k_nn > 63): the pair's heap is an LdsHeap behind the residual (K values, then K keys), stored in the same
// array order at stride K and folded by gq_merge<true>.
template <bool BIG>
__global__ __launch_bounds__(64) void gq_group_scan_wide(const uint16_t *__restrict__ wcodes, int m, int k, int d,
                                                         const float *__restrict__ pq_cents,
                                                         const int *__restrict__ from, const int *__restrict__ sdim,
                                                         const float *__restrict__ gcent, const int *__restrict__ bounds,
                                                         const float *__restrict__ Q, const int *__restrict__ nn,
                                                         int nn_stride, const int *__restrict__ nn_cnt, int stride, int B,
                                                         int K, float *__restrict__ scratch /*[gridDim.x][m][k]*/,
                                                         int *__restrict__ hk, float *__restrict__ hv, int *__restrict__ hs) {
  extern __shared__ float gw_res[];   // d (BIG: then K heap values and K heap keys)
  const int lane = threadIdx.x;
  float *T = scratch + (size_t)blockIdx.x * m * k;
  const long long pairs = (long long)B * stride;
  for (long long pr = blockIdx.x; pr < pairs; pr += gridDim.x) {
    const int q = (int)(pr / stride), t = (int)(pr - (long long)q * stride);
    if (t >= nn_cnt[q]) continue;
    const int c = nn[(size_t)q * nn_stride + t];
    for (int e = lane; e < d; e += 64) gw_res[e] = Q[(size_t)q * d + e] - gcent[(size_t)c * d + e];   // MathUtils.subtract
    // Index.prepareQuery on the residual (Index.scala:352-383): e ascending, unfused
    for (int j = 0; j < m; j++) {
      const int fr = from[j], sj = sdim[j];
      for (int cc = lane; cc < k; cc += 64) {
        const float *cent = pq_cents + (size_t)k * fr + (size_t)cc * sj;
        float acc = 0.f;
        for (int x = 0; x < sj; x++) {
          const float dd = gw_res[fr + x] - cent[x];
          acc += dd * dd;
        }
        T[(size_t)j * k + cc] = acc;
      }
    }
    __threadfence();   // the table is read back by other lanes through the vector L1
    const int row_from = bounds[c], row_until = bounds[c + 1];
    typename std::conditional<BIG, LdsHeap, RegHeap>::type h = [&] {
      if constexpr (BIG) return LdsHeap(gw_res + d, reinterpret_cast<int *>(gw_res + d + K), K, lane);
      else return RegHeap(K, lane);
    }();
    for (int rb = row_from / 64; rb < (row_until + 63) / 64; rb++) {
      const uint16_t *p = wcodes + (size_t)rb * m * 64 + lane;
      float acc = 0.f;                 // PQIndex.distances: j ascending, unfused fp32
      for (int j = 0; j < m; j++) acc += T[(size_t)j * k + p[(size_t)j * 64]];
      const int row = rb * 64 + lane;
      const bool valid = row >= row_from && row < row_until;
      unsigned long long mk = __ballot(valid && (h.size < K || h.val(0) > acc));
      while (mk) {
        const int l = __ffsll((long long)mk) - 1;
        mk &= mk - 1;
        const float x = readlane_f(acc, l);
        if (h.would_insert(x)) h.update(rb * 64 + l, x);
      }
    }
    const size_t o = ((size_t)q * stride + t) * K;
    if constexpr (BIG) {
      for (int i = lane; i < h.size; i += 64) { hk[o + i] = h.key(i); hv[o + i] = h.val(i); }
    } else {
      if (lane < h.size) { hk[o + lane] = h.k; hv[o + lane] = h.v; }
    }
    if (lane == 0) hs[(size_t)q * stride + t] = h.size;
    __threadfence();   // the next pair overwrites the table slot
  }
}

// ---- approximate pre-selection + exact re-ranking -------------------------------------------------------
// The reference scores a row of a searched group through the residual's own table: one m x 256 table per (query,
// group) pair -- 512 K tables of 98 Kflop per 1024-query batch at 10 M rows / LimitGroups(500), more work than
// the scan they serve (8.4 ms per batch in round 1, against 3 ms for the flat index scanning 20 times the rows).
// But the distance it computes is  |q - (g + r^_i)|^2  with  r^_i = decode(codes_i),  and
//     |q - x^_i|^2 = |q|^2 - 2 q.g - 2 sum_j q_j . c_j[code_ij] + |x^_i|^2 ,      x^_i = g + r^_i ,
// needs ONE table per QUERY (P[j][c] = -2 q_j . c_j[c], 16 KiB, shared by all its groups), one dot product per
// (query, group) and one precomputed number per row.  That value D~ is not the reference's arithmetic, so it only
// SELECTS: every query keeps the 64 rows with the smallest D~ of its searched groups (gq_approx_scan), those are
// re-scored with the reference's arithmetic (gq_rerank: MathUtils.subtract, Index.prepareQuery's and
// PQIndex.distances' summation order, bit for bit) and ordered by (distance, row); the answer is certified when
// the (K+1)-th exact distance lies below the 64th D~ minus an error margin that bounds |D~ - exact| -- then no
// row outside the 64 can reach the K+1 best.  Uncertified queries, queries with equal distances among their K+1
// best and queries that saw a NaN go to the literal kernels as before, so results stay the reference's.
__global__ void gq_row_norms(const uint8_t *__restrict__ codes, int ng, int vec, int m, int k, int d,
                             const float *__restrict__ pq_cents, const int *__restrict__ from, const int *__restrict__ sdim,
                             const float *__restrict__ gcent, const int *__restrict__ bounds, int g, int n,
                             float *__restrict__ xnorm, unsigned *__restrict__ xnmax_bits) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int lo = 0, hi = g;                       // group of row i: largest c with bounds[c] <= i (empty groups skipped)
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (bounds[mid] <= i) lo = mid; else hi = mid; }
  const float *gc = gcent + (size_t)lo * d;
  float acc = 0.f;
  for (int j = 0; j < m; j++) {
    const int code = codes[(((size_t)(i >> 6) * ng + j / vec) * 64 + (i & 63)) * vec + j % vec];
    const int fr = from[j], sj = sdim[j];
    const float *c = pq_cents + (size_t)k * fr + (size_t)code * sj;
    for (int t = 0; t < sj; t++) { const float v = gc[fr + t] + c[t]; acc += v * v; }
  }
  xnorm[i] = acc;
  atomicMax(xnmax_bits, __float_as_uint(acc == acc && acc < INFINITY ? acc : INFINITY));
}

// P[q][j][c] = -2 * (q_j . c_j[c]); entries beyond k (and padding quantizers) are 0
__global__ __launch_bounds__(256) void gq_ptables(const float *__restrict__ pq_cents, const int *__restrict__ from,
                                                  const int *__restrict__ sdim, int d, int m, int m_pad, int k,
                                                  const float *__restrict__ Q, float *__restrict__ P) {
  const int c = threadIdx.x, j = blockIdx.x, q = blockIdx.y;
  float acc = 0.f;
  if (j < m && c < k) acc = ptable_entry(Q, (size_t)q * d, pq_cents, from, sdim, k, j, c);
  P[((size_t)q * m_pad + j) * 256 + c] = acc;
}

constexpr int GA_WAVES = 16;    // waves of one query's workgroup: each takes every 16th searched group
constexpr int GA_C = 64;        // candidates kept per query
static_assert(GF_WAVES == GA_WAVES && GF_LIST == GA_C, "gf_survivors writes gq_approx_scan's lists");
template <int VEC>
__global__ __launch_bounds__(64 * GA_WAVES) void gq_approx_scan(const uint8_t *__restrict__ codes, int ng, int m_pad, int d,
                                                                const float *__restrict__ P, const float *__restrict__ xnorm,
                                                                const float *__restrict__ gcent,
                                                                const int *__restrict__ bounds, const float *__restrict__ Q,
                                                                const int *__restrict__ nn, int nn_stride,
                                                                const int *__restrict__ nn_cnt, float *__restrict__ lv,
                                                                int *__restrict__ li, int *__restrict__ nanflag) {
  using Word = typename CodeWord<VEC>::type;
  extern __shared__ float ga_lds[];           // m_pad * 256 table entries, then d query coordinates
  float *tab = ga_lds, *qv = ga_lds + m_pad * 256;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = blockIdx.x;
  for (int e = tid; e < m_pad * 256; e += 64 * GA_WAVES) tab[e] = P[(size_t)q * m_pad * 256 + e];
  for (int e = tid; e < d; e += 64 * GA_WAVES) qv[e] = Q[(size_t)q * d + e];
  __syncthreads();
  float qq = 0.f;
  for (int e = lane; e < d; e += 64) qq += qv[e] * qv[e];
  qq = wave_sum(qq);
  WaveList wl;
  wl.init();
  int cnt = 0, saw_nan = 0;
  const int ngroups = nn_cnt[q];
  const Word *cw = reinterpret_cast<const Word *>(codes);
  for (int t = wave; t < ngroups; t += GA_WAVES) {
    const int c = nn[(size_t)q * nn_stride + t];
    const int row_from = bounds[c], row_until = bounds[c + 1];
    float qg = 0.f;
    for (int e = lane; e < d; e += 64) qg += qv[e] * gcent[(size_t)c * d + e];
    qg = wave_sum(qg);
    const float base = qq - 2.0f * qg;
    const int rb_first = row_from >> 6, rb_end = (row_until + 63) >> 6;
    Word wnext{};
    if (rb_first < rb_end) wnext = cw[((size_t)rb_first * ng) * 64 + lane];
    for (int rb = rb_first; rb < rb_end; rb++) {
      const Word w0 = wnext;
      if (rb + 1 < rb_end) wnext = cw[((size_t)(rb + 1) * ng) * 64 + lane];
      const int row = rb * 64 + lane;
      const bool valid = row >= row_from && row < row_until;
      const float acc = approx_row_sum<VEC>(base + (valid ? xnorm[row] : 0.f), tab, ng, [=](int gi) {
        return gi == 0 ? w0 : cw[((size_t)rb * ng + gi) * 64 + lane];
      });
      if (__ballot(valid && acc != acc) != 0ull) saw_nan = 1;
      unsigned long long mk = __ballot(valid && (cnt < GA_C || wl.accepts(acc, row)));
      while (mk) {
        const int l = __ffsll((long long)mk) - 1;
        mk &= mk - 1;
        const float x = readlane_f(acc, l);
        const int r = rb * 64 + l;
        if (cnt < GA_C || wl.accepts(x, r)) {
          wl.insert(x, r, GA_C, lane);
          if (cnt < GA_C) cnt++;
        }
      }
    }
  }
  const size_t o = ((size_t)q * GA_WAVES + wave) * GA_C;
  lv[o + lane] = wl.v;
  li[o + lane] = wl.i;
  if (lane == 0) nanflag[q * GA_WAVES + wave] = saw_nan;
}

// 64-lane bitonic sort of (value, id) pairs, ascending by (value, id); padding = (+inf, INT_MAX).  (select.hpp's network
// with a step for pairs compiles gq_rerank to other code than this loop does: it keeps its own.)
__device__ inline void sort64_pairs(float &v, int &id, int lane) {
#pragma unroll
  for (int k = 2; k <= 64; k <<= 1)
#pragma unroll
    for (int j = k >> 1; j >= 1; j >>= 1) {
      const float ov = __shfl_xor(v, j);
      const int oi = __shfl_xor(id, j);
      const bool up = (lane & k) == 0, lower = (lane & j) == 0;
      const bool other_less = ov < v || (ov == v && oi < id);
      const bool take = (lower == up) ? other_less : !other_less && !(ov == v && oi == id);
      if (take) { v = ov; id = oi; }
    }
}

// exact re-scoring of one query's candidates (lane = candidate) + certificate; see the block comment above
__global__ __launch_bounds__(64) void gq_rerank(const uint8_t *__restrict__ codes, int ng, int vec, int m, int k, int d,
                                                const float *__restrict__ pq_cents, const int *__restrict__ from,
                                                const int *__restrict__ sdim, const float *__restrict__ gcent,
                                                const int *__restrict__ bounds, int g, const float *__restrict__ Q,
                                                const float *__restrict__ cv, const int *__restrict__ ci,
                                                const int *__restrict__ nanflag, float xnmax, int K,
                                                int *__restrict__ out_idx, float *__restrict__ out_dist,
                                                int *__restrict__ out_count, int *__restrict__ qlist,
                                                int *__restrict__ qcount) {
  const int q = blockIdx.x, lane = threadIdx.x;
  const float approx = cv[(size_t)q * GA_C + lane];
  const int row = ci[(size_t)q * GA_C + lane];
  const bool have = row != INT_MAX;
  const int ncand = __popcll(__ballot(have));
  const float a_last = readlane_f(approx, GA_C - 1);          // the largest kept D~ (every other row's is >= it)
  float qq = 0.f;
  for (int e = lane; e < d; e += 64) { const float x = Q[(size_t)q * d + e]; qq += x * x; }
  qq = wave_sum(qq);
  float D = INFINITY;
  if (have) {
    int lo = 0, hi = g;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (bounds[mid] <= row) lo = mid; else hi = mid; }
    const float *gc = gcent + (size_t)lo * d;
    const float *qp = Q + (size_t)q * d;
    D = 0.f;                                                  // PQIndex.distances: 0 + T[0] + T[1] + ... (unfused fp32)
    for (int j = 0; j < m; j++) {
      const int code = codes[(((size_t)(row >> 6) * ng + j / vec) * 64 + (row & 63)) * vec + j % vec];
      const int fr = from[j], sj = sdim[j];
      const float *c = pq_cents + (size_t)k * fr + (size_t)code * sj;
      float tj = 0.f;                                         // Index.prepareQuery on the residual (MathUtils.subtract)
      for (int t = 0; t < sj; t++) { const float dd = (qp[fr + t] - gc[fr + t]) - c[t]; tj += dd * dd; }
      D += tj;
    }
  }
  const bool nan_d = __ballot(have && D != D) != 0ull;
  float sv = have && D == D ? D : INFINITY;
  int si = have && D == D ? row : INT_MAX;
  sort64_pairs(sv, si, lane);
  const int nfin = __popcll(__ballot(si != INT_MAX));
  const int live = min(K, nfin);
  if (lane < K) {
    out_idx[(size_t)q * K + lane] = lane < live ? si : -1;
    out_dist[(size_t)q * K + lane] = lane < live ? sv : INFINITY;
  }
  const float nv = __shfl_down(sv, 1);
  const int ni = __shfl_down(si, 1);
  const bool tie = lane < K && si != INT_MAX && ni != INT_MAX && sv == nv;      // equal neighbours among the K+1 best
  // |D~ - exact| <= margin: both are sums of ~d + m terms of magnitude <= (|q| + |x^|)^2
  const float xm = __fsqrt_rn(qq) + __fsqrt_rn(xnmax);
  const float margin = 4.0f * (float)(d + 2 * m + 16) * 5.9604645e-8f * xm * xm;
  bool certified = true;
  if (ncand == GA_C) {                                        // rows were left out: the K+1 best must clear their bound
    const float ek = readlane_f(sv, min(K, GA_C - 1));        // (K+1)-th exact distance (K <= 63)
    certified = nfin > K && ek < a_last - margin && margin == margin && a_last == a_last;
  }
  int nanany = lane < GA_WAVES ? nanflag[q * GA_WAVES + lane] : 0;
  const bool redo = !certified || nan_d || __ballot(tie) != 0ull || __ballot(nanany != 0) != 0ull;
  if (lane == 0) {
    if (out_count) out_count[q] = live;
    if (redo) qlist[atomicAdd(qcount, 1)] = q;
  }
}

// ---- TopKHeap.merge of the group heaps in search order, Result.fromHeap ---------------------------
template <bool BIG>
__global__ __launch_bounds__(64) void gq_merge(const int *__restrict__ hk, const float *__restrict__ hv,
                                               const int *__restrict__ hs, const int *__restrict__ nn_cnt, int stride,
                                               int K, int *__restrict__ out_idx, float *__restrict__ out_dist,
                                               int *__restrict__ out_count, const int *__restrict__ qlist,
                                               const int *__restrict__ qcount) {
  extern __shared__ float gm_lds[];            // BIG: K values, then K keys
  const int lane = threadIdx.x;
  const int nq = qlist ? *qcount : (int)gridDim.x;
  for (int fx = blockIdx.x; fx < nq; fx += gridDim.x) {
  const int q = qlist ? qlist[fx] : fx;
  typename std::conditional<BIG, LdsHeap, RegHeap>::type h = [&] {
    if constexpr (BIG) return LdsHeap(gm_lds, reinterpret_cast<int *>(gm_lds + K), K, lane);
    else return RegHeap(K, lane);
  }();
  const int cnt = nn_cnt[q];
  for (int t = 0; t < cnt; t++) {
    const size_t o = ((size_t)q * stride + t) * K;
    const int sz = hs[(size_t)q * stride + t];
    if constexpr (BIG) {
      for (int i = 0; i < sz; i++) h.update(hk[o + i], hv[o + i]);                    // array order
    } else {
      const int kk = lane < sz ? hk[o + lane] : 0;
      const float vv = lane < sz ? hv[o + lane] : 0.f;
      for (int i = 0; i < sz; i++) h.update(readlane_i(kk, i), readlane_f(vv, i));   // array order
    }
  }
  const int live = h.size;
  h.drain([&](int i, int tk, float tv) {                    // Result.fromHeap
    if (lane == 0) { out_idx[(size_t)q * K + i] = tk; out_dist[(size_t)q * K + i] = tv; }
  });
  for (int i = live + lane; i < K; i += 64) { out_idx[(size_t)q * K + i] = -1; out_dist[(size_t)q * K + i] = INFINITY; }
  if (lane == 0 && out_count) out_count[q] = live;
  }
}

// residual dataset in grouped order: out[i] = X[perm[i]] - gcent[group_of[i]]
__global__ void gq_residuals(const float *__restrict__ X, int d, const int *__restrict__ perm,
                             const int *__restrict__ group_of, const float *__restrict__ gcent, long long total,
                             float *__restrict__ out) {
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (long long)gridDim.x * blockDim.x) {
    const long long i = t / d;
    const int e = (int)(t - i * d);
    out[t] = X[(size_t)perm[i] * d + e] - gcent[(size_t)group_of[i] * d + e];
  }
}

// ---- the query driver: run_grouped_query and its stages ---------------------------------------------
// The environment, read once per call (the tests set the variables after the library is loaded).
struct GroupedKnobs {
  bool literal = getenv("GULON_GROUPED_LITERAL") != nullptr;   // every query through the literal heaps: a testing aid
  bool stats = getenv("GULON_GROUPED_STATS") != nullptr;       // synchronous statistics to stderr: a debugging aid
};

struct GroupedCall {   // one batch: the arguments of run_grouped_query
  gulon_grouped_index *gx;
  const float *dQ;
  int B, K, strategy, limit;
  int *d_oi;
  float *d_od;
  int *d_oc;
  hipStream_t st;
  bool big_k() const { return K > GULON_MAX_K; }   // the heaps in LDS (LdsHeap) instead of a wavefront's registers
};

struct CoarseResult {
  int nn_stride;   // groups searched per query at most: the row length of nn
  int stride;      // per-group heaps per query (<= nn_stride)
  int lit_cap;     // > 0: group selection went through the (distance, id) sorts and the order-only ties (level 1) are
                   // still to be redone for the listed queries; capacity of the literal heap
};

void launch_literal_groups(const GroupedCall &c, int nn_stride, int cap, int level, int grid, const int *qlist,
                           const int *qcount) {
  gulon_grouped_index *gx = c.gx;
  hipLaunchKernelGGL(gq_literal_groups, dim3(grid), dim3(64), (size_t)cap * 8, c.st, gx->cdist.p, gx->g, cap, gx->bounds.p,
                     c.strategy == 1, c.limit, gx->lit_flag.p, level, qlist, qcount, gx->nn.p, nn_stride, gx->nn_cnt.p);
}

// searchSpace (Index.scala:284-299): the groups every query searches, in gx->nn / gx->nn_cnt.
// all_literal: every query's result will come from the literal heaps, merged in search order.
CoarseResult coarse_stage(const GroupedCall &c, bool all_literal) {
  gulon_grouped_index *gx = c.gx;
  const int g = gx->g, B = c.B, strategy = c.strategy, limit = c.limit;
  hipStream_t st = c.st;
  // groups searched per query: at most `nn_stride` (LimitVectors: every non-empty group holds >= 1 row; the
  // reference's leading empty group adds nothing to the count and is searched on top)
  CoarseResult r;
  r.nn_stride = std::max(1, (int)std::min<long long>((long long)limit + (strategy == 1 ? gx->n_empty : 0), g));
  r.stride = r.nn_stride;
  r.lit_cap = 0;
  gx->cdist.ensure((size_t)B * g);
  gx->nn.ensure((size_t)B * r.nn_stride);
  gx->nn_cnt.ensure((size_t)B);
  hipLaunchKernelGGL(gq_cdist, dim3(ceil_div(g, 256), ceil_div(B, CD_Q)), dim3(256), 0, st, gx->gcent_t.p, g, gx->d, c.dQ, B,
                     gx->cdist.p);
  if (strategy == 0 && limit <= GULON_MAX_K && limit >= 1) {
    hipLaunchKernelGGL(gq_nearest_groups, dim3(B), dim3(64), 0, st, gx->cdist.p, g, limit, gx->nn.p, r.nn_stride,
                       gx->nn_cnt.p);
    HIP_CHECK(hipGetLastError());
    return r;
  }
  int n2 = 64;
  while (n2 < g) n2 <<= 1;
  const size_t lds = (size_t)n2 * 8;
  GULON_UNSUPPORTED(lds > 144 * 1024, "%d groups: ordering all of them needs %zu B of LDS (> 144 KiB)", g, lds);
  HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(gq_sorted_groups),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const int *done = nullptr;
  gx->lit_flag.ensure((size_t)B);
  if (strategy == 0 && limit >= 1 && limit * 4 <= g) {
    // few of many: radix-select + sort of the selected; the full sort only runs for queries it gave up on
    int cap = 256;
    while (cap < limit + 128) cap <<= 1;
    gx->sel_ok.ensure((size_t)B);
    const size_t sel_lds = (size_t)cap * 8;
    auto kern = g <= 256 * 8 ? gq_select_groups<8> : g <= 256 * 40 ? gq_select_groups<40> : gq_select_groups<0>;
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sel_lds));
    hipLaunchKernelGGL(kern, dim3(B), dim3(256), sel_lds, st, gx->cdist.p, g, limit, cap, gx->nn.p,
                       r.nn_stride, gx->nn_cnt.p, gx->sel_ok.p, gx->lit_flag.p);
    done = gx->sel_ok.p;
  }
  hipLaunchKernelGGL(gq_sorted_groups, dim3(B), dim3(256), lds, st, gx->cdist.p, g, n2, gx->bounds.p, strategy == 1,
                     limit, gx->nn.p, r.nn_stride, gx->nn_cnt.p, done, gx->lit_flag.p);
  // queries whose answer hangs on equally distant centroids (or NaN distances): the reference's heap, literally
  const int hcap = strategy == 1 ? g : std::min(limit, g);
  if (hcap >= 1) {
    const size_t hl = (size_t)hcap * 8;
    GULON_UNSUPPORTED(hl > 144 * 1024, "%d groups: the literal heap needs %zu B of LDS (> 144 KiB)", hcap, hl);
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(gq_literal_groups),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)hl));
    launch_literal_groups(c, r.nn_stride, hcap, 2, B, nullptr, nullptr);
    if (all_literal) launch_literal_groups(c, r.nn_stride, hcap, 1, B, nullptr, nullptr);   // the order-only ties as well
    else r.lit_cap = hcap;
  }
  if (strategy == 1 && r.nn_stride > 64) {
    // LimitVectors rarely needs more than a handful of groups: size the per-group heaps by the
    // largest count of this batch (one small read-back) instead of by the worst case
    std::vector<int> h((size_t)B);
    HIP_CHECK(hipMemcpyAsync(h.data(), gx->nn_cnt.p, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    int mx = 1;
    for (int v : h) mx = std::max(mx, v);
    r.stride = mx;
  }
  HIP_CHECK(hipGetLastError());
  return r;
}

void ensure_group_heaps(const GroupedCall &c, int stride) {
  gulon_grouped_index *gx = c.gx;
  gx->hk.ensure((size_t)c.B * stride * c.K);
  gx->hv.ensure((size_t)c.B * stride * c.K);
  gx->hs.ensure((size_t)c.B * stride);
}

// TopKHeap.merge of the stored group heaps + Result.fromHeap: of every query (grid = B), or of the listed ones
void launch_gq_merge(const GroupedCall &c, int stride, int grid, const int *qlist, const int *qcount) {
  gulon_grouped_index *gx = c.gx;
  if (c.big_k())
    hipLaunchKernelGGL(gq_merge<true>, dim3(grid), dim3(64), sizeof(float) * 2 * (size_t)c.K, c.st, gx->hk.p, gx->hv.p,
                       gx->hs.p, gx->nn_cnt.p, stride, c.K, c.d_oi, c.d_od, c.d_oc, qlist, qcount);
  else
    hipLaunchKernelGGL(gq_merge<false>, dim3(grid), dim3(64), 0, c.st, gx->hk.p, gx->hv.p, gx->hs.p, gx->nn_cnt.p, stride,
                       c.K, c.d_oi, c.d_od, c.d_oc, qlist, qcount);
  HIP_CHECK(hipGetLastError());
}

// 16-bit codes: the literal heaps for every (query, group) pair, residual tables in global scratch (<= 1 GiB)
void wide_scan(const GroupedCall &c, const CoarseResult &co) {
  gulon_grouped_index *gx = c.gx;
  gulon_index *ix = gx->pq;
  const int B = c.B, K = c.K, stride = co.stride;
  hipStream_t st = c.st;
  ensure_group_heaps(c, stride);
  const size_t slot = (size_t)ix->m * ix->k * sizeof(float);
  const long long pairs = (long long)B * stride;
  const int blocks = (int)std::max<long long>(1, std::min<long long>(std::min<long long>(pairs, 4096),
                                                                    std::max<long long>(64, (1ll << 30) / (long long)slot)));
  gx->wide_tables.ensure((size_t)blocks * ix->m * ix->k);
  HIP_CHECK(hipMemsetAsync(gx->hs.p, 0, sizeof(int) * (size_t)B * stride, st));
  size_t lds = sizeof(float) * (size_t)ix->d;
  auto kern = gq_group_scan_wide<false>;
  if (c.big_k()) {   // the heaps in LDS (2 K words behind the residual), folded by the LDS merge
    lds += sizeof(float) * 2 * (size_t)K;
    GULON_UNSUPPORTED(lds > 160 * 1024, "grouped query needs %zu B of LDS (d = %d, k_nn = %d)", lds, ix->d, K);
    kern = gq_group_scan_wide<true>;
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  }
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(64), lds, st, ix->wcodes.p, ix->m, ix->k, ix->d, ix->cents.p, ix->from.p,
                     ix->sdim.p, gx->gcent.p, gx->bounds.p, c.dQ, gx->nn.p, co.nn_stride, gx->nn_cnt.p, stride, B, K,
                     gx->wide_tables.p, gx->hk.p, gx->hv.p, gx->hs.p);
  launch_gq_merge(c, stride, B, nullptr, nullptr);
}

struct GroupScanLds { size_t bytes; int slice_floats; };

// gq_group_scan's LDS: the four pairs' tables and residuals, one codebook slice, and for k_nn > 63 the four heaps
GroupScanLds group_scan_lds(const GroupedCall &c) {
  const gulon_index *ix = c.gx->pq;
  int smax = 1;
  std::vector<int> fr, un;
  subvectors(ix->d, ix->m, fr, un);
  for (int j = 0; j < ix->m; j++) smax = std::max(smax, un[j] - fr[j]);
  GroupScanLds l;
  l.slice_floats = 256 * smax;               // [x][256], transposed
  l.bytes = ((size_t)GQ_WAVES * (ix->m_pad * 256 + ix->d) + (size_t)l.slice_floats + (c.big_k() ? (size_t)GQ_WAVES * 2 * c.K : 0)) *
            sizeof(float);
  GULON_UNSUPPORTED(l.bytes > 160 * 1024, "grouped query needs %zu B of LDS (m = %d, d = %d, k_nn = %d)", l.bytes, ix->m, ix->d,
                    c.K);
  return l;
}

// the literal heap of every (query, searched group) pair: of `gy` rows of queries, or of the listed queries
void launch_group_scan(const GroupedCall &c, const CoarseResult &co, const GroupScanLds &l, int gy, const int *qlist,
                       const int *qcount) {
  gulon_grouped_index *gx = c.gx;
  gulon_index *ix = gx->pq;
  auto kern = c.big_k() ? (ix->vec == 16 ? gq_group_scan<16, true> : gq_group_scan<4, true>)
                        : (ix->vec == 16 ? gq_group_scan<16> : gq_group_scan<4>);
  HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)l.bytes));
  hipLaunchKernelGGL(kern, dim3(ceil_div(co.stride, GQ_WAVES), gy), dim3(64 * GQ_WAVES), l.bytes, c.st, ix->codes.p, ix->ng, ix->m,
                     ix->m_pad, ix->k, ix->d, ix->cents.p, ix->from.p, ix->sdim.p, gx->gcent.p, gx->bounds.p, c.dQ, gx->nn.p,
                     co.nn_stride, gx->nn_cnt.p, co.stride, c.K, gx->hk.p, gx->hv.p, gx->hs.p, qlist, qcount, l.slice_floats);
  HIP_CHECK(hipGetLastError());
}

// The queries gq_rerank listed, through the literal kernels: first the reference's heap order for those whose group
// ORDER hangs on equal centroid distances, then the group heaps and their merge (usually the list is empty)
void redo_flagged(const GroupedCall &c, const CoarseResult &co, const GroupScanLds &l) {
  gulon_grouped_index *gx = c.gx;
  const int fy = std::min(c.B, 16);
  if (co.lit_cap > 0) {
    launch_literal_groups(c, co.nn_stride, co.lit_cap, 1, fy, gx->qlist.p, gx->qcount.p);
    HIP_CHECK(hipGetLastError());
  }
  launch_group_scan(c, co, l, fy, gx->qlist.p, gx->qcount.p);
  launch_gq_merge(c, co.stride, fy, gx->qlist.p, gx->qcount.p);
}

void print_redo_stats(const GroupedCall &c) {   // GULON_GROUPED_STATS
  HIP_CHECK(hipStreamSynchronize(c.st));
  int nfl = 0;
  HIP_CHECK(hipMemcpy(&nfl, c.gx->qcount.p, sizeof(int), hipMemcpyDeviceToHost));
  fprintf(stderr, "[grouped] approximate pre-selection: %d of %d queries redone with literal heaps\n", nfl, c.B);
}

// by group with 8-bit bound tables (grouped_filter.hip) where a query searches more than a handful of groups; else
// every searched row through gq_approx_scan
bool by_group_applies(const GroupedCall &c, const CoarseResult &co) {
  gulon_grouped_index *gx = c.gx;
  gulon_index *ix = gx->pq;
  return gx->gfilter.built && group_filter_applies(ix->m, ix->m_pad, ix->ng, ix->vec, ix->k, ix->d) &&
         co.nn_stride > GF_SAMPLE_GROUPS && c.B <= 65535 &&          // (a grid's y extent carries the query)
         (long long)c.B * co.nn_stride <= (1ll << 28) &&             // (the pairs' tiles)
         (long long)c.B * gx->g <= (1ll << 27);                      // (the groups' query lists, room for all: 512 MiB at most)
}

// The pre-selection alone: per query the GA_C smallest (D~, row) of its searched rows in gx->amv / gx->ami, the flags in
// gx->anan and the queries' tables in gx->ptab -- by group, or every searched row through gq_approx_scan
void preselect(const GroupedCall &c, const CoarseResult &co, bool by_group) {
  gulon_grouped_index *gx = c.gx;
  gulon_index *ix = gx->pq;
  const int g = gx->g, B = c.B, nn_stride = co.nn_stride;
  hipStream_t st = c.st;
  gx->ptab.ensure((size_t)B * ix->m_pad * 256);
  gx->apv.ensure((size_t)B * GA_WAVES * GA_C); gx->api.ensure((size_t)B * GA_WAVES * GA_C);
  gx->amv.ensure((size_t)B * GA_C); gx->ami.ensure((size_t)B * GA_C);
  gx->anan.ensure((size_t)B * GA_WAVES);
  if (by_group) {   // (this path builds the tables where it quantizes them)
    group_filter_run(gx->gfilter, ix->codes.p, ix->ng, ix->vec, ix->m, ix->m_pad, ix->k, ix->d, gx->ptab.p, ix->cents.p,
                     ix->from.p, ix->sdim.p, gx->xnorm.p, gx->xnmax,
                     gx->gcent.p, gx->bounds.p, g, c.dQ, gx->cdist.p, gx->nn.p, nn_stride, gx->nn_cnt.p, B, gx->amv.p, gx->ami.p,
                     gx->anan.p, st);
  } else {
    // the query's table and coordinates, (m_pad * 256 + d) floats: at most 40 KiB, since GQ_WAVES = 4 times as much
    // (and a codebook slice) passed group_scan_lds' check against 160 KiB
    const size_t lds_ga = ((size_t)ix->m_pad * 256 + ix->d) * sizeof(float);
    auto kern = ix->vec == 16 ? gq_approx_scan<16> : gq_approx_scan<4>;
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds_ga));
    hipLaunchKernelGGL(gq_ptables, dim3(ix->m_pad, B), dim3(256), 0, st, ix->cents.p, ix->from.p, ix->sdim.p, ix->d, ix->m,
                       ix->m_pad, ix->k, c.dQ, gx->ptab.p);
    hipLaunchKernelGGL(kern, dim3(B), dim3(64 * GA_WAVES), lds_ga, st, ix->codes.p, ix->ng, ix->m_pad, ix->d, gx->ptab.p,
                       gx->xnorm.p, gx->gcent.p, gx->bounds.p, c.dQ, gx->nn.p, nn_stride, gx->nn_cnt.p, gx->apv.p, gx->api.p,
                       gx->anan.p);
    launch_merge(gx->apv.p, gx->api.p, GA_WAVES, (long long)GA_C, (long long)GA_WAVES * GA_C, B, GA_C - 1,
                 QueryOut::partial_lists(gx->amv.p, gx->ami.p), st);
  }
}

// gq_rerank over the lists in gx->amv / gx->ami / gx->anan: answers in d_oi / d_od / d_oc, the queries to redo appended
// to gx->qlist / gx->qcount
void launch_rerank(const GroupedCall &c) {
  gulon_grouped_index *gx = c.gx;
  gulon_index *ix = gx->pq;
  hipLaunchKernelGGL(gq_rerank, dim3(c.B), dim3(64), 0, c.st, ix->codes.p, ix->ng, ix->vec, ix->m, ix->k, ix->d, ix->cents.p,
                     ix->from.p, ix->sdim.p, gx->gcent.p, gx->bounds.p, gx->g, c.dQ, gx->amv.p, gx->ami.p, gx->anan.p, gx->xnmax,
                     c.K, c.d_oi, c.d_od, c.d_oc, gx->qlist.p, gx->qcount.p);
  HIP_CHECK(hipGetLastError());
}

// approximate pre-selection with one table per query, exact re-ranking of 64 candidates, certificate: answers in
// d_oi / d_od / d_oc, the queries to redo in gx->qlist / gx->qcount
void approx_stage(const GroupedCall &c, const CoarseResult &co, const GroupedKnobs &knobs) {
  gulon_grouped_index *gx = c.gx;
  gx->qlist.ensure((size_t)c.B);
  gx->qcount.ensure(1);
  HIP_CHECK(hipMemsetAsync(gx->qcount.p, 0, sizeof(int), c.st));
  preselect(c, co, by_group_applies(c, co));
  launch_rerank(c);
  if (knobs.stats) print_redo_stats(c);
}

void run_grouped_query(gulon_grouped_index *gx, const float *dQ, int B, int K, int strategy, int limit, int *d_oi,
                       float *d_od, int *d_oc, hipStream_t st) {
  GULON_REQUIRE(B >= 0 && K >= 0, "k and batch size must be non-negative");
  GULON_REQUIRE(strategy == 0 || strategy == 1, "strategy must be 0 (LimitGroups) or 1 (LimitVectors)");
  GULON_REQUIRE(limit >= 0, "limit must be non-negative");
  // k_nn > GULON_MAX_K (Tests.scala asks for up to 1000): the literal kernels with the heaps in LDS, for every query
  constexpr int GROUPED_MAX_K_BIG = 2048;
  GULON_UNSUPPORTED(K > GROUPED_MAX_K_BIG, "k_nn = %d > %d is not supported by the grouped index", K, GROUPED_MAX_K_BIG);
  if (B == 0) return;
  const GroupedKnobs knobs{};
  const GroupedCall c{gx, dQ, B, K, strategy, limit, d_oi, d_od, d_oc, st};
  if (c.big_k()) {   // the per-group heaps are B x groups x k_nn entries: batches of queries that keep them under 2 GiB
    const long long per_query = (long long)std::max(1, std::min(strategy == 1 ? gx->g : limit, gx->g)) * K;
    const int sub = (int)std::max<long long>(1, std::min<long long>(B, (1ll << 28) / std::max<long long>(1, per_query)));
    if (sub < B) {
      for (int q0 = 0; q0 < B; q0 += sub) {
        const int nb = std::min(sub, B - q0);
        run_grouped_query(gx, dQ + (size_t)q0 * gx->d, nb, K, strategy, limit, d_oi + (size_t)q0 * K, d_od + (size_t)q0 * K,
                          d_oc ? d_oc + q0 : nullptr, st);
      }
      return;
    }
  }
  if (K == 0) {
    if (d_oc) HIP_CHECK(hipMemsetAsync(d_oc, 0, sizeof(int) * (size_t)B, st));
    return;
  }
  const bool wide = gx->pq->wide;
  // Row norms exist for every 8-bit index that has rows (gulon_grouped_index_create); one without rows takes the
  // literal kernels, which are the reference for any input
  const bool literal_only = c.big_k() || knobs.literal || gx->xnorm.n == 0;
  const CoarseResult co = coarse_stage(c, wide || literal_only);
  if (wide) {
    wide_scan(c, co);
    return;
  }
  ensure_group_heaps(c, co.stride);
  const GroupScanLds l = group_scan_lds(c);
  if (literal_only) {
    launch_group_scan(c, co, l, B, nullptr, nullptr);
    launch_gq_merge(c, co.stride, B, nullptr, nullptr);
    return;
  }
  // the pre-selection for every query, then the literal heaps for the ones it flagged
  approx_stage(c, co, knobs);
  redo_flagged(c, co, l);
}

// A query from host pointers, under idx->mu: `fill(st)` puts the b queries into idx->q_dev, then the query, the
// download of the answers and the synchronise.
template <class Fill>
void query_from_host(gulon_grouped_index *idx, int b, int k_nn, int strategy, int limit, int32_t *out_idx, float *out_dist,
                     int32_t *out_count, Fill fill) {
  const size_t bk = (size_t)b * (size_t)k_nn;
  idx->q_dev.ensure((size_t)b * idx->d + 1);
  idx->oi.ensure(bk + 1); idx->od.ensure(bk + 1); idx->oc.ensure((size_t)b + 1);
  hipStream_t st = nullptr;
  StreamOrder so(idx->pq, st);
  if (b > 0) fill(st);
  run_grouped_query(idx, idx->q_dev.p, b, k_nn, strategy, limit, idx->oi.p, idx->od.p, idx->oc.p, st);
  if (bk) { idx->oi.download(out_idx, bk, st); idx->od.download(out_dist, bk, st); }
  if (b > 0 && out_count) idx->oc.download(out_count, b, st);
  so.done();
  HIP_CHECK(hipStreamSynchronize(st));
}

}  // namespace
}  // namespace gulon

using namespace gulon;

GULON_API int32_t gulon_dataset_group_residuals(const gulon_dataset *ds, const int32_t *perm,
                                                const int32_t *group_of, const float *group_centroids, int32_t g,
                                                gulon_dataset **out) {
  return guarded([&] {
    GULON_REQUIRE(ds != nullptr && out != nullptr && (ds->n == 0 || (perm && group_of)) && group_centroids && g >= 1,
                  "bad arguments");
    *out = nullptr;
    const int n = ds->n, d = ds->d;
    for (int i = 0; i < n; i++) {
      GULON_REQUIRE(perm[i] >= 0 && perm[i] < n, "perm[%d] = %d out of range", i, perm[i]);
      GULON_REQUIRE(group_of[i] >= 0 && group_of[i] < g, "group_of[%d] = %d out of range", i, group_of[i]);
    }
    std::unique_ptr<gulon_dataset> r(new gulon_dataset());
    r->n = n; r->d = d;
    const long long total = (long long)n * d;
    r->x.alloc(std::max<size_t>((size_t)total, 1));
    if (total) {
      DevBuf<int> dp, dg;
      DevBuf<float> dc;
      dp.upload(perm, n); dg.upload(group_of, n); dc.upload(group_centroids, (size_t)g * d);
      hipLaunchKernelGGL(gq_residuals, dim3((unsigned)std::min<long long>(ceil_div(total, 256), 1 << 20)), dim3(256), 0,
                         0, ds->x.p, d, dp.p, dg.p, dc.p, total, r->x.p);
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipDeviceSynchronize());
    }
    *out = r.release();
  });
}

GULON_API int32_t gulon_grouped_index_create(const uint8_t *codes, int32_t n, int32_t d, int32_t m, int32_t k,
                                             const float *pq_cents, const float *group_centroids,
                                             const int32_t *offsets, int32_t g, gulon_grouped_index **out) {
  return guarded([&] {
    GULON_REQUIRE(out != nullptr, "out is null");
    *out = nullptr;
    GULON_REQUIRE(g >= 1 && group_centroids != nullptr && (g == 1 || offsets != nullptr), "bad grouping");
    // GroupedIndex asserts centroids.length == offsets.length + 1 (Index.scala:240-241); offsets ascend
    std::vector<int> bounds((size_t)g + 1);
    bounds[0] = 0;
    for (int c = 1; c < g; c++) {
      GULON_REQUIRE(offsets[c - 1] >= bounds[c - 1] && offsets[c - 1] <= n, "group offsets must ascend within [0, n]");
      bounds[c] = offsets[c - 1];
    }
    bounds[g] = n;
    std::unique_ptr<gulon_grouped_index> gx(new gulon_grouped_index());
    for (int c = 0; c < g; c++) gx->n_empty += bounds[c + 1] == bounds[c];
    gulon_index *pq = nullptr;
    int32_t rc = gulon_index_create(codes, n, d, m, k, pq_cents, 0, &pq);
    if (rc != GULON_OK) throw DeviceError{rc};
    gx->pq = pq;
    gx->n = n; gx->d = d; gx->g = g;
    gx->gcent.upload(group_centroids, (size_t)g * d);
    {
      std::vector<float> tr((size_t)g * d);
      for (int c = 0; c < g; c++)
        for (int e = 0; e < d; e++) tr[(size_t)e * g + c] = group_centroids[(size_t)c * d + e];
      gx->gcent_t.upload(tr.data(), tr.size());
      HIP_CHECK(hipDeviceSynchronize());   // tr goes out of scope
    }
    gx->bounds.upload(bounds.data(), bounds.size());
    HIP_CHECK(hipDeviceSynchronize());
    if (!pq->wide && n > 0) {   // |g + decode(codes_i)|^2 per row: the per-row term of the approximate pre-selection
      gx->xnorm.alloc((size_t)n);
      DevBuf<unsigned> mx(1);
      HIP_CHECK(hipMemset(mx.p, 0, sizeof(unsigned)));
      hipLaunchKernelGGL(gq_row_norms, dim3(ceil_div(n, 256)), dim3(256), 0, 0, pq->codes.p, pq->ng, pq->vec, pq->m, pq->k, d,
                         pq->cents.p, pq->from.p, pq->sdim.p, gx->gcent.p, gx->bounds.p, g, n, gx->xnorm.p, mx.p);
      HIP_CHECK(hipGetLastError());
      unsigned h = 0;
      HIP_CHECK(hipMemcpy(&h, mx.p, sizeof(h), hipMemcpyDeviceToHost));
      memcpy(&gx->xnmax, &h, sizeof(float));
      if (gx->xnmax < INFINITY && group_filter_applies(pq->m, pq->m_pad, pq->ng, pq->vec, pq->k, d))
        group_filter_build(gx->gfilter, gx->xnorm.p, n, gx->gcent.p, gx->bounds.p, g, d);
    }
    *out = gx.release();
  });
}

GULON_API int32_t gulon_grouped_index_destroy(gulon_grouped_index *idx) {
  return guarded([&] { delete idx; });
}

GULON_API int32_t gulon_grouped_index_batch_query_dev(gulon_grouped_index *idx, const float *d_queries, int32_t b,
                                                      int32_t k_nn, int32_t strategy, int32_t limit,
                                                      int32_t *d_out_idx, float *d_out_dist, int32_t *d_out_count,
                                                      void *stream) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    std::lock_guard<std::mutex> lock(idx->mu);
    StreamOrder so(idx->pq, (hipStream_t)stream);   // the scratch is the handle's: behind the last call's device work
    run_grouped_query(idx, d_queries, b, k_nn, strategy, limit, d_out_idx, d_out_dist, d_out_count,
                      (hipStream_t)stream);
    so.done();
  });
}

GULON_API int32_t gulon_grouped_index_batch_query(gulon_grouped_index *idx, const float *queries, int32_t b,
                                                  int32_t k_nn, int32_t strategy, int32_t limit, int32_t *out_idx,
                                                  float *out_dist, int32_t *out_count) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    GULON_REQUIRE(b >= 0 && k_nn >= 0, "k and batch size must be non-negative");
    std::lock_guard<std::mutex> lock(idx->mu);
    query_from_host(idx, b, k_nn, strategy, limit, out_idx, out_dist, out_count, [&](hipStream_t st) {
      HIP_CHECK(hipMemcpyAsync(idx->q_dev.p, queries, sizeof(float) * (size_t)b * idx->d, hipMemcpyHostToDevice, st));
    });
  });
}

// ---- GroupedIndex.lookup (Index.scala:247-253) on row ids: centroids(partition) + decode(row), the partition found as
// the reference finds it -- Arrays.binarySearch(offsets, row), then i < 0 ? -i - 1 : i + 1 -- on the RAW offsets
// (bounds[1..g-1]).  Where offsets repeat (empty groups) that can be another group than the row's own (clusterOf's
// searchsorted(side = right)); the reference adds that group's centroid, and so does this (decode.hip).
GULON_API int32_t gulon_grouped_index_lookup_rows(gulon_grouped_index *idx, const int32_t *rows, int32_t b,
                                                  int32_t normalize, float *out) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    std::lock_guard<std::mutex> lock(idx->mu);
    decode_rows_host(idx->pq, idx->rows_dev, idx->q_dev, rows, b, idx->gcent.p, idx->bounds.p + 1, idx->g - 1,
                     normalize != 0, out, nullptr);
  });
}

GULON_API int32_t gulon_grouped_index_lookup_rows_dev(gulon_grouped_index *idx, const int32_t *d_rows, int32_t b,
                                                      int32_t normalize, float *d_out, void *stream) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    std::lock_guard<std::mutex> lock(idx->mu);
    StreamOrder so(idx->pq, (hipStream_t)stream);
    ensure_row_err(idx->pq);
    launch_decode_rows(idx->pq, d_rows, b, idx->gcent.p, idx->bounds.p + 1, idx->g - 1, normalize != 0, d_out,
                       idx->pq->row_err.p, (hipStream_t)stream);
    so.done();
  });
}

// Index.queryByWord (Index.scala:38-45) for a GroupedIndex on row ids: the lookup above (normalize: MathUtils.normalize,
// as GroupedIndex.query does for a normalized metric, :265-268), then gulon_grouped_index_batch_query on one stream.
GULON_API int32_t gulon_grouped_index_query_rows_dev(gulon_grouped_index *idx, const int32_t *d_rows, int32_t b,
                                                     int32_t k_nn, int32_t normalize, int32_t strategy, int32_t limit,
                                                     int32_t *d_out_idx, float *d_out_dist, int32_t *d_out_count,
                                                     void *stream) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    GULON_REQUIRE(b >= 0 && k_nn >= 0, "k and batch size must be non-negative");
    std::lock_guard<std::mutex> lock(idx->mu);
    const hipStream_t st = (hipStream_t)stream;
    StreamOrder so(idx->pq, st);
    ensure_row_err(idx->pq);
    idx->lq.ensure((size_t)b * idx->d + 1);
    launch_decode_rows(idx->pq, d_rows, b, idx->gcent.p, idx->bounds.p + 1, idx->g - 1, normalize != 0, idx->lq.p,
                       idx->pq->row_err.p, st);
    run_grouped_query(idx, idx->lq.p, b, k_nn, strategy, limit, d_out_idx, d_out_dist, d_out_count, st);
    so.done();
  });
}

GULON_API int32_t gulon_grouped_index_query_rows(gulon_grouped_index *idx, const int32_t *rows, int32_t b, int32_t k_nn,
                                                 int32_t normalize, int32_t strategy, int32_t limit, int32_t *out_idx,
                                                 float *out_dist, int32_t *out_count) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    GULON_REQUIRE(b >= 0 && k_nn >= 0, "k and batch size must be non-negative");
    GULON_REQUIRE(b == 0 || rows != nullptr, "rows is null");
    for (int r = 0; r < b; r++)   // checked before anything is launched
      GULON_REQUIRE(rows[r] >= 0 && rows[r] < idx->n, "row %d = %d outside [0, %d)", r, rows[r], idx->n);
    std::lock_guard<std::mutex> lock(idx->mu);
    query_from_host(idx, b, k_nn, strategy, limit, out_idx, out_dist, out_count, [&](hipStream_t st) {
      idx->rows_dev.ensure((size_t)b + 1);
      HIP_CHECK(hipMemcpyAsync(idx->rows_dev.p, rows, sizeof(int32_t) * (size_t)b, hipMemcpyHostToDevice, st));
      launch_decode_rows(idx->pq, idx->rows_dev.p, b, idx->gcent.p, idx->bounds.p + 1, idx->g - 1, normalize != 0,
                         idx->q_dev.p, nullptr, st);
    });
  });
}

// Offset queries: grouped_offset.hip ranks the rows of every query's searched groups -- coarse_stage's, as
// the ordinary query at the same (strategy, limit) searches them -- by distance + row_offsets[row]; the offsets and the
// excluded rows are indexed by grouped row position, as the returned ids are.
GULON_API int32_t gulon_grouped_index_query_offset(gulon_grouped_index *idx, const float *queries, int32_t b, int32_t k_nn,
                                                   int32_t strategy, int32_t limit, const float *row_offsets,
                                                   const int32_t *exclude, int32_t *out_idx, float *out_key,
                                                   int32_t *out_count) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    check_offset_host(row_offsets, idx->n, exclude, b, k_nn, 0);
    GULON_REQUIRE(strategy == 0 || strategy == 1, "strategy must be 0 (LimitGroups) or 1 (LimitVectors)");
    GULON_REQUIRE(limit >= 0, "limit must be non-negative");
    GULON_UNSUPPORTED(idx->pq->wide, "offset queries take byte codes: k = %d > 256 is not supported", idx->pq->k);
    const GroupScanLds l = group_scan_lds(GroupedCall{idx, nullptr, b, k_nn, strategy, limit, nullptr, nullptr, nullptr, nullptr});
    if (b == 0) return;
    GULON_REQUIRE(queries != nullptr && out_idx != nullptr && out_key != nullptr, "null argument");
    const size_t bk = (size_t)b * (size_t)k_nn;
    if (idx->n == 0) {   // no rows, no candidates: nothing is launched
      std::fill(out_idx, out_idx + bk, -1);
      std::fill(out_key, out_key + bk, INFINITY);
      if (out_count) std::fill(out_count, out_count + b, 0);
      return;
    }
    std::lock_guard<std::mutex> lock(idx->mu);
    const hipStream_t st = nullptr;
    StreamOrder so(idx->pq, st);
    GroupedOffsetWork &x = idx->offset;
    idx->q_dev.upload(queries, (size_t)b * idx->d, st);
    x.off.upload(row_offsets, (size_t)idx->n, st);
    if (exclude) x.ex.upload(exclude, (size_t)b, st);
    idx->oi.ensure(bk); idx->od.ensure(bk); idx->oc.ensure((size_t)b);
    // (coarse_stage's bound on the groups a query searches)
    const int slots = (int)std::min<long long>((long long)limit + (strategy == 1 ? idx->n_empty : 0), idx->g);
    const int per_pass = grouped_offset_pass(slots, k_nn + 1);
    for (int q0 = 0; q0 < b; q0 += per_pass) {
      const int nb = std::min(per_pass, b - q0);
      const GroupedCall c{idx, idx->q_dev.p + (size_t)q0 * idx->d, nb, k_nn, strategy, limit, nullptr, nullptr, nullptr, st};
      const CoarseResult co = coarse_stage(c, /*all_literal=*/true);
      const GroupedOffsetPass pass{idx->pq, idx->gcent.p, idx->bounds.p, c.dQ, nb, idx->nn.p, idx->nn_cnt.p, co.nn_stride,
                                   co.stride, l.bytes};
      launch_grouped_offset(pass, x, k_nn, x.off.p, exclude ? x.ex.p + q0 : nullptr, idx->oi.p + (size_t)q0 * k_nn,
                            idx->od.p + (size_t)q0 * k_nn, idx->oc.p + q0, st);
    }
    idx->oi.download(out_idx, bk, st); idx->od.download(out_key, bk, st);
    if (out_count) idx->oc.download(out_count, (size_t)b, st);
    so.done();
    HIP_CHECK(hipStreamSynchronize(st));
  });
}

namespace gulon {
GroupedParts grouped_parts(gulon_grouped_index *idx) {
  return {idx->pq, idx->gcent.p, idx->bounds.p + 1, idx->g - 1, &idx->mu, idx->bounds.p, idx->g};
}
}  // namespace gulon

GULON_API int32_t gulon_grouped_index_row_error(gulon_grouped_index *idx, int32_t *out) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr && out != nullptr, "null argument");
    std::lock_guard<std::mutex> lock(idx->mu);
    *out = take_row_err(idx->pq);
  });
}

#ifdef GULON_TEST_HOOKS
// The grouped pre-selection on its own (tests/test_gpu_grouped_stage.py, tests/grouped_stage_ref.py).  Builds a grouped
// index from gulon_grouped_index_create's arguments, runs coarse_stage as run_grouped_query does and then, on the same
// nn lists, preselect BOTH ways -- by group (group_filter_run) and through gq_ptables + gq_approx_scan + launch_merge --
// each followed by gq_rerank.  Returns GULON_SELFTEST_GROUPED_REFUSED (78) where the production driver would not take the
// by-group path for this index and batch (by_group_applies), or would not pre-select at all.
// out[]: 0 nn [b][nn_stride], 1 nn_cnt [b], 2 cdist [b][g], 3 xnorm [n], 4 xnlo [g], 5 xcode [ceil(n / 64) 64] bytes,
//   6 gnorm [g], 7 {xnmax, xn_step, gnmax}, 8 P [b][m_pad][256], 9 qs [b][4], 10 qb [b][GF_NT][256] bytes, 11 gcnt [g],
//   12 tiles [meta[0]] GfTile records (room for b nn_stride / 16 + g + 1), 13 meta [4], 14 qcnt [b],
//   15 queue [b][GF_CAP] (row, bits of the base): the first min(qcnt, GF_CAP) of a query, sorted by (row, base),
//   16-18 amv [b][64], ami [b][64], anan [b][16] of the by-group path, 19-21 of the scan path,
//   22-26 out_idx [b][k_nn], out_dist [b][k_nn], out_count [b], redo count [1], redo list [b] of the by-group path,
//   27-31 of the scan path.
// info: nn_stride, m_pad, vec, ng, GF_CAP, GF_PLACED.
// (Declared here and bound by its test: the header's list of hooks is pinned by test_abi.)
GULON_API int32_t gulon_selftest_grouped_stage(const uint8_t *codes, int32_t n, int32_t d, int32_t m, int32_t k,
                                               const float *pq_cents, const float *group_centroids, const int32_t *offsets,
                                               int32_t g, const float *queries, int32_t b, int32_t k_nn, int32_t strategy,
                                               int32_t limit, void **out, int32_t *info) {
  gulon_grouped_index *gx = nullptr;
  bool refused = false;
  const int32_t rc = guarded([&] {
    GULON_REQUIRE(codes && pq_cents && group_centroids && queries && out && info, "null argument");
    GULON_REQUIRE(n >= 1 && b >= 1 && b <= 4096 && k_nn >= 1 && k_nn <= GULON_MAX_K && (strategy == 0 || strategy == 1) && limit >= 1,
                  "bad arguments");
    for (int i = 0; i < 32; i++) GULON_REQUIRE(out[i] != nullptr, "out[%d] is null", i);
    GULON_REQUIRE(gulon_grouped_index_create(codes, n, d, m, k, pq_cents, group_centroids, offsets, g, &gx) == GULON_OK && gx, "no index");
    gulon_index *ix = gx->pq;
    GroupFilter &gf = gx->gfilter;
    if (ix->wide || gx->xnorm.n == 0 || !gf.built) { refused = true; return; }
    hipStream_t st = nullptr;
    const int B = b, K = k_nn;
    gx->q_dev.upload(queries, (size_t)B * d, st);
    DevBuf<int> oi((size_t)B * K), oc((size_t)B);
    DevBuf<float> od((size_t)B * K);
    const GroupedCall c{gx, gx->q_dev.p, B, K, strategy, limit, oi.p, od.p, oc.p, st};
    const CoarseResult co = coarse_stage(c, false);
    if (!by_group_applies(c, co)) { refused = true; return; }
    const int nn_stride = co.nn_stride;
    gx->qlist.ensure((size_t)B);
    gx->qcount.ensure(1);
    auto get = [&](int slot, const void *dev, size_t bytes) {
      if (bytes) HIP_CHECK(hipMemcpy(out[slot], dev, bytes, hipMemcpyDeviceToHost));
    };
    for (int path = 0; path < 2; path++) {   // 0: by group, 1: gq_approx_scan
      HIP_CHECK(hipMemsetAsync(gx->qcount.p, 0, sizeof(int), st));
      HIP_CHECK(hipMemsetAsync(gx->qlist.p, 0xFF, sizeof(int) * (size_t)B, st));
      preselect(c, co, path == 0);
      launch_rerank(c);
      HIP_CHECK(hipStreamSynchronize(st));
      const int l0 = 16 + 3 * path, r0 = 22 + 5 * path;
      get(l0, gx->amv.p, sizeof(float) * (size_t)B * GA_C);
      get(l0 + 1, gx->ami.p, sizeof(int) * (size_t)B * GA_C);
      get(l0 + 2, gx->anan.p, sizeof(int) * (size_t)B * GA_WAVES);
      get(r0, oi.p, sizeof(int) * (size_t)B * K);
      get(r0 + 1, od.p, sizeof(float) * (size_t)B * K);
      get(r0 + 2, oc.p, sizeof(int) * (size_t)B);
      get(r0 + 3, gx->qcount.p, sizeof(int));
      get(r0 + 4, gx->qlist.p, sizeof(int) * (size_t)B);
      if (path == 0) {   // the by-group path's state, before the other path overwrites the tables
        get(8, gx->ptab.p, sizeof(float) * (size_t)B * ix->m_pad * 256);
        get(9, gf.qs.p, sizeof(float) * (size_t)B * 4);
        get(10, gf.qb.p, (size_t)B * GF_NT * 256);
        get(11, gf.gcnt.p, sizeof(int) * (size_t)g);
        int meta[4];
        HIP_CHECK(hipMemcpy(meta, gf.meta.p, sizeof(meta), hipMemcpyDeviceToHost));
        memcpy(out[13], meta, sizeof(meta));
        const size_t tiles_room = (size_t)B * nn_stride / GF_QT + (size_t)g + 1;
        GULON_REQUIRE(meta[0] >= 0 && (size_t)meta[0] <= tiles_room, "internal: %d tiles", meta[0]);
        get(12, gf.tiles.p, sizeof(GfTile) * (size_t)meta[0]);
        std::vector<int> qcnt((size_t)B);
        HIP_CHECK(hipMemcpy(qcnt.data(), gf.qcnt.p, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost));
        memcpy(out[14], qcnt.data(), sizeof(int) * (size_t)B);
        std::vector<unsigned long long> ent((size_t)GF_CAP);
        for (int q = 0; q < B; q++) {
          const size_t cnt = (size_t)std::min(std::max(qcnt[q], 0), GF_CAP);
          if (cnt) HIP_CHECK(hipMemcpy(ent.data(), gf.queue.p + (size_t)q * GF_CAP, sizeof(uint2) * cnt, hipMemcpyDeviceToHost));
          std::vector<std::pair<uint32_t, uint32_t>> pr(cnt);
          for (size_t e = 0; e < cnt; e++) pr[e] = {(uint32_t)(ent[e] & 0xFFFFFFFFull), (uint32_t)(ent[e] >> 32)};
          std::sort(pr.begin(), pr.end());
          uint32_t *o = static_cast<uint32_t *>(out[15]) + (size_t)q * GF_CAP * 2;
          for (size_t e = 0; e < cnt; e++) { o[2 * e] = pr[e].first; o[2 * e + 1] = pr[e].second; }
        }
      }
    }
    get(0, gx->nn.p, sizeof(int) * (size_t)B * nn_stride);
    get(1, gx->nn_cnt.p, sizeof(int) * (size_t)B);
    get(2, gx->cdist.p, sizeof(float) * (size_t)B * g);
    get(3, gx->xnorm.p, sizeof(float) * (size_t)n);
    get(4, gf.xnlo.p, sizeof(float) * (size_t)g);
    get(5, gf.xcode.p, (size_t)ceil_div(n, 64) * 64);
    get(6, gf.gnorm.p, sizeof(float) * (size_t)g);
    const float sc[3] = {gx->xnmax, gf.xn_step, gf.gnmax};
    memcpy(out[7], sc, sizeof(sc));
    info[0] = nn_stride; info[1] = ix->m_pad; info[2] = ix->vec; info[3] = ix->ng; info[4] = GF_CAP; info[5] = GF_PLACED;
  });
  if (gx) (void)gulon_grouped_index_destroy(gx);
  return rc != GULON_OK ? rc : refused ? 78 : GULON_OK;
}

// The group selection on its own (tests/test_gpu_group_select.py, tests/group_select_ref.py).  Builds a
// grouped index from gulon_grouped_index_create's arguments and calls coarse_stage(c, all_literal) as the drivers do
// (K = 1).  lit_flag and sel_ok are filled with -1 first, so the caller sees which kernels wrote them.  Where the
// order-only ties are still to be redone (!all_literal and lit_cap > 0) the level-1 pass then runs as redo_flagged runs
// it, over a list of every query, and nn / nn_cnt are returned a second time.
// out[]: 0 nn [b][nn_stride], 1 nn_cnt [b], 2 cdist [b][g], 3 lit_flag [b], 4 sel_ok [b], 5 nn after the level-1 pass,
//   6 nn_cnt after it (5 and 6 are left alone where the pass does not run).  Room for [b][min(limit + g, g)] = [b][g]
//   entries in 0 and 5.
// info: nn_stride, stride, lit_cap.
// (Declared here and bound by its test, like the hook above.)
GULON_API int32_t gulon_selftest_group_selection(const uint8_t *codes, int32_t n, int32_t d, int32_t m, int32_t k,
                                                 const float *pq_cents, const float *group_centroids, const int32_t *offsets,
                                                 int32_t g, const float *queries, int32_t b, int32_t strategy, int32_t limit,
                                                 int32_t all_literal, void **out, int32_t *info) {
  gulon_grouped_index *gx = nullptr;
  const int32_t rc = guarded([&] {
    GULON_REQUIRE(pq_cents && group_centroids && queries && out && info, "null argument");
    GULON_REQUIRE(b >= 1 && b <= 4096 && (strategy == 0 || strategy == 1) && limit >= 1, "bad arguments");
    for (int i = 0; i < 7; i++) GULON_REQUIRE(out[i] != nullptr, "out[%d] is null", i);
    GULON_REQUIRE(gulon_grouped_index_create(codes, n, d, m, k, pq_cents, group_centroids, offsets, g, &gx) == GULON_OK && gx, "no index");
    hipStream_t st = nullptr;
    const int B = b;
    gx->q_dev.upload(queries, (size_t)B * d, st);
    gx->lit_flag.ensure((size_t)B);
    gx->sel_ok.ensure((size_t)B);
    HIP_CHECK(hipMemsetAsync(gx->lit_flag.p, 0xFF, sizeof(int) * (size_t)B, st));
    HIP_CHECK(hipMemsetAsync(gx->sel_ok.p, 0xFF, sizeof(int) * (size_t)B, st));
    const GroupedCall c{gx, gx->q_dev.p, B, 1, strategy, limit, nullptr, nullptr, nullptr, st};
    const CoarseResult co = coarse_stage(c, all_literal != 0);
    HIP_CHECK(hipStreamSynchronize(st));
    auto get = [&](int slot, const void *dev, size_t bytes) {
      if (bytes) HIP_CHECK(hipMemcpy(out[slot], dev, bytes, hipMemcpyDeviceToHost));
    };
    get(0, gx->nn.p, sizeof(int) * (size_t)B * co.nn_stride);
    get(1, gx->nn_cnt.p, sizeof(int) * (size_t)B);
    get(2, gx->cdist.p, sizeof(float) * (size_t)B * g);
    get(3, gx->lit_flag.p, sizeof(int) * (size_t)B);
    get(4, gx->sel_ok.p, sizeof(int) * (size_t)B);
    if (!all_literal && co.lit_cap > 0) {   // redo_flagged's pass over the group order, every query listed
      std::vector<int> ql((size_t)B);
      for (int q = 0; q < B; q++) ql[q] = q;
      gx->qlist.upload(ql.data(), (size_t)B, st);
      gx->qcount.upload(&B, 1, st);
      launch_literal_groups(c, co.nn_stride, co.lit_cap, 1, std::min(B, 16), gx->qlist.p, gx->qcount.p);
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipStreamSynchronize(st));
      get(5, gx->nn.p, sizeof(int) * (size_t)B * co.nn_stride);
      get(6, gx->nn_cnt.p, sizeof(int) * (size_t)B);
    }
    info[0] = co.nn_stride; info[1] = co.stride; info[2] = co.lit_cap;
  });
  if (gx) (void)gulon_grouped_index_destroy(gx);
  return rc;
}
#endif
