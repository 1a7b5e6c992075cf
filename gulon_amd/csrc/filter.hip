// Quantized lower-bound filter in front of the exact ADC scan (PQIndex.batchQuery,
// Index.scala:393-440).  Results are the exact path's, bit for bit; only the work changes.
//
// The exact scan gathers one fp32 table entry per (query, row, quantizer) from LDS, and the LDS
// gather bandwidth is what bounds it.  A table entry here is 8 bits, so one
// ds_read_b128 serves 16 queries instead of 4:
//
//   1. the exact distances of a few thousand strided sample rows give every query a valid upper
//      bound tau on its final (K+1)-th distance (the (K+1)-th smallest of a subset);
//   2. per query the fp32 table T_j[c] is quantized DOWNWARDS (min_j comes out of build_tables):
//        q_j[c] = min(QMAX, floor((T_j[c] - min_j) / delta)),  delta = (tau' - sum_j min_j) / QL,
//      where tau' = tau * (1 + 2 m u), u = 2^-24, covers the rounding of the reference's
//      sequential fp32 sum D against the real sum R (all terms >= 0: D >= R (1 - m u)).
//      (As evaluated, in fp64: tau' = tau * (1 + 2 m_pad * 5.97e-8) * (1 + 1e-9) -- m and u rounded up, and a margin
//      for the fp64 arithmetic itself; wf_quantize of wide_filter.hip: the same with its m.)
//      Then  sum_j min_j + delta * sum_j q_j[c_j]  <=  R,  and a row with  sum_j q_j > QL  has
//      R > tau', hence D > tau: it cannot be among the K+1 smallest and is dropped;
//   3. the (few) surviving (query, row) pairs are queued and re-evaluated with the exact fp32
//      tables in the reference's summation order, and merged into the running (K+1)-lists under
//      the same (distance, row id) order as the exact scan.
//
// The rows go through three filter stages over disjoint, strided sets of row blocks (two short
// ones that tighten tau, then the rest).  A query whose bound is unusable (NaN/inf) or whose survivor queue overflows is redone
// by the exact scan (per query tile, decided on the device), so the filter never changes a result.
//
// This file: the kernels and one launcher per kernel.  The query driver that strings them together, level 2 of the tie
// replay and the stage hook of the tests: filter_query.hip.
#include <atomic>
#include <type_traits>

#include "scan.hpp"
#include "select.hpp"

namespace gulon {

namespace {

// (FILTER_THREADS, filter_kernel's workgroup, NSLOT and FILTER_LDS_BUDGET: scan.hpp)
constexpr int BOUND_THREADS = 1024;                     // bound_tables' workgroup

// fp32 table entry (j, c) of query q; W queries are interleaved per entry (scan.hip build_tables)
__device__ inline float table_at(const float *__restrict__ tables, int W, int m_pad, int q, int j, int c) {
  return tables[(((size_t)(q / W) * m_pad + j) * 256 + c) * W + q % W];
}

// ---- quantize the tables of four queries (one dword of an entry) against the current bounds ----
__global__ __launch_bounds__(256) void qt_quantize(const float *__restrict__ tables, int W, int Bp, int m_pad, int k,
                                                   int B, const float *__restrict__ mins,
                                                   const float *__restrict__ fin_v, const int *__restrict__ fin_i,
                                                   const float *__restrict__ tau0, int keff, int qmax, int QW,
                                                   uint8_t *__restrict__ qtab /*[Bq/QW][m_pad][256][QW]*/,
                                                   int *__restrict__ fb_tile, int qt,
                                                   const int *__restrict__ slot = nullptr /* table / minima of query q: those of slot[q] */) {
  // One workgroup = the 256 centroids of ONE quantizer for FOUR queries (one dword of a table entry): 4 x the
  // workgroups of a 16-query form with a quarter of the serial work each -- the kernel is latency, not throughput
  // (20 us per launch on a 1.25 M-row shard as 1024 workgroups that walked their 16 queries in four dependent steps).
  __shared__ float s_inv32[4];
  __shared__ float s_min[4];
  __shared__ int s_dead[4];
  __shared__ float s_mins[4 * 144];                // the four queries' table minima (m_pad <= 144)
  const int g4 = blockIdx.x, j = blockIdx.y, c = threadIdx.x;
  // everything the workgroup reads is requested up front -- its table entries, the 4 x m_pad minima (coalesced) and
  // each query's bound -- so that the memory round trips overlap
  float vv[4];
#pragma unroll
  for (int u = 0; u < 4; u++) {
    const int q = g4 * 4 + u;
    vv[u] = (q < Bp && c < k) ? table_at(tables, W, m_pad, slot ? slot[q] : q, j, c) : 0.f;
  }
  for (int e = c; e < 4 * m_pad; e += 256) {
    const int qq = e / m_pad, jj = e - qq * m_pad, q = g4 * 4 + qq;
    s_mins[e] = q < B ? mins[(size_t)(slot ? slot[q] : q) * m_pad + jj] : 0.f;
  }
  float tau = INFINITY;
  int fb = 1;
  if (c < 4 && g4 * 4 + c < B) {
    const int q = g4 * 4 + c;
    // bound = the sample's, tightened by the running list once that is full
    const float t0 = tau0[q], fv = fin_v[(size_t)q * keff + keff - 1];
    const int fi = fin_i[(size_t)q * keff + keff - 1];
    fb = fb_tile[q / qt];
    tau = fi != INT_MAX ? fminf(t0, fv) : t0;
  }
  __syncthreads();
  if (c < 4) {
    const int q = g4 * 4 + c;
    int dead = 1;
    double delta = 1.0;
    if (q < B) {
      if (fb != 0) {
        // this query tile already goes to the exact scan (unusable bound, queue overflow, or a
        // first stage that let too many rows through): nothing of it is filtered any more
      } else if (!(tau < INFINITY)) {
        if (j == 0) fb_tile[q / qt] = 1;          // no usable bound: this query is redone exactly
      } else {
        double sum_min = 0.0;
        for (int jj = 0; jj < m_pad; jj++) sum_min += (double)s_mins[c * m_pad + jj];
        const double taup = (double)tau * (1.0 + 2.0 * m_pad * 5.97e-8) * (1.0 + 1e-9);
        double budget = taup - sum_min;
        if (!(budget > 0.0)) budget = 0.0;
        delta = budget / (double)(qmax - 1);
        if (delta < 1e-290) delta = 1e-290;
        dead = 0;
      }
    }
    s_dead[c] = dead;
    // 1 / delta for the fp32 levels below: rounded to fp32 (<= 2^-24 relative), then shrunk by 2^-21; for a delta so
    // small that the reciprocal overflows fp32 the largest finite value short of it, 3.0e38, stands in (+inf would turn
    // an entry AT its minimum, x = 0, into 0 * inf = NaN and that into the top level): the levels then come out far
    // below x / delta -- 0 for every x below 1 / 3.0e38 -- which is valid (levels only ever round down) and filters
    // little; entries from about QMAX / 3.0e38 up still get the top level
    float inv32 = (float)(1.0 / delta);
    inv32 = inv32 < INFINITY ? inv32 * (1.0f - 4.76837158e-7f) : 3.0e38f;
    s_inv32[c] = inv32;
    s_min[c] = s_mins[c * m_pad + j];
  }
  __syncthreads();
  // The level of an entry in fp32, rounded DOWN for certain: x = T - min (one rounding, <= 2^-24 relative), times the
  // reciprocal of delta, which the prologue shrank by 2^-21 (fp64 -> fp32, the shrinking, the subtraction, the product: four roundings of
  // 2^-24 each = 2^-22) -- they cannot carry the product above the real quotient x / delta, so  level * delta <= x  holds as the bound
  // needs it (the fp64 form of this -- conversions, a guard loop -- was a dozen half- and quarter-rate instructions
  // per entry on a vector ALU that another batch's main stage keeps 90 % busy).  Levels are < 256: exact in fp32.
  uint32_t word = 0;
#pragma unroll
  for (int u = 0; u < 4; u++) {
    const int q = g4 * 4 + u;
    const bool have = q < Bp && c < k;
    const float v = vv[u];
    int qv = qmax;
    if (have && !s_dead[u] && v == v) {
      float x = v - s_min[u];
      if (!(x > 0.f)) x = 0.f;
      const float r = x * s_inv32[u];
      if (r < (float)qmax) qv = (int)r;                      // floor: r >= 0
    }
    word |= (uint32_t)qv << (8 * u);
  }
  // queries 4 g4 .. + 3 -> dword (4 g4 % QW) / 4 of entry [4 g4 / QW][j][c] (QW bytes per entry)
  const int grp = (g4 * 4) / QW, part = (g4 * 4 % QW) / 4;
  reinterpret_cast<uint32_t *>(qtab)[(((size_t)grp * m_pad + j) * 256 + c) * (QW / 4) + part] = word;
}

// ---- initial bounds from a strided sample of row blocks ---------------------------------------
// One workgroup per W queries (bound_tables below), their W-interleaved fp32 table in LDS, lane = row as in the
// exact scan -- but no top-k lists in the loop: every lane only keeps the minimum exact distance
// of the rows it saw (1024 disjoint groups of rows per workgroup).  Any K+1 group minima belong
// to K+1 distinct rows, so the (K+1)-th smallest group minimum bounds the final (K+1)-th
// distance from above; with 1024 groups it is almost always the sample's own (K+1)-th distance.
// Selection = one 64-lane bitonic sort per wave and query, then a sorted merge of the 16 waves.
// (sort64_asc / merge64_asc: select.hpp.)

template <int W> struct FTab;
template <> struct FTab<4> { using type = float4; };
template <> struct FTab<2> { using type = float2; };
template <> struct FTab<1> { using type = float; };

// ---- the batch's first kernel: reset + Index.prepareQuery + sample scan in ONE launch ---------------------------
// The three were separate launches (filter_reset, build_tables, bound_scan): 5 + 25 + 40 us on a 1.25 M-row shard, a
// quarter of what the batch spends outside its main-stage kernel, and build_tables' 4096 workgroups take the whole chip
// from another batch's filter kernel for their 20 us.  A sample-scan workgroup needs the fp32 tables of its W queries
// in LDS anyway, so it BUILDS them there -- Index.prepareQuery's arithmetic (Index.scala:352-383: d = q - c,
// sum += d * d, sequential, unfused), the same expression build_tables evaluates, hence the same bits -- writes them
// out for the survivor pass, reduces the per-(query, quantizer) minima the quantisation needs, and clears its share of
// the batch's counters on the way.  16 waves: wave w builds quantizers w, w + 16, ...; quantizer and
// query are wave-uniform, so the query values arrive through scalar loads.
template <int VEC, int W>
__global__ __launch_bounds__(BOUND_THREADS) void bound_tables(
    const float *__restrict__ cents, const int *__restrict__ from, const int *__restrict__ sdim, int d, int m, int k,
    const float *__restrict__ Q, float *__restrict__ tables, float *__restrict__ mins,
    const uint8_t *__restrict__ codes, const uint8_t *__restrict__ perm /* codes = the conflict-ordered copy: its row order */,
    int pwin /* blocks per ordering window of that copy - 1 */, int ng, int m_pad, int row_from, int row_until, int rb_begin, int e_count,
    RbMap mp, int B, int keff, float *__restrict__ tau0, float *__restrict__ fin_v, int *__restrict__ fin_i,
    float *__restrict__ bounds_out, unsigned *__restrict__ gtau, int n_gtau, int *__restrict__ fb_tile, int n_fb,
    int *__restrict__ sv_cnt, int n_cnt) {
  constexpr int NW = BOUND_THREADS / 64;
  using Word = typename CodeWord<VEC>::type;
  using TV = typename FTab<W>::type;
  extern __shared__ uint4 qlds[];
  TV *lds = reinterpret_cast<TV *>(qlds);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qg = blockIdx.x;
  // (1) this batch's counters: pruning thresholds of the fallback scan, tile flags, survivor sub-queue fill levels
  for (int t = qg * BOUND_THREADS + tid; t < max(n_gtau, max(n_fb, n_cnt)); t += gridDim.x * BOUND_THREADS) {
    if (t < n_gtau) gtau[t] = 0x7F800000u;   // +inf
    if (t < n_fb) fb_tile[t] = 0;
    if (t < n_cnt) sv_cnt[t] = 0;
  }
  if (qg * W >= B) return;                    // a padding group of the last query tile: no table, no bound
  // (2) tables of queries qg*W .. +W-1, W-interleaved: entry (j, c) at lds[j * 256 + c].  Wave w owns quantizers
  // w, w + 16, ...: sub-vector bounds and query values are wave-uniform, lane l evaluates centroids l, l + 64,
  // l + 128, l + 192 one after the other, and the table minimum of a (query, quantizer) pair is a reduction inside the
  // wave.  The loops are ROLLED on purpose: every wave runs through this code once per batch, out of a cold instruction
  // cache -- unrolled (6.5 KiB) the section took 17.8 us of which the arithmetic is < 1 us (per-phase stamps); what
  // such straight-line code costs is its size.
  for (int j = wave; j < m_pad; j += NW) {
    int fr = 0, s = 0;
    if (j < m) { fr = from[j]; s = sdim[j]; }
    const float *cc = cents + (size_t)k * fr;
    float mnu[W];
#pragma unroll
    for (int u = 0; u < W; u++) mnu[u] = INFINITY;
#pragma unroll 1
    for (int i = 0; i < 4; i++) {
      const int c = lane + 64 * i;
      float acc[W];
#pragma unroll
      for (int u = 0; u < W; u++) acc[u] = 0.f;
#pragma unroll 1
      for (int t0 = 0; t0 < s; t0 += 8) {
        // eight dimensions per step.  The query values: lane 8 u + e loads component t0 + e of query u (one vector
        // load; 32 guarded scalar loads took eight memory round trips), every lane then reads them with v_readlane.
        // Dimensions beyond s contribute (0 - 0)^2 = +0 to a sum that is >= +0 or NaN: no change.
        float qreg = 0.f;
        {
          const int lu = lane >> 3, le = lane & 7;
          if (lu < W && t0 + le < s && qg * W + lu < B) qreg = Q[(size_t)(qg * W + lu) * d + fr + t0 + le];
        }
        // the centroid's eight components: two 16-byte loads where all eight exist (dword-aligned: s is arbitrary).
        // Eight dword loads per lane, 32 bytes apart from lane to lane, touched every cache line eight times over and
        // made this loop L1-bound: 3 us per centroid group (per-phase stamps)
        float cv[8];
        if (t0 + 8 <= s) {
          typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
          f32x4u lo = {0.f, 0.f, 0.f, 0.f}, hi = {0.f, 0.f, 0.f, 0.f};
          if (c < k) {
            const f32x4u *row = reinterpret_cast<const f32x4u *>(cc + (size_t)c * s + t0);
            lo = row[0]; hi = row[1];
          }
#pragma unroll
          for (int e = 0; e < 4; e++) { cv[e] = lo[e]; cv[4 + e] = hi[e]; }
        } else {
#pragma unroll
          for (int e = 0; e < 8; e++) cv[e] = (t0 + e < s && c < k) ? cc[(size_t)c * s + t0 + e] : 0.f;
        }
#pragma unroll
        for (int e = 0; e < 8; e++) {
#pragma unroll
          for (int u = 0; u < W; u++) {
            const float dd = readlane_f(qreg, 8 * u + e) - cv[e];
            acc[u] += dd * dd;
          }
        }
      }
      TV tv;
#pragma unroll
      for (int u = 0; u < W; u++) {
        if (!(c < k && qg * W + u < B)) acc[u] = 0.f;         // entries beyond k / of padding queries: zero
        reinterpret_cast<float *>(&tv)[u] = acc[u];
        if (c < k && acc[u] == acc[u]) mnu[u] = fminf(mnu[u], acc[u]);   // NaN entries are ignored
      }
      lds[j * 256 + c] = tv;       // (to LDS only: see the copy-out below)
    }
#pragma unroll
    for (int u = 0; u < W; u++) {
      float x = mnu[u];
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) x = fminf(x, __shfl_xor(x, o));
      if (lane == 0) mins[(size_t)(qg * W + u) * m_pad + j] = x;
    }
  }
  __syncthreads();
  // (3) the sample scan (see above): lane = row, every lane keeps the minimum exact distance it saw
  const Word *cw = reinterpret_cast<const Word *>(codes);
  int mp_p = wave / mp.width, mp_r = wave - mp_p * mp.width;
  auto block_of = [&](int p, int r) { return rb_begin + p * mp.period + mp.lo + r; };
  auto advance = [&](int &p, int &r) { r += NW; while (r >= mp.width) { r -= mp.width; p++; } };
  float mn[W];
#pragma unroll
  for (int u = 0; u < W; u++) mn[u] = INFINITY;
  Word w_first{};
  if (wave < e_count) w_first = cw[((size_t)block_of(mp_p, mp_r) * ng) * 64 + lane];
  // The tables leave for global memory (the survivor pass and the quantisation read them) only now, in one burst
  // BEHIND the first code-word request.  vmcnt counts loads and stores together, in order: with the store of a
  // centroid group inside the build loop, the next group's loads waited for that store to be acknowledged (~3 us
  // each, per-phase stamps: first group after 2.7 us, fourth after 11.5); a wait for the code word requested before
  // the burst leaves the stores in flight.
  for (int e = tid; e < m_pad * 256; e += BOUND_THREADS)
    reinterpret_cast<TV *>(tables)[(size_t)qg * m_pad * 256 + e] = lds[e];
  for (int e = wave; e < e_count; e += NW) {
    const int rb = block_of(mp_p, mp_r);
    advance(mp_p, mp_r);
    const Word *p = cw + ((size_t)rb * ng) * 64 + lane;
    Word w = w_first;
    if (e + NW < e_count) w_first = cw[((size_t)block_of(mp_p, mp_r) * ng) * 64 + lane];
    float acc[W];                            // the reference's order: j ascending, unfused fp32
#pragma unroll
    for (int u = 0; u < W; u++) acc[u] = 0.f;
    for (int g = 0; g < ng; g++) {
      Word wn = w;
      if (g + 1 < ng) wn = p[(size_t)(g + 1) * 64];
      const TV *tj = lds + g * VEC * 256;
#pragma unroll
      for (int b = 0; b < VEC; b++) {
        const TV t = tj[b * 256 + code_byte<VEC>(w, b)];
        const float *tf = reinterpret_cast<const float *>(&t);
#pragma unroll
        for (int u = 0; u < W; u++) acc[u] += tf[u];
      }
      w = wn;
    }
    // which row a lane holds only matters in a window the range cuts (the conflict-ordered copy deals a window's rows to
    // the lanes of its blocks by `perm`; the sample only needs distances of DISTINCT rows of the range)
    bool valid = true;
    const int wrow = (rb & ~pwin) * 64;               // first row of the block's ordering window
    if (wrow < row_from || wrow + 64 * (pwin + 1) > row_until) {
      const int row = wrow + (perm ? (int)perm[(size_t)rb * 64 + lane] : lane);
      valid = row >= row_from && row < row_until;
    }
    if (valid) {
#pragma unroll
      for (int u = 0; u < W; u++) mn[u] = fminf(mn[u], acc[u]);   // NaN distances are ignored
    }
  }
  __syncthreads();                     // the table is dead: reuse LDS for the per-wave sorted minima
  float *sv = reinterpret_cast<float *>(qlds);
#pragma unroll
  for (int u = 0; u < W; u++) sv[(u * NW + wave) * 64 + lane] = mn[u];
#pragma unroll 1                       // (one copy of the sorting network, not W: code size again)
  for (int u = 0; u < W; u++) {
    float *slot = sv + (u * NW + wave) * 64 + lane;
    *slot = sort64_asc(*slot, lane);
  }
  __syncthreads();
  if (wave < W) {
    const int u = wave, q = qg * W + u;
    float best = sv[(u * NW) * 64 + lane];
#pragma unroll 1
    for (int w2 = 1; w2 < NW; w2++) best = merge64_asc(best, sv[(u * NW + w2) * 64 + lane], lane);
    if (q < B) {
      if (lane == keff - 1) tau0[q] = best;          // +inf when fewer than K+1 groups saw a row
      if (lane < keff) { fin_v[(size_t)q * keff + lane] = INFINITY; fin_i[(size_t)q * keff + lane] = INT_MAX; }
      if (bounds_out && lane < keff) bounds_out[(size_t)q * keff + lane] = best;   // for the other shards
    }
  }
}

// ---- bounds shared across shards: tau0[q] = the keff-th smallest of the union of `lists` ascending
// arrays of keff sample distances (one per shard, this shard's own among them).  Each of them belongs
// to a distinct row of the whole index, so the value bounds the index-wide keff-th distance from above.
// One wave per query; bisection over the ordered bit patterns (32 counting passes over <= 64 * lists values).
__global__ __launch_bounds__(256) void shared_tau(const float *__restrict__ all /*[lists][B][keff]*/, int lists, int B,
                                                  int keff, float *__restrict__ tau0) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= B) return;
  const int n = lists * keff;
  auto key_at = [&](int i) {
    const int l = i / keff, e = i - l * keff;
    return ordered_key(all[((size_t)l * B + q) * keff + e]);    // unsigned order = float order
  };
  constexpr int R = 4;                                           // values per lane held in registers
  uint32_t held[R];
#pragma unroll
  for (int r = 0; r < R; r++) held[r] = lane + 64 * r < n ? key_at(lane + 64 * r) : 0xFFFFFFFFu;
  uint32_t t = 0;
  for (int bit = 31; bit >= 0; bit--) {
    const uint32_t cand = t | (1u << bit);
    int c = 0;
#pragma unroll
    for (int r = 0; r < R; r++) c += held[r] < cand ? 1 : 0;
    for (int i = lane + 64 * R; i < n; i += 64) c += key_at(i) < cand ? 1 : 0;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) c += __shfl_xor(c, o);
    if (c < keff) t = cand;                                      // fewer than keff values below: go up
  }
  if (lane == 0) {
    const float v = ordered_float(t);
    if (v == v) tau0[q] = fminf(tau0[q], v);
  }
}

// ---- the filter: lane = row, 16*NQG queries per workgroup, NADD entries summed per byte -------
// MAIN only tags the instantiation used for the last (large) stage, so that profilers list it apart
// from the short first stage.
template <int QW> struct QEntry;                     // QW queries (one byte each) per table entry
template <> struct QEntry<16> { using type = uint4; };
template <> struct QEntry<8> { using type = uint2; };
template <> struct QEntry<4> { using type = uint32_t; };

// (pk_sub_sat_u16: select.hpp)
__device__ inline uint32_t pk_min_u16(uint32_t a, uint32_t b) {   // per 16-bit half: min(a, b), unsigned
  typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}

template <int QW, int NQG, int VEC, int NADD, int MAIN,
          int NG1 /* 1: a single code word per row (ng == 1); 2: and `codes` is the conflict-ordered copy, `perm` its row order;
                     3: and `codes` is the key-sorted copy, `perm` its 32-bit row ids (conflict_order.hip) */,
          int PFX = 0 /* key-sorted main stage: quantizers tested per row before the others are looked up (0: all at once) */>
__global__ __launch_bounds__(FILTER_THREADS) void filter_kernel(
    const uint8_t *__restrict__ codes, const uint8_t *__restrict__ perm, int ng, int m_pad, const uint8_t *__restrict__ qtab, int row_from, int row_until,
    int rb_begin, int e_count, int e_per_chunk, RbMap mp, int *__restrict__ cnt, int *__restrict__ queue, int cap /* entries per sub-queue */,
    const int *__restrict__ fb_tile, int qt, int B,
    int pwin /* ordered copy: blocks per ordering window - 1 (0 or 3) -- `perm` = a row's place in its window */) {
  constexpr int NW = FILTER_THREADS / 64;
  constexpr uint32_t QMAXP = (255u / NADD) * 0x00010001u;   // QMAX in both halves; survive <=> sum <= QMAX - 1
  constexpr int DW = QW / 4;     // dwords per entry
  // The kernel runs at the LDS random-gather floor, and the vector L1 is a second gather
  // pipe that sits idle: the entries of the last GLB quantizers of a code word are read from the quantized
  // table in global memory (4 KiB per tile and quantizer: L1-resident) instead of its LDS copy, requested at
  // the top of the row block so that their latency passes under the LDS gathers.  Measured on the 10 M-row
  // bench index (two batches in flight / main stage alone): 3.44 / 3.00 ms with every entry from LDS,
  // 3.06 / 2.66 with 2 from L1, 3.04 / 2.57 with 3, 3.06 / 2.66 with 4 (requested where they are used instead
  // of up front: 3.21, 3.23, 3.36; five 3.96, eight 5.58 -- the L1 path saturates quickly).  It pays only where
  // LDS is the one busy pipe: 16-byte entries, four entries summed per widening, two workgroups per CU (m <= 16);
  // with 4-byte code words, wider indexes (m = 32, 64, 100) or the 7-bit levels it measured 2-50 % slower.
  // What the L1 path carries (scripts/micro/l1_gather.hip): a 16-byte gather returns 64 bytes per
  // cycle at best -- 16.5 cycles per wave-instruction whenever its lanes touch up to 16 distinct 128-byte lines or
  // equal lines sit in neighbouring lanes -- and 32 cycles for 64 random entries of a 4 KiB table; the coalesced code
  // word costs another 16.  Three random look-ups and the code word are 112 cycles of the ~118 a row block takes: that
  // is why a fourth never paid.  In the key-sorted copy (NG1 == 3) a row block holds one value of code 15 and a few of
  // code 14, so those two cost 16.5 cycles each and a FOURTH look-up fits (2 x 32 + 2 x 16.5 + 16 = 113) -- one LDS
  // gather fewer per block.  Measured per batch at 10 M rows: 2.33 ms window-ordered, 2.26 with 3 L1 look-ups in the
  // sorted copy, 2.24 with 4, 2.66 with 5.
  constexpr bool SORTED = NG1 == 3;
  constexpr int GLB = (QW == 16 && NQG == 1 && VEC == 16 && NADD == 4 && NG1) ? (SORTED ? GULON_FILTER_SORT_GLB : GULON_FILTER_GLB) : 0;
  using Word = typename CodeWord<VEC>::type;
  using QE = typename QEntry<QW>::type;
  extern __shared__ uint4 qlds_raw[];
  QE *qlds = reinterpret_cast<QE *>(qlds_raw);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // (MAIN == 2: chunks along x -- consecutive workgroups go to different XCDs, and with the tiles served in the order of
  // their row limits every XCD then gets the same share of every tile)
  const int tile = MAIN == 2 ? blockIdx.y : blockIdx.x, chunk = MAIN == 2 ? blockIdx.x : blockIdx.y;
  const int ntile = MAIN == 2 ? gridDim.y : gridDim.x;
  const int tab = m_pad * 256;   // entries per QW-query group
  {   // every query of this tile already goes to the exact scan: nothing to do here
    const int q_lo = tile * NQG * QW, q_hi = min(B, q_lo + NQG * QW);
    bool any_live = false;
    if (q_hi > q_lo)
      for (int t = q_lo / qt; t <= (q_hi - 1) / qt; t++) any_live = any_live || fb_tile[t] == 0;
    if (!any_live) return;
  }
  // MAIN == 2 (the tie replay's long level, one flag per query, every row block of the range): behind the flags sits
  // one number per query tile, the last row block any of its queries can still take a row from (replay.hip)
  int e_limit = e_count;
  if constexpr (MAIN == 2) {
    const int nflags = (ntile * NQG * QW + 15) & ~15;
    e_limit = min(e_count, (fb_tile[nflags + tile] | pwin) - rb_begin + 1);   // (a row sits somewhere in its window)
    if (chunk * e_per_chunk >= e_limit) return;
  }
  // spreads the queue-tail atomics of one query over NSLOT counters
  const int slot = (chunk * NW + wave) & (NSLOT - 1);
  {
    const int n16 = NQG * tab * QW / 16;   // 16-byte units (tab * QW is a multiple of 16)
    const uint4 *src = reinterpret_cast<const uint4 *>(qtab) + (size_t)tile * n16;
    // (the key-sorted form never reads the LDS copy of its L1-served quantizers: the last of the one group's table)
    const int n16_lds = SORTED ? (VEC - GLB) * 256 * QW / 16 : n16;
    for (int e = tid; e < n16_lds; e += FILTER_THREADS) qlds_raw[e] = src[e];
    if (tid == 0) *reinterpret_cast<int *>(qlds_raw + n16) = NW;   // run counter: the first NW runs are the waves' own
  }
  __syncthreads();

  const int e0 = chunk * e_per_chunk;
  const int e1 = min(e_limit, e0 + e_per_chunk);
  const Word *cw = reinterpret_cast<const Word *>(codes);
  auto block_of = [&](int p, int r) { return rb_begin + p * mp.period + mp.lo + r; };
  // The chunk's row blocks are handed to the waves in RUNS through a counter in LDS, not dealt out in a fixed
  // stride.  The LDS arbiter serves older waves first, so with a fixed share each the sixteen waves of a workgroup
  // finished in four groups ~12 us apart (1.25 M-row shard, per-wave stamps: first wave 77 us, last 113 us), the
  // workgroup's slot -- 16 wave slots and 64 KiB of LDS, which the next workgroup needs all at once -- stayed
  // occupied by a thinning set of waves for a third of its life, and with both workgroups of a CU in that state the
  // gather pipe ran dry (53 % of the chip's wave slots active at the troughs).  Drawing runs, fast waves take more
  // blocks and all sixteen end within one run of each other.  The next run is drawn a whole run ahead (the result of
  // the ds_add_rtn is read four row blocks later), so the code word of the next block -- the next of this run or
  // the first of the next -- is still requested one block ahead.
  constexpr int RUN = 4;
  const int nruns = (e1 - e0 + RUN - 1) / RUN;
  // block list position e -> (period p, offset r) = (e / width, e % width), once per run: multiply-high by
  // floor((2^32 - 1) / width) + 1, exact for e < 2^32 / width
  const uint32_t magic = mp.width > 1 ? 0xFFFFFFFFu / (uint32_t)mp.width + 1u : 0u;
  auto locate = [&](int e, int &p, int &r) {
    p = mp.width > 1 ? (int)__umulhi((uint32_t)e, magic) : e;
    r = e - p * mp.width;
  };
  int *run_ctr = reinterpret_cast<int *>(qlds_raw + NQG * tab * QW / 16);   // = NW after the staging barrier
  int run = wave, e = e0 + run * RUN, e_run_end = min(e1, e + RUN);
  int mp_p = 0, mp_r = 0, grab_v = 0;
  Word w_first{};
  if (run < nruns) {
    locate(e, mp_p, mp_r);
    if (lane == 0) grab_v = atomicAdd(run_ctr, 1);
    w_first = cw[((size_t)block_of(mp_p, mp_r) * ng) * 64 + lane];
  }
  // PFX: a row block is first tested on PFX of its sixteen quantizers only -- the two sorted ones (15, 14: half-price
  // L1 look-ups, see above) and PFX - 2 from LDS.  Partial sums are <= full sums, so every (query, row) pair the full
  // test keeps has a row that passes for some query of the tile; at the bench's bounds a few percent of the rows do.
  // Such a lane appends its place in the sorted copy to the wave's ring in LDS (ballot + mbcnt, one ds_write_b32, the
  // fill level uniform; nothing leaves the wave), and whenever the ring holds 64 places every lane takes one, gathers
  // that row's code word (L2) and the wave runs the full sixteen look-ups, test and queueing below on them -- the
  // same code, `pos` instead of rb * 64 + lane; what is left at the end of the wave's last run goes through with the
  // idle lanes dead.  The stage's survivor set is the full test's, pair for pair.
  constexpr int RING = 128;      // places per wave: < 64 waiting + <= 64 appended
  int *ring = reinterpret_cast<int *>(qlds_raw + NQG * tab * QW / 16 + 1) + wave * RING;
  int fill = 0, head = 0;        // (uniform; places appended / taken so far)
  // Where the bounds separate little (rows without a tail of near ones: iid data) most rows pass, and the prefix test is
  // work on top of the full one: by the vector instructions alone (per block: 110 full test, 78 prefix test, 114 full
  // test of a ring) it pays while fewer than (110 - 78) / 114 = 0.28 of the rows pass.  A wave that has seen more than
  // a quarter of its rows pass, over eight blocks or more, empties its ring and takes its remaining blocks whole, as
  // without PFX.  (Per batch on the iid bench data: 2.63 ms without PFX, 4.13 with no switch, 2.92-2.95 with the switch
  // at a quarter or at an eighth -- what is left is every wave's eight probe blocks and this kernel's whole-block turns
  // against the kernel without PFX.  At an eighth waves of small ranges, whose bounds are looser, switch for nothing:
  // 1.25 M rows 0.396 ms against 0.38 at a quarter, 1 M rows 0.356 against 0.34.)
  int seen = 0;                  // blocks this wave has put through the prefix test
  bool direct = false;
  while (PFX ? (run < nruns || fill != head) : run < nruns) {
    int rb = 0, pos = 0;
    bool live = true;
    Word w{};
    const bool whole = PFX > 0 && direct && fill == head;    // this turn: one block, every lane its row (run < nruns here)
    bool more = PFX > 0 ? whole || (!direct && run < nruns && fill - head < 64) : true;
    while (more) {   // (without PFX, or `whole`: once)
      rb = block_of(mp_p, mp_r);
      // the block after this one
      int e_n = e + 1, p_n = mp_p, r_n = mp_r + 1, run_n = run, end_n = e_run_end;
      if (r_n == mp.width) { r_n = 0; p_n++; }
      if (e_n == e_run_end) {
        run_n = __builtin_amdgcn_readfirstlane(grab_v);
        if (run_n < nruns) {
          e_n = e0 + run_n * RUN;
          end_n = min(e1, e_n + RUN);
          locate(e_n, p_n, r_n);
          if (lane == 0) grab_v = atomicAdd(run_ctr, 1);
        }
      }
      w = w_first;
      // (unconditional: the last iteration re-reads its own block -- a conditional load costs a copy of the word back)
      w_first = cw[((size_t)(run_n < nruns ? block_of(p_n, r_n) : rb) * ng) * 64 + lane];
      run = run_n; e = e_n; e_run_end = end_n; mp_p = p_n; mp_r = r_n;
      pos = rb * 64 + lane;
      if constexpr (PFX > 0) if (!whole) {
        constexpr int PL1 = 2;                 // look-ups through the vector L1: the sorted quantizers 15 and 14
        static_assert(PFX == 0 || (SORTED && MAIN == 1 && GLB >= PL1 && PFX > PL1 && PFX - PL1 <= VEC - GLB && DW == 4 && NQG == 1),
                      "the prefix test is the key-sorted main stage's");
        constexpr int NL = PFX - PL1;          // look-ups from LDS: quantizers 0 .. NL - 1
        typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
        const uint8_t *tj_glb = qtab + (size_t)tile * tab * sizeof(QE);
        QE gl[PL1];
#pragma unroll
        for (int a = 0; a < PL1; a++)
          gl[a] = *reinterpret_cast<const QE *>(tj_glb + (size_t)(VEC - 1 - a) * 256 * sizeof(QE) +
                                                code_byte<VEC>(w, VEC - 1 - a) * (uint32_t)sizeof(QE));
        uint32_t pa[2 * DW];
#pragma unroll
        for (int x = 0; x < 2 * DW; x++) pa[x] = 0;
        // the PFX entries in NGRP byte-sum groups of even size (10: 3 + 3 + 4, not 4 + 4 + 2 -- a sum of three is one
        // three-operand add, and the widening is paid per group either way)
        constexpr int NGRP = (PFX + NADD - 1) / NADD;
#pragma unroll
        for (int gi = 0; gi < NGRP; gi++) {
          const int b = gi * PFX / NGRP, b_end = (gi + 1) * PFX / NGRP;
          uint32_t xs[DW];
#pragma unroll
          for (int dd = 0; dd < DW; dd++) xs[dd] = 0;
#pragma unroll
          for (int a = 0; a < NADD; a++) {     // bytes cannot carry: at most NADD entries, NADD * QMAX <= 255
            const int en = b + a;
            if (en >= b_end) continue;
            if (en < NL) {
              const u32x4 y = reinterpret_cast<const __attribute__((address_space(3))) u32x4 *>(0)[en * 256 + code_byte<VEC>(w, en)];
#pragma unroll
              for (int dd = 0; dd < DW; dd++) xs[dd] += y[dd];
            } else {
#pragma unroll
              for (int dd = 0; dd < DW; dd++) xs[dd] += reinterpret_cast<const uint32_t *>(&gl[en - NL])[dd];
            }
          }
#pragma unroll
          for (int dd = 0; dd < DW; dd++) {
            pa[2 * dd] += xs[dd];                                                // (unmasked: see `acc` below)
            pa[2 * dd + 1] += __builtin_amdgcn_perm(0u, xs[dd], 0x0C030C01u);   // bytes 1 and 3
          }
        }
        // A lane passes iff one of its sixteen sums is <= QMAX - 1: iff the smaller of the two per-half minima over the
        // eight accumulators is -- a minimum tree and ONE saturating subtraction instead of eight and an OR tree (the
        // same rows; 1.5 % of the step: profiles/r06/configs.md).  The subtraction W - 2^8 O stays a shift and a
        // subtraction: v_mad_i32_i24 (O, -256, W) is the same number mod 2^32 and cost 0.2 ms per step.
        uint32_t least = 0;
#pragma unroll
        for (int dd = 0; dd < DW; dd++) {
          pa[2 * dd] -= pa[2 * dd + 1] << 8;
          const uint32_t pair = pk_min_u16(pa[2 * dd], pa[2 * dd + 1]);
          least = dd == 0 ? pair : pk_min_u16(least, pair);
        }
        const uint32_t near = pk_sub_sat_u16(QMAXP, least);
        const unsigned long long mask = __ballot(near != 0);
        if (mask != 0ull) {
          const int before = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
          if (near != 0) ring[(fill + before) & (RING - 1)] = pos;
          fill += __popcll(mask);
        }
        seen++;
        direct = seen >= 8 && fill * 4 > seen * 64;
      }
      more = PFX > 0 && !whole && !direct && run < nruns && fill - head < 64;
    }
    if constexpr (PFX > 0) if (!whole) {
      // (one wave: its LDS accesses execute in order, the places written above are read back below)
      __builtin_amdgcn_wave_barrier();
      const int take = min(64, fill - head);
      if (take == 0) continue;              // an empty ring: the last run has ended, or the wave goes on block by block
      live = lane < take;
      pos = ring[(head + lane) & (RING - 1)];
      if (!live) pos = rb * 64 + lane;      // (an idle lane: any word of the copy)
      head += take;
      __builtin_amdgcn_wave_barrier();
      w = cw[pos];
    }
    const Word *p = cw + ((size_t)rb * ng) * 64 + lane;

    // acc[s][2*dd+1] : 16-bit sums of queries 4dd+1 (low half) and 4dd+3 (high half) of group s
    // acc[s][2*dd]   : queries 4dd and 4dd+2 -- after the words.  While the words are walked it is the plain 32-bit sum W
    //   of the byte-sum dwords: with S_i the sum of byte i, W = S0 + 2^8 S1 + 2^16 S2 + 2^24 S3 (mod 2^32) and the odd
    //   accumulator is O = S1 + 2^16 S3 exactly, so W - 2^8 O = S0 + 2^16 S2 (mod 2^32, and that is below 2^32: every
    //   S_i < 2^16) -- one subtraction per dword after the last word instead of a mask per dword and widening
    uint32_t acc[NQG][2 * DW];
#pragma unroll
    for (int s = 0; s < NQG; s++)
#pragma unroll
      for (int x = 0; x < 2 * DW; x++) acc[s][x] = 0;

    // one code word (VEC quantizers) of the row block; G0: the index has a single word per row (m <= 16), so the
    // table offsets are compile-time constants -- an LDS address is then one SDWA shift of the code byte (the entry's
    // quantizer rides in the instruction's offset field) instead of an extraction and a shift-add
    // (the word by value in, the next one out: a captured `w` that the body overwrites ended up in scratch memory for
    // every multi-word form -- 32 bytes per lane, the prefetched word waited for at once: m = 64 ran 13 % slower)
    auto word = [&](const int g, auto G0, const Word w) __attribute__((always_inline)) -> Word {
      Word wn = w;
      if (!decltype(G0)::value && g + 1 < ng) wn = p[(size_t)(g + 1) * 64];
      const QE *tj_lds = decltype(G0)::value ? qlds : qlds + g * VEC * 256;
      // the L1-served entries are the LAST GLB of the word, requested first: their latency passes under the
      // LDS gathers of the other entries (byte sums commute).  Uniform base (SGPR pair) + 32-bit lane offset: one
      // instruction per address instead of a 64-bit add chain
      const uint8_t *tj_glb = qtab + ((size_t)tile * NQG * tab + (decltype(G0)::value ? 0 : g * VEC * 256)) * sizeof(QE);
      QE gl[GLB > 0 ? GLB : 1][NQG];
#pragma unroll
      for (int a0 = 0; a0 < GLB; a0++)
#pragma unroll
        for (int s = 0; s < NQG; s++) {
          const int a = SORTED ? GLB - 1 - a0 : a0;   // the sorted quantizers (the word's last two) first
          const uint8_t *base = tj_glb + ((size_t)(VEC - GLB + a) * 256 + (size_t)s * tab) * sizeof(QE);
          const uint32_t off = code_byte<VEC>(w, VEC - GLB + a) * (uint32_t)sizeof(QE);
          gl[a][s] = *reinterpret_cast<const QE *>(base + off);
        }
#pragma unroll
      for (int b = 0; b < VEC; b += NADD) {
        uint32_t c[NADD];
#pragma unroll
        for (int a = 0; a < NADD; a++) c[a] = code_byte<VEC>(w, b + a);
#pragma unroll
        for (int s = 0; s < NQG; s++) {
          uint32_t xs[DW];
#pragma unroll
          for (int dd = 0; dd < DW; dd++) xs[dd] = 0;
#pragma unroll
          for (int a = 0; a < NADD; a++) {   // bytes cannot carry: NADD * QMAX <= 255
            const int e = b + a;
            if (e >= VEC - GLB) {
#pragma unroll
              for (int dd = 0; dd < DW; dd++) xs[dd] += reinterpret_cast<const uint32_t *>(&gl[e - (VEC - GLB)][s])[dd];
            } else if constexpr (decltype(G0)::value && QW == 16) {
              // the tables sit at LDS address 0 (the kernel has no static LDS; checked by the host at launch): with
              // a literal base the whole address is  (code byte << 4) + constant  -- one SDWA shift
              typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
              const u32x4 y = reinterpret_cast<const __attribute__((address_space(3))) u32x4 *>(0)[e * 256 + c[a] + s * tab];
#pragma unroll
              for (int dd = 0; dd < DW; dd++) xs[dd] += y[dd];
            } else {
              const QE y = tj_lds[e * 256 + c[a] + s * tab];
#pragma unroll
              for (int dd = 0; dd < DW; dd++) xs[dd] += reinterpret_cast<const uint32_t *>(&y)[dd];
            }
          }
#pragma unroll
          for (int dd = 0; dd < DW; dd++) {
            acc[s][2 * dd] += xs[dd];                                                // (unmasked: see `acc`)
            acc[s][2 * dd + 1] += __builtin_amdgcn_perm(0u, xs[dd], 0x0C030C01u);   // bytes 1 and 3
          }
        }
      }
      return wn;
    };
    // the same with the word's number a compile-time constant: table addresses are  (code byte << log2 entry size) +
    // literal, as in the one-word form (the tables sit at LDS address 0); taken where the index has exactly NGC words
    auto word_c = [&](auto gc, const Word w) __attribute__((always_inline)) -> Word {
      constexpr int g = decltype(gc)::value;
      Word wn = w;
      if (g + 1 < ng) wn = p[(size_t)(g + 1) * 64];
      typedef unsigned lvec __attribute__((ext_vector_type(DW)));
#pragma unroll
      for (int b = 0; b < VEC; b += NADD) {
        uint32_t c[NADD];
#pragma unroll
        for (int a = 0; a < NADD; a++) c[a] = code_byte<VEC>(w, b + a);
#pragma unroll
        for (int s = 0; s < NQG; s++) {
          uint32_t xs[DW];
#pragma unroll
          for (int dd = 0; dd < DW; dd++) xs[dd] = 0;
#pragma unroll
          for (int a = 0; a < NADD; a++) {   // bytes cannot carry: NADD * QMAX <= 255
            const int e = g * VEC + b + a;
            const lvec y = reinterpret_cast<const __attribute__((address_space(3))) lvec *>(0)[e * 256 + c[a] + s * tab];
#pragma unroll
            for (int dd = 0; dd < DW; dd++) xs[dd] += y[dd];
          }
#pragma unroll
          for (int dd = 0; dd < DW; dd++) {
            acc[s][2 * dd] += xs[dd];                                                // (unmasked: see `acc`)
            acc[s][2 * dd + 1] += __builtin_amdgcn_perm(0u, xs[dd], 0x0C030C01u);   // bytes 1 and 3
          }
        }
      }
      return wn;
    };
    if constexpr (NG1) (void)word(0, std::true_type{}, w);
#define WC(G) w = word_c(std::integral_constant<int, G>{}, w)
    // (the two forms measured: BASELINE config 5's m = 64 -- 15.16 -> 14.5 ms per batch -- and the reference CLI's default
    // m = 25 -- 0.759 -> 0.716 ms.  Unrolled for every word count the kernels grew to the 128-register limit, and the
    // m = 32 form (two 16-byte words, 16-byte entries) aborted; the others keep the loop.)
    else if (QW == 8 && VEC == 16 && ng == 4) { WC(0); WC(1); WC(2); WC(3); }
    else if (QW == 16 && VEC == 4 && ng == 7) { WC(0); WC(1); WC(2); WC(3); WC(4); WC(5); WC(6); }
#undef WC
    else
      for (int g = 0; g < ng; g++) w = word(g, std::false_type{}, w);

#pragma unroll
    for (int s = 0; s < NQG; s++)
#pragma unroll
      for (int dd = 0; dd < DW; dd++) acc[s][2 * dd] -= acc[s][2 * dd + 1] << 8;
    // conflict-ordered copy: which row a lane holds is only looked up (one byte) when a lane has something to report
    constexpr bool PERM = NG1 >= 2;
    int row = rb * 64 + lane;
    bool valid = PERM ? live : (row >= row_from && row < row_until);
    uint32_t any = 0;
    uint32_t left[NQG][2 * DW];
#pragma unroll
    for (int s = 0; s < NQG; s++)
#pragma unroll
      for (int x = 0; x < 2 * DW; x++) {
        left[s][x] = pk_sub_sat_u16(QMAXP, acc[s][x]);   // non-zero half <=> that query keeps this row
        any |= left[s][x];
      }
    if (__ballot(valid && any != 0) != 0ull) {
      // rare path.  Its queue addresses are uniform and loop-invariant, and hoisted out of the scan loop
      // they would hold ~60 SGPRs for the whole kernel -- past the 102 that still allow two workgroups per
      // CU.  Opaque copies keep that arithmetic in here.
      int *cnt_l = cnt, *queue_l = queue, *fb_l = const_cast<int *>(fb_tile);
      int slot_l = slot, tile_l = tile;
      asm volatile("" : "+s"(cnt_l), "+s"(queue_l), "+s"(slot_l), "+s"(tile_l), "+s"(fb_l));
      if (PERM) {
        const uint8_t *perm_l = perm;
        int pwin_l = pwin;
        asm volatile("" : "+s"(perm_l), "+s"(pwin_l));
        if constexpr (SORTED) row = reinterpret_cast<const int *>(perm_l)[PFX > 0 ? (size_t)pos : (size_t)rb * 64 + lane];   // (-1: padding)
        else row = (rb & ~pwin_l) * 64 + perm_l[(size_t)rb * 64 + lane];
        valid = live && row >= row_from && row < row_until;
      }
#pragma unroll
      for (int s = 0; s < NQG; s++)
#pragma unroll
        for (int x = 0; x < 2 * DW; x++) {
          const uint32_t l = valid ? left[s][x] : 0u;
          if (__ballot(l != 0) == 0ull) continue;
          const int q0 = (tile_l * NQG + s) * QW + 4 * (x >> 1) + (x & 1);
          // a full sub-queue means the bound separates nothing for this query: flag its tile at once, so that
          // the workgroups of the tile that have not started yet return immediately (the exact scan redoes it)
          enqueue_halves<NSLOT>(l, q0, slot_l, row, cnt_l, queue_l, cap, [&](int q) -> int & { return fb_l[q / qt]; });
        }
    }
  }
}

// ---- exact re-evaluation of the survivors; one workgroup (4 waves) per query -------------------
// Wave 0 continues the query's running (K+1)-list; waves 1-3 collect into empty lists but only
// what beats the running list's last entry; the four sorted lists are merged through LDS at the end.
constexpr int SV_WAVES = 4;
// One workgroup = the W queries that share a W-interleaved fp32 table (scan.hip build_tables), SV_WAVES waves each:
// the table (m_pad x 256 x W floats, 64 KiB at m = 16) is copied to LDS once, coalesced, and the sixteen look-ups of
// every survivor are LDS gathers.  (One workgroup per query gathering from the table in global memory sent 17
// scattered 64-byte requests per survivor through the texture path -- 4.4 M per batch -- which is also the path the
// main-stage kernel of the next batch serves three of its sixteen look-ups from.)
template <int VEC>
__global__ __launch_bounds__(64 * SV_WAVES * 4) void survivors_kernel(
    const uint8_t *__restrict__ codes, int ng, int m_pad, const float *__restrict__ tables, int W, int row_base,
    int *__restrict__ cnt, const int *__restrict__ queue, int cap, int B, int keff, float *__restrict__ fin_v,
    int *__restrict__ fin_i, int *__restrict__ fb_tile, int qt, int give_up /* survivors beyond which the filter is abandoned; 0: never */) {
  using Word = typename CodeWord<VEC>::type;
  extern __shared__ uint4 sv_lds_raw[];
  float *tlds = reinterpret_cast<float *>(sv_lds_raw);
  __shared__ unsigned long long mk[4][(SV_WAVES - 1) * 64];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave_wg = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qslot = wave_wg / SV_WAVES, wave = wave_wg - qslot * SV_WAVES;   // query of the group, wave of the query
  const int q = blockIdx.x * W + qslot;
  {
    const int n16 = m_pad * 256 * W / 4;      // 16-byte units (W * 256 floats per quantizer: a multiple of 4)
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 *src = reinterpret_cast<const u32x4 *>(tables) + (size_t)blockIdx.x * n16;
    u32x4 *dst = reinterpret_cast<u32x4 *>(sv_lds_raw);
    if (blockIdx.x * W < B)      // (read once: past the vector L1 the main-stage kernels gather from)
      for (int e = tid; e < n16; e += 64 * SV_WAVES * W) dst[e] = __builtin_nontemporal_load(src + e);
  }
  // sub-queue fill levels -> exclusive offsets of a flat numbering of this query's survivors
  SurvivorQueues<NSLOT> sq(cnt, q, lane);
  __syncthreads();                                  // every wave has read the counters; the table is in LDS
  sq.clear(wave == 0);
  bool active = q < B;                              // (uniform per query; no early return: barriers below)
  if (active && sq.overflowed(cap)) {
    if (wave == 0 && lane == 0) fb_tile[q / qt] = 1;   // a sub-queue overflowed: the exact scan redoes this query tile
    sq.clamp(cap);
  }
  int n = sq.count();
  if (active && give_up > 0 && n > give_up) {
    // the bound lets too many rows through for this query (data without a tail of near rows):
    // filtering the rest would cost more than it saves -- its tile goes to the exact scan
    if (wave == 0 && lane == 0) fb_tile[q / qt] = 1;
    active = false;
  }
  if (!active) n = 0;
  auto entry = [&](int e) { return sq.entry(queue, q, cap, e); };   // e-th survivor of the query, e < n

  // The running list and every candidate as ONE 64-bit key, (distance bits << 32) | row id: distances are sums of
  // squares (>= +0, or NaN, which sorts behind +inf and never enters), so the unsigned order of the key is the
  // (distance, row id) order of the lists.  A wave sorts the 64 candidates of a step with a bitonic network and merges
  // them into its running 64-list (the keff smallest are what counts): ~300 instructions per step.  (Feeding the
  // candidates one by one into a sorted register list -- ballot, readlane, shift, ~40 instructions each, every
  // candidate while a list fills up -- made this small kernel cost the batch 55 us next to another batch's main
  // stage, which leaves no vector-ALU slots to spare.)
  constexpr unsigned long long KEY_PAD = 0x7F8000007FFFFFFFull;      // (+inf, INT_MAX)
  auto make_key = [](float v, int r) { return ((unsigned long long)__float_as_uint(v) << 32) | (unsigned)r; };
  unsigned long long run = KEY_PAD;
  if (active && lane < keff) run = make_key(fin_v[(size_t)q * keff + lane], fin_i[(size_t)q * keff + lane]);
  const unsigned long long bound_key = shfl_u64(run, keff - 1);     // what a candidate has to beat
  if (wave != 0) run = KEY_PAD;                                      // wave 0 continues the list, the others start empty
  // W-interleaved fp32 tables (the group's copy in LDS): entry (j, c) of query q at (j * 256 + c) * W + q%W
  const float *tq = tlds + qslot;
  const Word *cw = reinterpret_cast<const Word *>(codes);
  // survivors e = (SV_WAVES * it + wave) * 64 + lane; two-deep software pipeline: row ids two
  // batches ahead, first code word one batch ahead
  constexpr int STEP = 64 * SV_WAVES;
  const int e0 = wave * 64 + lane;
  int row_n = e0 < n ? entry(e0) : 0;
  Word w_n = cw[((size_t)(row_n >> 6) * ng) * 64 + (row_n & 63)];
  int row_nn = e0 + STEP < n ? entry(e0 + STEP) : 0;
  unsigned long long admit = bound_key;                               // tightens to this wave's keff-th key
  for (int e = e0; e - lane < n; e += STEP) {
    const bool have = e < n;
    const int row = row_n;
    const Word w0 = w_n;
    row_n = row_nn;
    w_n = cw[((size_t)(row_n >> 6) * ng) * 64 + (row_n & 63)];
    row_nn = e + 2 * STEP < n ? entry(e + 2 * STEP) : 0;
    float d = 0.f;                      // the reference's order: j ascending, unfused fp32
    for (int g = 0; g < ng; g++) {
      const Word w = g == 0 ? w0 : cw[((size_t)(row >> 6) * ng + g) * 64 + (row & 63)];
      float t[VEC];
#pragma unroll
      for (int b = 0; b < VEC; b++) t[b] = tq[((size_t)(g * VEC + b) * 256 + code_byte<VEC>(w, b)) * W];
#pragma unroll
      for (int b = 0; b < VEC; b++) d += t[b];
    }
    unsigned long long key = make_key(d, row + row_base);
    if (!(have && key < admit)) key = KEY_PAD;
    if (__ballot(key != KEY_PAD) == 0ull) continue;
    run = merge64_u64(run, sort64_u64(key, lane), lane);
    admit = shfl_u64(run, keff - 1);
    if (admit > bound_key) admit = bound_key;
  }
  if (wave > 0) mk[qslot][(wave - 1) * 64 + lane] = run;
  __syncthreads();
  if (wave == 0 && active) {
#pragma unroll 1
    for (int w2 = 0; w2 < SV_WAVES - 1; w2++) run = merge64_u64(run, mk[qslot][w2 * 64 + lane], lane);
    if (lane < keff) {
      fin_v[(size_t)q * keff + lane] = __uint_as_float((unsigned)(run >> 32));
      fin_i[(size_t)q * keff + lane] = (int)(unsigned)run;
    }
  }
}

template <int QW, int NQG, int VEC, int NADD>
void launch_filter_t(gulon_index *ix, int ftiles, int nchunks, int rb_begin, int e_count, int e_per_chunk, RbMap mp,
                     int from, int until, int cap, int stage, int B, hipStream_t st, int *fb, int qt, bool sorted,
                     int prefix) {
  const int W_fp32 = ix->w;
  size_t lds_bytes = (size_t)NQG * ix->m_pad * 256 * QW + 16;   // tables + the run counter
  // (the single-word form only for the instantiation the headline index runs on: m = 16, two workgroups per CU)
  constexpr bool one_word_form = QW == 16 && NQG == 1 && VEC == 16 && NADD == 4;
  // stage: 0 a short stage, 1 the main stage (a tag of its own for the profilers), 2 the tie replay's long level
  // (per-tile row limits behind the flags)
#define GULON_FILTER_PICK(NG1_) \
  (stage == 1 ? filter_kernel<QW, NQG, VEC, NADD, 1, NG1_> : stage == 2 ? filter_kernel<QW, NQG, VEC, NADD, 2, NG1_> \
                                                                         : filter_kernel<QW, NQG, VEC, NADD, 0, NG1_>)
  // the one-word form and the WC(...) forms address the tables from LDS offset 0: no kernel this launch can pick may
  // have static LDS (checked once per instantiation)
  static const bool lds_at_zero = [] {
    for (int stage = 0; stage < 3; stage++)
      for (auto k : {GULON_FILTER_PICK(0), GULON_FILTER_PICK(one_word_form), GULON_FILTER_PICK(2 * one_word_form)}) {
        hipFuncAttributes fa;
        HIP_CHECK(hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(k)));
        if (fa.sharedSizeBytes != 0) return false;
      }
    if constexpr (one_word_form)
      for (auto k : {filter_kernel<QW, NQG, VEC, NADD, 0, 3>, filter_kernel<QW, NQG, VEC, NADD, 1, 3>}) {
        hipFuncAttributes fa;
        HIP_CHECK(hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(k)));
        if (fa.sharedSizeBytes != 0) return false;
      }
    return true;
  }();
  GULON_REQUIRE(lds_at_zero, "internal: the filter kernels address their tables from LDS offset 0");
  auto kern = GULON_FILTER_PICK(0);
  const uint8_t *codes = ix->codes.p, *perm = nullptr;
  if (one_word_form && ix->ng == 1) {
    kern = GULON_FILTER_PICK(one_word_form);
    if (ix->fcodes.p && tuning_of(ix).filter_order > 0) {   // the conflict-ordered copy of the codes (conflict_order.hip)
      kern = GULON_FILTER_PICK(2 * one_word_form);
      codes = ix->fcodes.p;
      perm = ix->fperm.p;
    }
  }
  if (sorted) {   // the key-sorted copy: the whole-index launches of the short and the main stage
    GULON_REQUIRE(one_word_form && ix->ng == 1 && ix->scodes.p && ix->sids.p && stage != 2,
                  "internal: no key-sorted form of this filter launch");
    if constexpr (one_word_form) {
      kern = stage == 1 ? filter_kernel<QW, NQG, VEC, NADD, 1, 3> : filter_kernel<QW, NQG, VEC, NADD, 0, 3>;
      codes = ix->scodes.p;
      perm = reinterpret_cast<const uint8_t *>(ix->sids.p);
      if (stage == 1 && prefix > 0) {
        // the main stage with the prefix test: a ring of 128 places per wave behind the run counter.  Taken where two
        // such workgroups fit a CU, as without the rings (2 x 72 KiB of 160; asked once per device) and the kernel has
        // no static LDS (tables at offset 0); elsewhere the launch stays the form without the prefix
        const auto pkern = filter_kernel<QW, NQG, VEC, NADD, 1, 3, FILTER_PREFIX_P>;
        const size_t plds = lds_bytes + (size_t)(FILTER_THREADS / 64) * 128 * sizeof(int);
        constexpr int MAX_DEV = 64;
        static std::atomic<int> fits[MAX_DEV];   // per device -- 0: not asked yet, 1: two resident, -1: not
        int dev = 0;
        HIP_CHECK(hipGetDevice(&dev));
        GULON_REQUIRE(dev >= 0 && dev < MAX_DEV, "device ordinal %d out of range", dev);
        int f = fits[dev].load(std::memory_order_relaxed);
        if (f == 0) {
          const void *k = reinterpret_cast<const void *>(pkern);
          int nb = 0;
          hipFuncAttributes fa;
          HIP_CHECK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plds));
          HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k, FILTER_THREADS, plds));
          HIP_CHECK(hipFuncGetAttributes(&fa, k));
          f = fa.sharedSizeBytes == 0 && nb >= 2 ? 1 : -1;
          fits[dev].store(f, std::memory_order_relaxed);
        }
        if (f > 0) {
          kern = pkern;
          lds_bytes = plds;
        }
      }
    }
  }
  HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds_bytes));
  hipLaunchKernelGGL(kern, stage == 2 ? dim3(nchunks, ftiles) : dim3(ftiles, nchunks), dim3(FILTER_THREADS), lds_bytes, st, codes, perm, ix->ng, ix->m_pad,
                     ix->qtab.p, from, until, rb_begin, e_count, e_per_chunk, mp, ix->sv_cnt.p, ix->sv_queue.p, cap,
                     fb ? fb : ix->fb_tile.p, fb ? qt : W_fp32 * ix->nsub, B, sorted ? 3 : perm ? ix->fwindow - 1 : 0);
  HIP_CHECK(hipGetLastError());
}

// The filter kernel owns the LDS of every CU, so two of them (query batches in flight on
// different streams) cannot usefully overlap -- they would only time-slice and blur each other's
// duration.  Launches are therefore chained through one event per device: a batch's small,
// latency-bound kernels overlap with another batch's filter, the filters themselves run in turn.
struct FilterLane {   // per device: completion of the most recent main-stage launch (created on first use, never destroyed)
  static constexpr int MAX_DEVICES = 64;
  std::atomic<hipEvent_t> ev[MAX_DEVICES];
  FilterLane() { for (auto &e : ev) e.store(nullptr, std::memory_order_relaxed); }
  // the device's event; `fresh` = this call created it (nothing to wait for yet).  Lock-free after the first launch
  // on a device: the launch path of every batch of every index goes through here.
  hipEvent_t of(int dev, bool &fresh) {
    fresh = false;
    GULON_REQUIRE(dev >= 0 && dev < MAX_DEVICES, "device ordinal %d out of range", dev);
    hipEvent_t e = ev[dev].load(std::memory_order_acquire);
    if (e) return e;
    hipEvent_t mine = nullptr;
    HIP_CHECK(hipEventCreateWithFlags(&mine, hipEventDisableTiming));
    if (ev[dev].compare_exchange_strong(e, mine, std::memory_order_acq_rel)) { fresh = true; return mine; }
    (void)hipEventDestroy(mine);            // another thread was first
    return e;
  }
};
FilterLane &filter_lane() { static FilterLane l; return l; }

// queries per quantized table entry: as many as LDS holds for one group (16 up to m_pad = 36,
// 8 up to 72, 4 up to 144) ...
int filter_qw(const gulon_index *ix) {
  int qw = 16;
  while (qw > 4 && (size_t)ix->m_pad * 256 * qw > FILTER_LDS_BUDGET) qw /= 2;
  return qw;
}
// ... and how many such groups a workgroup takes: two only if two workgroups of that size still
// fit a CU's 160 KiB -- two resident workgroups hide each other's table staging and barriers
// (measured at m = 16: 3.18 -> 3.01 ms for the main stage against one workgroup with two groups)
int filter_nqg(const gulon_index *ix) {
  return (size_t)ix->m_pad * 256 * filter_qw(ix) * 4 <= 160 * 1024 ? 2 : 1;
}

}  // namespace

hipEvent_t filter_lane_event(int dev, bool &fresh) { return filter_lane().of(dev, fresh); }


int device_cus() {
  static std::atomic<int> cus[FilterLane::MAX_DEVICES];
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  GULON_REQUIRE(dev >= 0 && dev < FilterLane::MAX_DEVICES, "device ordinal %d out of range", dev);
  int n = cus[dev].load(std::memory_order_relaxed);
  if (n == 0) {
    HIP_CHECK(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
    n = std::max(1, n);
    cus[dev].store(n, std::memory_order_relaxed);
  }
  return n;
}

FilterShape filter_shape(const gulon_index *ix) {
  const ScanTuning &t = tuning_of(ix);
  FilterShape f;
  f.qw = filter_qw(ix);
  f.nqg = filter_nqg(ix);
  // 4 (6-bit levels) is cheapest, but the bound's slack grows with m / levels, so wide indexes take 2 (7-bit levels)
  // unless told otherwise
  f.nadd = t.filter_nadd ? t.filter_nadd : (ix->m_pad <= 16 ? 4 : 2);
  f.qmax = 255 / f.nadd;
  f.cap = std::max(64, t.filter_cap / NSLOT);
  const size_t filter_lds = (size_t)f.nqg * ix->m_pad * 256 * f.qw;
  const int resident = std::max(1, std::min(2048 / FILTER_THREADS, (int)(160 * 1024 / filter_lds)));
  f.slots = device_cus() * resident;
  return f;
}

// The filter launches of an index whose ordered code copy spans windows of several blocks (conflict_order.hip) cover
// whole windows: a row of [from, until) may sit in any block of its window.  Rows outside the range that come along are
// rejected one by one where a lane reports a survivor.  Returns the first block and the number of blocks to scan.
void filter_block_range(const gulon_index *ix, int qw, int nqg, int nadd, int from, int until, int &rb_begin,
                        int &rb_total) {
  rb_begin = from / 64;
  int rb_end = ceil_div(until, 64);
  const bool ordered = ix->fcodes.p && ix->ng == 1 && ix->vec == 16 && qw == 16 && nqg == 1 && nadd == 4 &&
                       tuning_of(ix).filter_order > 0;
  if (ordered && ix->fwindow > 1) {
    const int w = ix->fwindow;
    rb_begin -= rb_begin % w;
    rb_end = std::min(ceil_div(ix->n, 64), ceil_div(rb_end, w) * w);
  }
  rb_total = rb_end - rb_begin;
}

bool filter_eligible(const gulon_index *ix, int K, int rb_total) {
  const ScanTuning &t = tuning_of(ix);
  return t.filter && !ix->wide && K >= 1 && K <= GULON_MAX_K && (size_t)ix->m_pad * 256 * 4 <= FILTER_LDS_BUDGET &&
         rb_total >= t.filter_min_rb && rb_total >= t.filter_period;
}

// sample size ~ sqrt(rows): the sample scan costs ~1.4 us per 1000 rows, the first filter
// stage's slow path ~ rows / sample -- 54 K rows at 10 M, 19 K at 1.25 M; filter_sample caps it
int filter_sample_rows(const ScanTuning &t, int rb_total) {
  return std::max(4096, std::min(t.filter_sample, (int)(17.0 * std::sqrt((double)rb_total * 64.0))));
}

// ONE launch: the batch's counters, Index.prepareQuery for all queries (with the table minima of the B real
// queries; the padding queries of the last 16-query quantisation group are dead and never read theirs) and the
// bounds from a strided sample of about filter_sample rows, which also resets the running lists
void launch_bound_tables(gulon_index *ix, const float *dQ, int B, int Bp, int Bq, int ntiles, int keff, int from,
                         int until, int rb_begin, int rb_total, float *bounds_out, hipStream_t st) {
  const ScanTuning &t = tuning_of(ix);
  const int W = ix->w, NW = t.threads / 64;
  const int sblocks = std::max(NW, std::min(rb_total, ceil_div(filter_sample_rows(t, rb_total), 64)));
  const RbMap smap{std::max(1, rb_total / sblocks), 0, 1};
  const int se = rbmap_count(rb_total, smap);
  const size_t lds_bytes = std::max((size_t)ix->m_pad * 256 * 4 * W, (size_t)W * NW * 64 * 4);
  // the sample scan is a pure gather of 16-byte fp32 entries: it reads the conflict-ordered copy where there is one
  const bool ordered = ix->fcodes.p && ix->ng == 1 && ix->vec == 16 && t.filter_order > 0;
  const uint8_t *scodes = ordered ? ix->fcodes.p : ix->codes.p, *sperm = ordered ? ix->fperm.p : nullptr;
  auto go = [&](auto kern, int W_) {
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds_bytes));
    hipLaunchKernelGGL(kern, dim3(Bp / W_), dim3(BOUND_THREADS), lds_bytes, st, ix->cents.p, ix->from.p, ix->sdim.p,
                       ix->d, ix->m, ix->k, dQ, ix->tables.p, ix->qmins.p, scodes, sperm, ordered ? ix->fwindow - 1 : 0,
                       ix->ng, ix->m_pad, from, until, rb_begin, se, smap, B, keff, ix->tau0.p, ix->fin_v.p, ix->fin_i.p,
                       bounds_out, ix->gtau.p, Bp, ix->fb_tile.p, ntiles, ix->sv_cnt.p, Bq * NSLOT);
  };
  if (ix->vec == 16) { if (W == 4) go(bound_tables<16, 4>, 4); else if (W == 2) go(bound_tables<16, 2>, 2); else go(bound_tables<16, 1>, 1); }
  else               { if (W == 4) go(bound_tables<4, 4>, 4); else if (W == 2) go(bound_tables<4, 2>, 2); else go(bound_tables<4, 1>, 1); }
  HIP_CHECK(hipGetLastError());
}

void launch_shared_tau(gulon_index *ix, const float *all_bounds, int lists, int B, int keff, hipStream_t st) {
  hipLaunchKernelGGL(shared_tau, dim3(ceil_div(B, 4)), dim3(256), 0, st, all_bounds, lists, B, keff, ix->tau0.p);
  HIP_CHECK(hipGetLastError());
}

void launch_qt_quantize(gulon_index *ix, const float *tables, int W, int Bp, int B, int Bq, const float *mins,
                        const float *fin_v, const int *fin_i, const float *tau0, int keff, int qmax, int qw, int *fb,
                        int qt, const int *slot, hipStream_t st) {
  hipLaunchKernelGGL(qt_quantize, dim3(Bq / 4, ix->m_pad), dim3(256), 0, st, tables, W, Bp, ix->m_pad, ix->k, B, mins,
                     fin_v, fin_i, tau0, keff, qmax, qw, ix->qtab.p, fb, qt, slot);
  HIP_CHECK(hipGetLastError());
}

void launch_filter(gulon_index *ix, int qw, int nqg, int nadd, int ftiles, int nchunks, int rb_begin, int e_count,
                   int e_per_chunk, RbMap mp, int from, int until, int cap, int stage, int B, hipStream_t st, int *fb,
                   int qt, bool sorted, int prefix) {
#define GO(W_, Q, V, A) \
  launch_filter_t<W_, Q, V, A>(ix, ftiles, nchunks, rb_begin, e_count, e_per_chunk, mp, from, until, cap, stage, B, st, fb, qt, sorted, prefix)
#define GO_QV(W_, Q, V) do { if (nadd == 4) GO(W_, Q, V, 4); else GO(W_, Q, V, 2); } while (0)
#define GO_W(W_) do {                                                  \
    if (ix->vec == 16) { if (nqg == 2) GO_QV(W_, 2, 16); else GO_QV(W_, 1, 16); } \
    else               { if (nqg == 2) GO_QV(W_, 2, 4); else GO_QV(W_, 1, 4); }   \
  } while (0)
  if (qw == 16) GO_W(16); else if (qw == 8) GO_W(8); else GO_W(4);
#undef GO_W
#undef GO_QV
#undef GO
}

void launch_survivors(gulon_index *ix, int B, int Bq, int keff, int cap, int give_up, hipStream_t st) {
  const int W = ix->w;
  const size_t sv_lds = (size_t)ix->m_pad * 256 * W * sizeof(float);
  auto kern = ix->vec == 16 ? survivors_kernel<16> : survivors_kernel<4>;
  HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sv_lds));
  hipLaunchKernelGGL(kern, dim3(Bq / W), dim3(64 * SV_WAVES * W), sv_lds, st, ix->codes.p, ix->ng, ix->m_pad, ix->tables.p,
                     W, ix->row_base, ix->sv_cnt.p, ix->sv_queue.p, cap, B, keff, ix->fin_v.p, ix->fin_i.p,
                     ix->fb_tile.p, W * ix->nsub, give_up);
  HIP_CHECK(hipGetLastError());
}

}  // namespace gulon
