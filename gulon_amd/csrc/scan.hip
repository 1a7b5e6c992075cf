// ADC scan path: Index.prepareQuery -> PQIndex.distances -> TopKHeap -> Result.fromHeap
// (Index.scala:352-440, TopKHeap.scala, Index.scala:83-94), re-designed for gfx950.
//
// The table build, the scan kernels, the driver of a flat query (run_query) and the query entry points; the handle
// itself is index_handle.hip, the merge of the scan's partial lists merge.hip.
//
// Kernels
//   build_tables     per-query m x 256 distance tables, 4 queries interleaved (float4)
//   scan_kernel      tables in LDS (ds_read_b128 = 4 queries per lookup), codes streamed
//                    coalesced, j-ordered fp32 sums, wavefront-register top-k
#include "scan.hpp"

namespace gulon {

// ---------------------------------------------------------------------------
// Index.prepareQuery (Index.scala:352-383): T[q][j][c] = sum_t (q[from_j+t]-c[t])^2,
// sequential, unfused.  INTERLEAVED: written as [q/4][j_pad][256][q%4] for the scan;
// otherwise as the reference's [B][m][k].
// ---------------------------------------------------------------------------
template <bool INTERLEAVED, int W>
__global__ void build_tables(const float *__restrict__ cents, const int *__restrict__ from,
                             const int *__restrict__ sdim, int d, int m, int k, int m_pad,
                             const float *__restrict__ Q, int B, float *__restrict__ T,
                             const int *__restrict__ live_queries, float *__restrict__ mins) {
  // one thread per (query group of W, quantizer, centroid); a block of 256 threads = the 256
  // centroids of ONE (query group, quantizer), so the per-(query, quantizer) table minimum the
  // quantized filter needs (NaN entries ignored) is a block reduction here (mins != nullptr)
  // (launched with 256 threads: quantizer and query group are block-uniform, so the query values
  // come through scalar loads; the centroid coordinates are fetched eight at a time)
  if (live_queries) B = min(B, *live_queries);   // device-side query count (tie replay: usually 0)
  const int nqg = (B + W - 1) / W;
  if ((long long)blockIdx.x >= (long long)nqg * m_pad) return;
  const int c = threadIdx.x;
  const int j = blockIdx.x % m_pad;
  const int qg = blockIdx.x / m_pad;
  const long long t = (long long)blockIdx.x * 256 + c;
  float acc[W];
#pragma unroll
  for (int u = 0; u < W; u++) acc[u] = 0.f;
  if (j < m && c < k) {
    const int fr = from[j], s = sdim[j];
    const float *cc = cents + (size_t)k * fr + (size_t)c * s;
    for (int t0 = 0; t0 < s; t0 += 8) {
      float cv[8];
#pragma unroll
      for (int e = 0; e < 8; e++) cv[e] = t0 + e < s ? cc[t0 + e] : 0.f;
#pragma unroll
      for (int e = 0; e < 8; e++) {
        if (t0 + e < s) {
#pragma unroll
          for (int u = 0; u < W; u++) {
            const int q = qg * W + u;
            if (q < B) {
              const float dd = Q[(size_t)q * d + fr + t0 + e] - cv[e];
              acc[u] += dd * dd;
            }
          }
        }
      }
    }
  }
  if (INTERLEAVED && mins != nullptr) {
    __shared__ unsigned smin[W];
    if (threadIdx.x < W) smin[threadIdx.x] = 0x7F800000u;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < W; u++) {
      float x = (c < k && acc[u] == acc[u]) ? acc[u] : INFINITY;   // entries beyond k are not real table entries
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) x = fminf(x, __shfl_xor(x, o));
      if ((threadIdx.x & 63) == 0) atomicMin(&smin[u], __float_as_uint(x));   // entries are >= +0: uint order
    }
    __syncthreads();
    if (threadIdx.x < W) mins[(size_t)(qg * W + threadIdx.x) * m_pad + j] = __uint_as_float(smin[threadIdx.x]);
  }
  if (INTERLEAVED) {
#pragma unroll
    for (int u = 0; u < W; u++) T[(size_t)t * W + u] = acc[u];
  } else if (j < m && c < k) {
#pragma unroll
    for (int u = 0; u < W; u++) {
      int q = qg * W + u;
      if (q < B) T[((size_t)q * m + j) * k + c] = acc[u];
    }
  }
}

// ---------------------------------------------------------------------------
// The scan.  One workgroup = QT = 4*NSUB queries x one chunk of row blocks.
// LDS holds NSUB interleaved tables ([j][c] -> float4 of 4 queries); lane = row;
// every (row, quantizer) costs one ds_read_b128 per sub-table and 4 adds.
// ---------------------------------------------------------------------------
// W queries are interleaved per table entry: W = 4 -> ds_read_b128, 2 -> b64, 1 -> b32.
template <int W> struct TabVec;
template <> struct TabVec<4> { using type = float4; };
template <> struct TabVec<2> { using type = float2; };
template <> struct TabVec<1> { using type = float; };

template <int W, int NSUB, int VEC, int THREADS, bool PRUNE>
__device__ __forceinline__ void scan_body(
    const uint8_t *__restrict__ codes, int ng, int m_pad, const float4 *__restrict__ tables,
    int row_from, int row_until, int row_base, int rb_begin, int e_count, int e_per_chunk, RbMap mp, int nchunks,
    int keff, float *__restrict__ part_v, int *__restrict__ part_i, unsigned *__restrict__ gtau, int tau_off4,
    int prune_from, const float *__restrict__ lbv, const int *__restrict__ lbi,
    const uint8_t *__restrict__ perm /* non-null: `codes` is the conflict-ordered copy (conflict_order.hip), perm its row order */,
    const int tile /* query tile of this pass */) {
  constexpr int QT = W * NSUB;
  constexpr int NW = THREADS / 64;
  using Word = typename CodeWord<VEC>::type;
  using TV = typename TabVec<W>::type;
  extern __shared__ float4 lds_raw[];
  const TV *lds = reinterpret_cast<const TV *>(lds_raw);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int chunk = blockIdx.y;
  const int tab_entries = m_pad * 256;  // entries (of W floats) per sub-table

  // Shared pruning thresholds, as the bits of non-negative floats (so unsigned min == float
  // min): tau_sh[q] >= the (K+1)-th smallest distance of query q over everything scanned so
  // far by ANY wave of ANY workgroup (gtau is the cross-workgroup copy).  A row whose
  // distance exceeds it can never be in the final top-(K+1), so it is dropped before the
  // (expensive, wave-serial) insertion.  Only speed depends on how fresh these values are.
  unsigned *tau_sh = reinterpret_cast<unsigned *>(lds_raw + tau_off4);
  if (tid < QT) tau_sh[tid] = __hip_atomic_load(&gtau[tile * QT + tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);

  // stage the NSUB sub-tables of this query tile
  {
    const int n16 = NSUB * tab_entries * W / 4;   // float4 units
    const float4 *src = tables + (size_t)tile * n16;
    for (int e = tid; e < n16; e += THREADS) lds_raw[e] = src[e];
  }
  __syncthreads();

  WaveList wl[QT];
  int cnt[QT];
#pragma unroll
  for (int q = 0; q < QT; q++) { wl[q].init(); cnt[q] = 0; }

  // large-K "peeling" rounds: only entries strictly after (lbq, lbiq) in (distance, row id)
  // order are eligible (the earlier ones were returned by previous rounds)
  const bool peel = lbv != nullptr;
  float lbq[QT];
  int lbiq[QT];
#pragma unroll
  for (int q = 0; q < QT; q++) {
    lbq[q] = peel ? lbv[tile * QT + q] : -1.f;
    lbiq[q] = peel ? lbi[tile * QT + q] : -1;
  }

  // this chunk's share of the eligible row blocks, in e-space (RbMap); (mp_p, mp_r) tracks
  // e = mp_p * width + mp_r without a division per row block
  const int e0 = chunk * e_per_chunk;
  const int e1 = min(e_count, e0 + e_per_chunk);
  const Word *cw = reinterpret_cast<const Word *>(codes);
  int mp_p = (e0 + wave) / mp.width, mp_r = (e0 + wave) - mp_p * mp.width;
  auto block_of = [&](int p, int r) { return rb_begin + p * mp.period + mp.lo + r; };
  auto advance = [&](int &p, int &r) { r += NW; while (r >= mp.width) { r -= mp.width; p++; } };

  // software pipeline: the first code word of the NEXT row block is in flight while this
  // one is being looked up (global latency would otherwise idle the LDS pipe)
  Word w_first{};
  if (e0 + wave < e1) w_first = cw[((size_t)block_of(mp_p, mp_r) * ng) * 64 + lane];
  for (int e = e0 + wave; e < e1; e += NW) {
    const int rb = block_of(mp_p, mp_r);
    advance(mp_p, mp_r);
    float acc[QT];
#pragma unroll
    for (int q = 0; q < QT; q++) acc[q] = 0.f;

    const Word *p = cw + ((size_t)rb * ng) * 64 + lane;
    Word w = w_first;
    if (e + NW < e1) w_first = cw[((size_t)block_of(mp_p, mp_r) * ng) * 64 + lane];

    // workgroup-shared thresholds (wave-uniform LDS reads); <= keeps exact-tie candidates
    float tsh[QT];
#pragma unroll
    for (int q = 0; q < QT; q++)
      tsh[q] = __uint_as_float(__hip_atomic_load(&tau_sh[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));

    // Exact early termination.  Every table entry is a sum of squares (>= 0) and binary32
    // addition of a non-negative term is monotone, so a j-ordered PARTIAL sum is a lower
    // bound of the full distance.  Once all 64 rows x 4 queries of a sub-table are already
    // above their thresholds, none of them can enter a top-(K+1) list and the remaining
    // look-ups of that sub-table are skipped; rows that survive still get bit-exact sums.
    bool live[NSUB];
#pragma unroll
    for (int s = 0; s < NSUB; s++) live[s] = true;

    for (int g = 0; g < ng; g++) {
      Word wn = w;
      if (g + 1 < ng) wn = p[(size_t)(g + 1) * 64];
      const TV *tj = lds + g * VEC * 256;
#pragma unroll
      for (int seg = 0; seg < VEC / 4; seg++) {
        if (PRUNE && g * VEC + seg * 4 >= prune_from) {
#pragma unroll
          for (int s = 0; s < NSUB; s++)
            if (live[s]) {
              bool in = false;
#pragma unroll
              for (int u = 0; u < W; u++) in = in || acc[W * s + u] <= tsh[W * s + u];
              live[s] = __ballot(in) != 0ull;
            }
        }
#pragma unroll
        for (int s = 0; s < NSUB; s++) {
          if (!PRUNE || live[s]) {
#pragma unroll
            for (int bb = 0; bb < 4; bb++) {
              const int b = seg * 4 + bb;
              uint32_t c = code_byte<VEC>(w, b);
              TV t = tj[b * 256 + c + s * tab_entries];
              const float *tf = reinterpret_cast<const float *>(&t);
#pragma unroll
              for (int u = 0; u < W; u++) acc[W * s + u] += tf[u];
            }
          }
        }
      }
      w = wn;
    }

    const int row = rb * 64 + lane;
    // (ordered copy: which row a lane holds is looked up only when some lane has a candidate)
    const bool valid = perm != nullptr || (row >= row_from && row < row_until);
    unsigned long long masks[QT];
    unsigned long long any = 0;
#pragma unroll
    for (int q = 0; q < QT; q++) {
      unsigned long long mk = (!PRUNE || live[q / W]) ? __ballot(valid && acc[q] <= tsh[q]) : 0ull;
      masks[q] = mk;
      any |= mk;
    }
    if (any) {
      int place = lane;
      unsigned long long in_range = ~0ull;
      if (perm) {
        place = perm[(size_t)rb * 64 + lane];
        const int prow = rb * 64 + place;
        in_range = __ballot(prow >= row_from && prow < row_until);
      }
#pragma unroll
      for (int q = 0; q < QT; q++) {
        unsigned long long mk = masks[q] & in_range;
        while (mk) {
          int l = __ffsll((long long)mk) - 1;
          mk &= mk - 1;
          float cv = readlane_f(acc[q], l);
          int cr = rb * 64 + readlane_i(place, l) + row_base;
          if (peel && !(cv > lbq[q] || (cv == lbq[q] && cr > lbiq[q]))) continue;
          if (cnt[q] < keff || wl[q].accepts(cv, cr)) {
            wl[q].insert(cv, cr, keff, lane);
            if (cnt[q] < keff) cnt[q]++;
            if (wl[q].tau < tsh[q]) {   // this wave's list is full and tighter: publish
              tsh[q] = wl[q].tau;
              if (lane == 0)
                __hip_atomic_fetch_min(&tau_sh[q], __float_as_uint(wl[q].tau), __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_WORKGROUP);
            }
          }
        }
      }
    }
    // every 32 row blocks one wave trades thresholds with the other workgroups of this tile
    if (wave == 0 && (((e - e0) / NW) & 31) == 31 && lane < QT) {
      unsigned mine = __hip_atomic_load(&tau_sh[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      unsigned old = __hip_atomic_fetch_min(&gtau[tile * QT + lane], mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (old < mine)
        __hip_atomic_fetch_min(&tau_sh[lane], old, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
  }

  // merge the NW per-wave lists of every query through LDS (tables are dead now)
  __syncthreads();
  float *sv = reinterpret_cast<float *>(lds_raw);
  int *si = reinterpret_cast<int *>(sv + QT * NW * 64);
  merge_wave_lists<QT, NW>(wl, sv, si, keff, lane, wave, [&](int q, const WaveList &out) {
    if (lane < keff) {
      size_t o = ((size_t)(tile * QT + q) * nchunks + chunk) * keff + lane;
      part_v[o] = out.v;
      part_i[o] = out.i;
    }
    if (lane == 0 && out.tau < INFINITY)
      __hip_atomic_fetch_min(&gtau[tile * QT + q], __float_as_uint(out.tau), __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
  });
}

#define GULON_SCAN_PARAMS                                                                                          \
  const uint8_t *__restrict__ codes, int ng, int m_pad, const float4 *__restrict__ tables, int row_from,           \
      int row_until, int row_base, int rb_begin, int e_count, int e_per_chunk, RbMap mp, int nchunks, int keff,     \
      float *__restrict__ part_v, int *__restrict__ part_i, unsigned *__restrict__ gtau, int tau_off4,              \
      int prune_from, const float *__restrict__ lbv, const int *__restrict__ lbi, const uint8_t *__restrict__ perm
#define GULON_SCAN_ARGS                                                                                            \
  codes, ng, m_pad, tables, row_from, row_until, row_base, rb_begin, e_count, e_per_chunk, mp, nchunks, keff,      \
      part_v, part_i, gtau, tau_off4, prune_from, lbv, lbi, perm

// workgroup (x, y) = query tile x (fastest: the tiles of one chunk run together) x chunk y of the row blocks
template <int W, int NSUB, int VEC, int THREADS, bool PRUNE>
__global__ __launch_bounds__(THREADS) void scan_kernel(GULON_SCAN_PARAMS) {
  scan_body<W, NSUB, VEC, THREADS, PRUNE>(GULON_SCAN_ARGS, (int)blockIdx.x);
}

// The filter's fallback launch: only the query tiles flagged in tile_enable (one flag per tile_div tiles) are
// scanned, normally none.  It sits on the critical path of its batch while ANOTHER batch's filter kernel
// fills the chip, and a workgroup is dispatched only where a leaving filter workgroup makes room: 64 KiB of
// LDS and, per SIMD, 4 x 56 + 64 = 288 registers.  Four waves of the regular one-sub-table instantiation
// (84 VGPRs) need 352 and waited for a completely empty CU -- for the other batch's whole 3 ms kernel --, so
// this twin is compiled for 7 waves per SIMD (<= 72 VGPRs); and since even then every workgroup waits for
// its turn (256 empty workgroups: 0.9 ms on average), the launch is `gridDim.x` workgroups wide, each
// looping over the tiles x, x + gridDim.x, ...: narrow while nothing falls back, wide once something did
// (*hint, host-mapped, read by the host when it sizes the next launch).
template <int W, int NSUB, int VEC, int THREADS, bool PRUNE>
__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(7))) void scan_kernel_lean(
    GULON_SCAN_PARAMS, const int *__restrict__ tile_enable, int tile_div, int ntiles, int *__restrict__ hint) {
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    if (tile_enable[tile / tile_div] == 0) continue;
    if (hint && threadIdx.x == 0 && blockIdx.y == 0) *hint = 1;
    scan_body<W, NSUB, VEC, THREADS, PRUNE>(GULON_SCAN_ARGS, tile);
    __syncthreads();   // every wave is done with this tile's tables and thresholds in LDS
  }
}
#undef GULON_SCAN_PARAMS
#undef GULON_SCAN_ARGS

void launch_build_tables(int W, gulon_index *ix, const float *dQ, int B, int Bpad, float *tables, hipStream_t st,
                         const int *live_queries, float *mins) {
  long long total = (long long)(Bpad / W) * ix->m_pad * 256;
  if (total <= 0) return;
#define BT(WW)                                                                                             \
  hipLaunchKernelGGL((build_tables<true, WW>), dim3(ceil_div(total, 256)), dim3(256), 0, st, ix->cents.p,   \
                     ix->from.p, ix->sdim.p, ix->d, ix->m, ix->k, ix->m_pad, dQ, B, tables, live_queries, mins)
  if (W == 4) BT(4); else if (W == 2) BT(2); else BT(1);
#undef BT
  HIP_CHECK(hipGetLastError());
}

bool replay_enabled() {
  static const bool on = [] { const char *e = getenv("GULON_TIE_REPLAY"); return !(e && atoi(e) == 0); }();
  return on;
}

QueryOut merge_outputs(const FlatCall &c) {
  QueryOut out = c.out;
  if (out.final_out() && replay_enabled() && out.flags == nullptr) {
    c.ix->flags_scratch.ensure((size_t)c.B);
    out.flags = c.ix->flags_scratch.p;
  }
  return out;
}

void finish_replay(const FlatCall &c, int *flags, bool literal_pass) {
  if (!(c.out.final_out() && replay_enabled())) return;
  // queries with exact distance ties: replay the reference heap's insertion history
  run_tie_replay(c, flags);
  // queries whose distances can be NaN / +inf: the literal heap over all rows (TopKHeap.scala:69-79)
  if (literal_pass) run_nonfinite_literal(c, c.out.flags);
}

void finish_query(const FlatCall &c, const float *in_v, const int *in_i, int lists, long long stride_l,
                  long long stride_q, bool literal_pass) {
  const QueryOut out = merge_outputs(c);
  launch_merge(in_v, in_i, lists, stride_l, stride_q, c.B, c.K, out, c.st);
  finish_replay(c, out.flags, literal_pass);
}

}  // namespace gulon

using namespace gulon;

namespace {

template <int W, int NSUB, int VEC, int SCAN_THREADS, bool PRUNE>
void launch_scan_p(gulon_index *ix, int ntiles, int nchunks, int rb_begin, int e_count, int e_per_chunk, RbMap mp,
                   int from, int until, int keff, hipStream_t st, const float *lbv, const int *lbi,
                   const int *tile_enable, int tile_div, int grid_x, int *hint) {
  size_t lds_bytes = (size_t)NSUB * ix->m_pad * 256 * W * sizeof(float);
  size_t merge_bytes = (size_t)W * NSUB * (SCAN_THREADS / 64) * 64 * 8;
  if (merge_bytes > lds_bytes) lds_bytes = merge_bytes;
  const int tau_off4 = (int)(lds_bytes / sizeof(float4));   // shared thresholds live after tables/merge area
  lds_bytes += 64;
  int prune_from = tuning_of(ix).prune_from >= 0 ? tuning_of(ix).prune_from : ix->m_pad / 2;
  if (prune_from < 4) prune_from = 4;
  if (tile_enable) {   // the filter's fallback (launch_scan with one_sub): grid_x workgroups loop over the tiles
    if constexpr (NSUB == 1) {
      auto kern = scan_kernel_lean<W, NSUB, VEC, SCAN_THREADS, PRUNE>;
      HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds_bytes));
      hipLaunchKernelGGL(kern, dim3(std::max(1, std::min(grid_x, ntiles)), nchunks), dim3(SCAN_THREADS), lds_bytes, st,
                         ix->codes.p, ix->ng, ix->m_pad, reinterpret_cast<const float4 *>(ix->tables.p), from, until,
                         ix->row_base, rb_begin, e_count, e_per_chunk, mp, nchunks, keff, ix->part_v.p, ix->part_i.p,
                         ix->gtau.p, tau_off4, prune_from, lbv, lbi, (const uint8_t *)nullptr, tile_enable, tile_div, ntiles, hint);
      HIP_CHECK(hipGetLastError());
      return;
    } else {
      GULON_REQUIRE(false, "internal: tile-enabled scans use one sub-table");
    }
  }
  auto kern = scan_kernel<W, NSUB, VEC, SCAN_THREADS, PRUNE>;
  HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds_bytes));
  // one-word codes: the exact scan's table gathers are the same ds_read_b128 of 256 x 16-byte entries per quantizer as
  // the filter's, so the conflict-ordered copy serves it too (13 of its 16 quantizers were ordered for)
  // (the exact scan walks row blocks one at a time: it reads the ordered copy only where a block holds its own rows)
  const bool ordered = VEC == 16 && ix->ng == 1 && ix->fcodes.p && ix->fwindow == 1 && tuning_of(ix).filter_order > 0;
  hipLaunchKernelGGL(kern, dim3(ntiles, nchunks), dim3(SCAN_THREADS), lds_bytes, st, ordered ? ix->fcodes.p : ix->codes.p,
                     ix->ng, ix->m_pad,
                     reinterpret_cast<const float4 *>(ix->tables.p), from, until, ix->row_base, rb_begin, e_count,
                     e_per_chunk, mp, nchunks, keff, ix->part_v.p, ix->part_i.p, ix->gtau.p, tau_off4, prune_from, lbv,
                     lbi, ordered ? ix->fperm.p : (const uint8_t *)nullptr);
  HIP_CHECK(hipGetLastError());

}

template <int W, int NSUB, int VEC>
void launch_scan_t(gulon_index *ix, int ntiles, int nchunks, int rb_begin, int e_count, int e_per_chunk, RbMap mp,
                   int from, int until, int keff, hipStream_t st, const float *lbv, const int *lbi,
                   const int *tile_enable, int tile_div, int grid_x, int *hint) {
  constexpr int TH = 1024;
  if (tuning_of(ix).prune)
    launch_scan_p<W, NSUB, VEC, TH, true>(ix, ntiles, nchunks, rb_begin, e_count, e_per_chunk, mp, from, until, keff,
                                          st, lbv, lbi, tile_enable, tile_div, grid_x, hint);
  else
    launch_scan_p<W, NSUB, VEC, TH, false>(ix, ntiles, nchunks, rb_begin, e_count, e_per_chunk, mp, from, until, keff,
                                           st, lbv, lbi, tile_enable, tile_div, grid_x, hint);
}

}  // namespace

namespace gulon {
void launch_scan(gulon_index *ix, int ntiles, int nchunks, int rb_begin, int e_count, int e_per_chunk, RbMap mp,
                 int from, int until, int keff, hipStream_t st, const float *lbv, const int *lbi,
                 const int *tile_enable, bool one_sub, int grid_x, int *hint) {
  // tile_enable (the filter's fallback) comes with one_sub: W-query tiles (one sub-table, <= 64 KiB of LDS)
  // whatever the index prefers; ntiles counts THOSE tiles, tile_enable keeps one flag per ix->nsub of them,
  // and grid_x workgroups per chunk loop over them
  GULON_REQUIRE((tile_enable != nullptr) == one_sub, "internal: tile_enable <=> one_sub");
  const int nsub = one_sub ? 1 : ix->nsub;
  const int tile_div = one_sub ? ix->nsub : 1;
#define GO(WW, NS, V)                                                                                          \
  launch_scan_t<WW, NS, V>(ix, ntiles, nchunks, rb_begin, e_count, e_per_chunk, mp, from, until, keff, st, lbv, lbi, \
                           tile_enable, tile_div, grid_x, hint)
  if (ix->w == 4) {
    if (ix->vec == 16) {
      if (nsub == 4) GO(4, 4, 16); else if (nsub == 2) GO(4, 2, 16); else GO(4, 1, 16);
    } else {
      if (nsub == 4) GO(4, 4, 4); else if (nsub == 2) GO(4, 2, 4); else GO(4, 1, 4);
    }
  } else if (ix->w == 2) {
    if (ix->vec == 16) GO(2, 1, 16); else GO(2, 1, 4);
  } else {
    if (ix->vec == 16) GO(1, 1, 16); else GO(1, 1, 4);
  }
#undef GO
}
}  // namespace gulon

namespace {

__global__ void fill_f32(float *__restrict__ p, long long n, float v) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}
void launch_fill_f32(float *p, long long n, float v, hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(fill_f32, dim3((unsigned)ceil_div(n, 256LL)), dim3(256), 0, st, p, n, v);
  HIP_CHECK(hipGetLastError());
}

// ---- run_query: table build + scan + merge of one batch, in the order of its checks ----

void validate(const FlatCall &c) {
  GULON_REQUIRE(c.from <= c.until, "expected: from <= until");                                  // Index.scala:418
  GULON_REQUIRE(c.from >= 0 && c.until <= c.ix->n, "expected: from >= 0 && until <= length");   // Index.scala:419
  GULON_REQUIRE(c.K >= 0 && c.B >= 0, "k and batch size must be non-negative");
  GULON_UNSUPPORTED(c.K > GULON_MAX_K_PEELED, "k_nn = %d > %d is not supported", c.K, GULON_MAX_K_PEELED);
  GULON_UNSUPPORTED(c.K + 1 > GULON_MAX_K_PEELED && !c.out.final_out(), "k_nn = %d: a shard returns k_nn + 1 <= %d entries",
                    c.K, GULON_MAX_K_PEELED);
}

int row_blocks(const FlatCall &c) { return ceil_div(c.until, 64) - c.from / 64; }

// first half of a query with shared bounds: ranges the filter does not take have no bounds to offer (+inf).  Returns
// whether that was the whole call.
bool bounds_only_unfiltered(const FlatCall &c) {
  if (!(c.sb && c.sb->phase == 1)) return false;
  const int rbt = row_blocks(c);
  if (c.K >= 1 && rbt > 0 && filter_eligible(c.ix, c.K, rbt)) return false;
  launch_fill_f32(c.sb->bounds_out, (long long)c.B * (c.K + 1), INFINITY, c.st);
  return true;
}

// empty heaps (no neighbours asked for, or no row block in the range): nothing to scan.  Final lists of (-1, +inf) with
// zero counts and flags; partial lists of K + 1 entries of (+inf, INT_MAX), also where a peeled round would be 64 long.
// Every output is written where the caller gave one, on the call's stream.
bool empty_result(const FlatCall &c) {
  if (!(c.K == 0 || row_blocks(c) <= 0)) return false;
  const QueryOut &o = c.out;
  if (o.idx && c.K > 0) {
    HIP_CHECK(hipMemsetAsync(o.idx, 0xFF, sizeof(int) * (size_t)c.B * c.K, c.st));
    launch_fill_f32(o.dist, (long long)c.B * c.K, INFINITY, c.st);
  }
  if (o.count) HIP_CHECK(hipMemsetAsync(o.count, 0, sizeof(int) * (size_t)c.B, c.st));
  if (o.flags) HIP_CHECK(hipMemsetAsync(o.flags, 0, sizeof(int) * (size_t)c.B, c.st));
  if (o.part_v) launch_fill_list(o.part_v, o.part_i, (long long)c.B * (c.K + 1), c.st);
  return true;
}

// what the byte-coded scans share: the padded batch, and the chunks of a launch of ~target_blocks workgroups
struct ScanShape {
  int W, QT, ntiles, Bp, rb_begin, rb_total, nchunks, rb_per_chunk;
  explicit ScanShape(const FlatCall &c)
      : W(c.ix->w), QT(W * c.ix->nsub), ntiles(ceil_div(c.B, QT)), Bp(ntiles * QT), rb_begin(c.from / 64),
        rb_total(row_blocks(c)) {
    const ScanTuning &t = tuning_of(c.ix);
    scan_chunks(rb_total, ceil_div(t.target_blocks, ntiles), t.threads / 64, nchunks, rb_per_chunk);
  }
};
const RbMap ALL_BLOCKS{1, 0, 1};

// K > GULON_MAX_K: the result comes 64 entries per scan round (PeelRounds, merge.hip); no tie replay
void run_peeled_query(const FlatCall &c) {
  gulon_index *ix = c.ix;
  const ScanShape s(c);
  launch_build_tables(s.W, ix, c.dQ, c.B, s.Bp, (ix->tables.ensure((size_t)s.Bp * ix->m_pad * 256), ix->tables.p), c.st);
  ix->part_v.ensure((size_t)s.Bp * s.nchunks * 64);
  ix->part_i.ensure((size_t)s.Bp * s.nchunks * 64);
  ix->gtau.ensure((size_t)s.Bp);
  PeelRounds peel(ix, c.B, s.Bp, c.B, c.K, c.st);
  for (int r = 0; r < peel.rounds; r++) {
    HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)ix->gtau.p, 0x7F800000 /* +inf */, (size_t)s.Bp, c.st));
    launch_scan(ix, s.ntiles, s.nchunks, s.rb_begin, s.rb_total, s.rb_per_chunk, ALL_BLOCKS, c.from, c.until, 64, c.st,
                peel.bounds(0).v, peel.bounds(0).i);
    peel.append(r, 0, c.B, s.nchunks);
  }
  peel.finish(c.out);
}

void run_plain_query(const FlatCall &c) {
  gulon_index *ix = c.ix;
  const ScanShape s(c);
  const int keff = c.K + 1;
  ix->tables.ensure((size_t)s.Bp * ix->m_pad * 256);
  ix->part_v.ensure((size_t)s.Bp * s.nchunks * keff);
  ix->part_i.ensure((size_t)s.Bp * s.nchunks * keff);
  ix->gtau.ensure((size_t)s.Bp);
  HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)ix->gtau.p, 0x7F800000 /* +inf */, (size_t)s.Bp, c.st));

  launch_build_tables(s.W, ix, c.dQ, c.B, s.Bp, ix->tables.p, c.st);
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (ix->profile) {
    e0 = ix->take_event();
    e1 = ix->take_event();
    HIP_CHECK(hipEventRecord(e0, c.st));
  }
  launch_scan(ix, s.ntiles, s.nchunks, s.rb_begin, s.rb_total, s.rb_per_chunk, ALL_BLOCKS, c.from, c.until, keff, c.st);
  if (ix->profile) {
    HIP_CHECK(hipEventRecord(e1, c.st));
    ix->events.emplace_back(e0, e1);
    ix->prof_rows += c.until - c.from;
  }
  finish_query(c, ix->part_v.p, ix->part_i.p, s.nchunks, (long long)keff, (long long)s.nchunks * keff, true);
}

void run_query(const FlatCall &c) {
  validate(c);
  if (c.B == 0) return;
  if (!c.sb || c.sb->phase != 2) c.ix->last_filter_tiles = 0;
  if (bounds_only_unfiltered(c)) return;
  if (empty_result(c)) return;
  const bool peeled = c.K > GULON_MAX_K;
  if (c.ix->wide) run_wide_query(c);
  else if (!peeled && filter_eligible(c.ix, c.K, row_blocks(c))) run_filter_query(c);
  else if (peeled) run_peeled_query(c);
  else run_plain_query(c);
}

}  // namespace

namespace gulon {
void batch_query_dev_on(gulon_index *idx, const float *d_queries, int32_t b, int32_t k_nn, int32_t from, int32_t until,
                        int32_t *d_out_idx, float *d_out_dist, int32_t *d_out_count, int32_t *d_out_flags,
                        hipStream_t st, bool map_view) {
  std::lock_guard<std::mutex> lock(idx->mu);
  idx->pend_b = -1;
  StreamOrder so(idx, st);
  run_query({idx, d_queries, b, k_nn, from, until,
             QueryOut::final_lists(d_out_idx, d_out_dist, d_out_count, d_out_flags), st, nullptr});
  if (map_view) launch_map_rows(idx, d_out_idx, (long long)b * k_nn, st);
  so.done();
}
}  // namespace gulon

GULON_API int32_t gulon_index_batch_query_dev(gulon_index *idx, const float *d_queries, int32_t b, int32_t k_nn,
                                              int32_t from, int32_t until, int32_t *d_out_idx, float *d_out_dist,
                                              int32_t *d_out_count, int32_t *d_out_flags, void *stream) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    batch_query_dev_on(idx, d_queries, b, k_nn, from, until, d_out_idx, d_out_dist, d_out_count, d_out_flags,
                       (hipStream_t)stream, false);
  });
}

GULON_API int32_t gulon_index_scan_partial_dev(gulon_index *idx, const float *d_queries, int32_t b, int32_t k_nn,
                                               int32_t from, int32_t until, float *d_part_dist, int32_t *d_part_idx,
                                               void *stream) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    std::lock_guard<std::mutex> lock(idx->mu);
    idx->pend_b = -1;
    StreamOrder so(idx, (hipStream_t)stream);
    run_query({idx, d_queries, b, k_nn, from, until, QueryOut::partial_lists(d_part_dist, d_part_idx),
               (hipStream_t)stream, nullptr});
    so.done();
  });
}

GULON_API int32_t gulon_index_scan_bounds_dev(gulon_index *idx, const float *d_queries, int32_t b, int32_t k_nn,
                                              int32_t from, int32_t until, float *d_bounds, void *stream) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr && d_bounds != nullptr, "null argument");
    GULON_UNSUPPORTED(k_nn > GULON_MAX_K, "k_nn = %d > GULON_MAX_K = %d is only supported for unsharded queries", k_nn,
                      GULON_MAX_K);
    std::lock_guard<std::mutex> lock(idx->mu);
    const SharedBounds sb{1, d_bounds, nullptr, 0};
    idx->pend_b = -1;
    StreamOrder so(idx, (hipStream_t)stream);
    run_query({idx, d_queries, b, k_nn, from, until, QueryOut{}, (hipStream_t)stream, &sb});   // no outputs but sb's
    so.done();
    idx->pend_b = b; idx->pend_k = k_nn; idx->pend_from = from; idx->pend_until = until;
  });
}

GULON_API int32_t gulon_index_scan_partial_bounded_dev(gulon_index *idx, const float *d_queries, int32_t b,
                                                       int32_t k_nn, int32_t from, int32_t until,
                                                       const float *d_all_bounds, int32_t lists, float *d_part_dist,
                                                       int32_t *d_part_idx, void *stream) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr && d_all_bounds != nullptr && lists >= 1, "bad arguments");
    std::lock_guard<std::mutex> lock(idx->mu);
    GULON_REQUIRE(idx->pend_b == b && idx->pend_k == k_nn && idx->pend_from == from && idx->pend_until == until,
                  "scan_partial_bounded must follow scan_bounds on the same index with the same arguments");
    idx->pend_b = -1;
    const SharedBounds sb{2, nullptr, d_all_bounds, lists};
    StreamOrder so(idx, (hipStream_t)stream);
    run_query({idx, d_queries, b, k_nn, from, until, QueryOut::partial_lists(d_part_dist, d_part_idx),
               (hipStream_t)stream, &sb});
    so.done();
  });
}

namespace {
// A host-pointer query.  stage(c, st) puts the b queries into c->stage_q on the workspace's stream.
template <class Stage>
void host_query(gulon_index *idx, int32_t b, int32_t k_nn, int32_t from, int32_t until, int32_t *out_idx,
                float *out_dist, int32_t *out_count, int32_t *out_flags, bool map_view, Stage stage) {
  GULON_REQUIRE(b >= 0 && k_nn >= 0, "k and batch size must be non-negative");
  // concurrent callers (Tests.scala:109-122 queries from a thread pool) each get a workspace of their own
  gulon_index *c = acquire_host_context(idx);
  struct Release { gulon_index *i, *c; ~Release() { release_host_context(i, c); } } rel{idx, c};
  std::lock_guard<std::mutex> lock(c->mu);
  c->pend_b = -1;
  size_t bk = (size_t)b * (size_t)k_nn;
  c->stage_q.ensure((size_t)b * c->d + 1);
  c->stage_oi.ensure(bk + 1);
  c->stage_od.ensure(bk + 1);
  c->stage_oc.ensure((size_t)b + 1);
  c->stage_of.ensure((size_t)b + 1);
  if (!c->host_stream) HIP_CHECK(hipStreamCreateWithFlags(&c->host_stream, hipStreamNonBlocking));
  hipStream_t st = c->host_stream;
  StreamOrder so(c, st);
  stage(c, st);
  run_query({c, c->stage_q.p, b, k_nn, from, until,
             QueryOut::final_lists(c->stage_oi.p, c->stage_od.p, c->stage_oc.p, c->stage_of.p), st, nullptr});
  if (map_view) launch_map_rows(c, c->stage_oi.p, (long long)bk, st);   // the context borrows the view's map
  if (bk) {
    c->stage_oi.download(out_idx, bk, st);
    c->stage_od.download(out_dist, bk, st);
  }
  if (b > 0 && out_count) c->stage_oc.download(out_count, b, st);
  if (b > 0 && out_flags) c->stage_of.download(out_flags, b, st);
  so.done();
  HIP_CHECK(hipStreamSynchronize(st));
}
}  // namespace

namespace gulon {
void batch_query_host_on(gulon_index *idx, const float *queries, int32_t b, int32_t k_nn, int32_t from, int32_t until,
                         int32_t *out_idx, float *out_dist, int32_t *out_count, int32_t *out_flags, bool map_view) {
  host_query(idx, b, k_nn, from, until, out_idx, out_dist, out_count, out_flags, map_view,
             [&](gulon_index *c, hipStream_t st) {
    if (b > 0) HIP_CHECK(hipMemcpyAsync(c->stage_q.p, queries, sizeof(float) * (size_t)b * c->d, hipMemcpyHostToDevice, st));
  });
}
}  // namespace gulon

GULON_API int32_t gulon_index_batch_query(gulon_index *idx, const float *queries, int32_t b, int32_t k_nn,
                                          int32_t from, int32_t until, int32_t *out_idx, float *out_dist,
                                          int32_t *out_count, int32_t *out_flags) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    batch_query_host_on(idx, queries, b, k_nn, from, until, out_idx, out_dist, out_count, out_flags, false);
  });
}

GULON_API int32_t gulon_prepare_query(const float *cents, int32_t d, int32_t m, int32_t k, const float *queries,
                                      int32_t b, float *t_out) {
  return guarded([&] {
    GULON_REQUIRE(d >= 1 && m >= 1 && m <= d && k >= 1 && b >= 0, "bad shape");
    if (b == 0) return;
    std::vector<int> from, until, sdim(m);
    subvectors(d, m, from, until);
    for (int j = 0; j < m; j++) sdim[j] = until[j] - from[j];
    DevBuf<int> dfrom, dsd; DevBuf<float> dc, dq, dt((size_t)b * m * k);
    dfrom.upload(from.data(), m); dsd.upload(sdim.data(), m);
    dc.upload(cents, (size_t)k * d); dq.upload(queries, (size_t)b * d);
    if (k > 256) {
      launch_build_tables_wide(dc.p, dfrom.p, dsd.p, d, m, k, dq.p, 0, b, dt.p, nullptr);
      dt.download(t_out, (size_t)b * m * k);
      HIP_CHECK(hipDeviceSynchronize());
      return;
    }
    long long total = (long long)((b + 3) / 4) * m * 256;
    hipLaunchKernelGGL((build_tables<false, 4>), dim3(ceil_div(total, 256)), dim3(256), 0, 0, dc.p, dfrom.p, dsd.p, d, m, k,
                       m, dq.p, b, dt.p, (const int *)nullptr, (float *)nullptr);
    HIP_CHECK(hipGetLastError());
    dt.download(t_out, (size_t)b * m * k);
    HIP_CHECK(hipDeviceSynchronize());
  });
}

// ---- query by stored rows (Index.queryByWord, Index.scala:38-45, with SortedIndex.lookup, Index.scala:318-319):
// decode the rows on the device (decode.hip), optionally MathUtils.normalize them (SortedIndex.prepare for a
// normalized metric, Index.scala:324-331), then the batch query of gulon_index_batch_query, all on one stream.  The
// decoded queries live in the handle's (or host context's) stage_q.
GULON_API int32_t gulon_index_query_rows_dev(gulon_index *idx, const int32_t *d_rows, int32_t b, int32_t k_nn,
                                             int32_t normalize, int32_t from, int32_t until, int32_t *d_out_idx,
                                             float *d_out_dist, int32_t *d_out_count, int32_t *d_out_flags,
                                             void *stream) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    GULON_REQUIRE(b >= 0 && k_nn >= 0, "k and batch size must be non-negative");
    std::lock_guard<std::mutex> lock(idx->mu);
    idx->pend_b = -1;
    const hipStream_t st = (hipStream_t)stream;
    StreamOrder so(idx, st);
    ensure_row_err(idx);
    idx->stage_q.ensure((size_t)b * idx->d + 1);
    launch_decode_rows(idx, d_rows, b, nullptr, nullptr, 0, normalize != 0, idx->stage_q.p, idx->row_err.p, st);
    run_query({idx, idx->stage_q.p, b, k_nn, from, until,
               QueryOut::final_lists(d_out_idx, d_out_dist, d_out_count, d_out_flags), st, nullptr});
    so.done();
  });
}

GULON_API int32_t gulon_index_query_rows(gulon_index *idx, const int32_t *rows, int32_t b, int32_t k_nn,
                                         int32_t normalize, int32_t from, int32_t until, int32_t *out_idx,
                                         float *out_dist, int32_t *out_count, int32_t *out_flags) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    GULON_REQUIRE(b >= 0 && k_nn >= 0, "k and batch size must be non-negative");
    GULON_REQUIRE(b == 0 || rows != nullptr, "rows is null");
    for (int r = 0; r < b; r++)   // checked before anything is launched
      GULON_REQUIRE(rows[r] >= 0 && rows[r] < idx->n, "row %d = %d outside [0, %d)", r, rows[r], idx->n);
    host_query(idx, b, k_nn, from, until, out_idx, out_dist, out_count, out_flags, false,
               [&](gulon_index *c, hipStream_t st) {
      c->stage_rows.ensure((size_t)b + 1);
      if (b == 0) return;
      HIP_CHECK(hipMemcpyAsync(c->stage_rows.p, rows, sizeof(int32_t) * (size_t)b, hipMemcpyHostToDevice, st));
      launch_decode_rows(c, c->stage_rows.p, b, nullptr, nullptr, 0, normalize != 0, c->stage_q.p, nullptr, st);
    });
  });
}
