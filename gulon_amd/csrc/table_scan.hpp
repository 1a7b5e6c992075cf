// The flat table scan: what the offset queries (offset.hip), the rank queries (rank.hip) and the flat
// 3CosMul scan (cosmul.hip) have in common.  A workgroup of TABLE_SCAN_THREADS holds E Index.prepareQuery tables
// [E][m_pad][256] in LDS (stage_tables) and its waves walk the 64-row code blocks of a row chunk, lane = row, one running
// sum per table (table_scan_rows); what becomes of the E sums of a row -- a key into a WaveList, a counter -- is the
// caller's, and so is what the tables' LDS holds after the walk.
#pragma once
#include "scan.hpp"

namespace gulon {

constexpr int TABLE_SCAN_THREADS = 1024;                 // the workgroup: 16 waves, one row block each per step
constexpr size_t TABLE_LDS_BUDGET = 144 * 1024;          // the LDS the tables of one workgroup may take
constexpr size_t FLAT_TABLE_BYTES = size_t(256) << 20;   // the tables of one pass of a flat form
constexpr int EXACT_SUB_BATCH = 4096;                    // queries per pass of an exact form: bounds its chunk lists

#ifdef __HIPCC__
__device__ __forceinline__ bool finite_key(float t) { return fabsf(t) < INFINITY; }   // false for NaN

// `live` tables of `tab` floats from `tables` to lds4, as float4 with every thread of the workgroup striding, the slots
// from `live` up to `slots` filled with zeros (slots = live: none); then the barrier that lets every wave read them.
__device__ __forceinline__ void stage_tables(float4 *lds4, const float *__restrict__ tables, int tab, int live, int slots,
                                             int tid) {
  const float4 *src = reinterpret_cast<const float4 *>(tables);
  const int n4 = live * (tab / 4), all4 = slots * (tab / 4);
  for (int e = tid; e < all4; e += TABLE_SCAN_THREADS) lds4[e] = e < n4 ? src[e] : make_float4(0.f, 0.f, 0.f, 0.f);
  __syncthreads();
}

// The row blocks rb0 + wave, rb0 + wave + 16, ... < rb1 of a chunk against the E tables at `lds`, `tab` floats apart:
// per row acc[t] += T_t[j][code_j] with j ascending from 0.f, as scan.hip's exact scan adds them, then sink(rb, acc).
// The order of the additions is the parity contract with the reference's ADC sum; four codes per step keep 4 * E
// look-ups in flight and E = 8 free of scratch.  Any E from 1 to 8.
template <int E, int VEC, class Sink>
__device__ __forceinline__ void table_scan_rows(const uint8_t *__restrict__ codes, int ng, int tab, const float *lds,
                                                int rb0, int rb1, int lane, int wave, Sink sink) {
  using Word = typename CodeWord<VEC>::type;
  const Word *cw = reinterpret_cast<const Word *>(codes);
  for (int rb = rb0 + wave; rb < rb1; rb += TABLE_SCAN_THREADS / 64) {
    float acc[E];
#pragma unroll
    for (int t = 0; t < E; t++) acc[t] = 0.f;
    const Word *p = cw + ((size_t)rb * ng) * 64 + lane;
    for (int g = 0; g < ng; g++) {
      const Word w = p[(size_t)g * 64];
      const float *tj = lds + g * VEC * 256;
#pragma unroll 1
      for (int seg = 0; seg < VEC / 4; seg++) {
        const uint32_t x = code_word32<VEC>(w, seg);
#pragma unroll
        for (int bb = 0; bb < 4; bb++) {
          const float *te = tj + (seg * 4 + bb) * 256 + ((x >> (8 * bb)) & 0xFFu);
#pragma unroll
          for (int t = 0; t < E; t++) acc[t] += te[t * tab];
        }
      }
    }
    sink(rb, acc);
  }
}
#endif

// E in {8, 4, 2, 1} (anything else: 1) and vec in {4, 16} (anything else: 16) as compile-time constants:
// f(std::integral_constant<int, E>, std::integral_constant<int, VEC>).
template <class F>
void dispatch_e_vec(int E, int vec, F f) {
  auto with_e = [&](auto e) {
    if (vec == 4) f(e, std::integral_constant<int, 4>{});
    else f(e, std::integral_constant<int, 16>{});
  };
  switch (E) {
    case 8: with_e(std::integral_constant<int, 8>{}); break;
    case 4: with_e(std::integral_constant<int, 4>{}); break;
    case 2: with_e(std::integral_constant<int, 2>{}); break;
    default: with_e(std::integral_constant<int, 1>{}); break;
  }
}

}  // namespace gulon
