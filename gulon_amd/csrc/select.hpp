// What the query-path filters (filter.hip, wide_filter.hip, grouped_filter.hip, the selection kernels of grouped.hip)
// share: ordered keys, the block radix select, the packed saturating subtract, the wave sum, the 64-lane bitonic
// networks and the survivor sub-queues.  One copy of each; device code only, but for the test hooks'
// read-back of the sub-queues at the end.
#pragma once

#include "common.hpp"

namespace gulon {

// ---- float <-> unsigned key whose unsigned order is the float order (-0 < +0; NaNs at the two ends) ----
__device__ __forceinline__ unsigned ordered_key(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ordered_float(unsigned t) {
  return __uint_as_float((t & 0x80000000u) ? (t & 0x7FFFFFFFu) : ~t);
}

__device__ inline uint32_t pk_sub_sat_u16(uint32_t a, uint32_t b) {   // per 16-bit half: max(a - b, 0)
  uint32_t d;
  asm("v_pk_sub_u16 %0, %1, %2 clamp" : "=v"(d) : "v"(a), "v"(b));
  return d;
}

// The sum over a wavefront, in every lane.  The base |q|^2 - 2 q.g of the grouped index's approximate distance D~ is
// made of such sums, and the by-group filter's lists equal gq_approx_scan's only while both add in THIS order.
__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

// ---- block radix select ---------------------------------------------------------------------------------------------
struct RadixSelectState {
  unsigned prefix, remaining;   // the key bytes fixed so far; the rank wanted among the keys that share them
};

// The key of the `want`-th smallest of the workgroup's keys: four counting passes over the key bytes, high to low.
// Eight sub-counters per bin (keys that share their high bytes would serialise their atomics on one or two LDS words),
// the bins walked by a prefix sum over one wavefront.  for_each_key(f) calls f(key) once for every real key of the
// calling thread; it is called once per pass.  hsub: 256 x 8 words of LDS, hist: 256 words, state: in LDS (hist apart
// from state: as one 1032-byte object they cost gf_quant 12 bytes of LDS padding).  Four barriers per pass; the routine
// writes its own initial state and returns after the last barrier (hsub and hist are the caller's again at once).
// Preconditions: every one of the NT threads of the workgroup calls it; 1 <= want <= the number of keys.
template <int NT, class Keys>
__device__ __forceinline__ unsigned block_radix_select(Keys for_each_key, unsigned want, unsigned *hsub, unsigned *hist,
                                                       RadixSelectState &state) {
  static_assert(NT >= 256 && NT % 64 == 0, "one thread per bin");
  const int tid = threadIdx.x;
  if (tid == 0) { state.prefix = 0u; state.remaining = want; }
  unsigned mask = 0u;
  for (int shift = 24; shift >= 0; shift -= 8) {
    for (int e = tid; e < 256 * 8; e += NT) hsub[e] = 0u;
    __syncthreads();
    const unsigned prefix = state.prefix;
    for_each_key([&](unsigned key) __attribute__((always_inline)) {
      if ((key & mask) == prefix) atomicAdd(&hsub[((key >> shift) & 255u) * 8 + (tid & 7)], 1u);
    });
    __syncthreads();
    if (NT == 256 || tid < 256) {
      unsigned h = 0;
#pragma unroll
      for (int x = 0; x < 8; x++) h += hsub[tid * 8 + x];
      hist[tid] = h;
    }
    __syncthreads();
    if (tid < 64) {
      // the bin in which the running count reaches `remaining`: four bins per lane, a prefix sum over the lanes
      const unsigned h0 = hist[4 * tid], h1 = hist[4 * tid + 1], h2 = hist[4 * tid + 2], h3 = hist[4 * tid + 3];
      const unsigned mine = h0 + h1 + h2 + h3;
      unsigned incl = mine;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned up = __shfl_up(incl, o);
        if (tid >= o) incl += up;
      }
      const unsigned rem = state.remaining;
      const unsigned long long reach = __ballot(incl >= rem);
      // (a total below `remaining` cannot happen -- every pass keeps at least `remaining` keys -- but the last lane takes
      // it then)
      const int first = reach ? __ffsll((long long)reach) - 1 : 63;
      if (tid == first) {
        unsigned cum = incl - mine;
        int bin = 4 * tid;
        if (cum + h0 >= rem) { }
        else if (cum + h0 + h1 >= rem) { cum += h0; bin += 1; }
        else if (cum + h0 + h1 + h2 >= rem) { cum += h0 + h1; bin += 2; }
        else { cum += h0 + h1 + h2; bin += 3; }
        state.remaining = rem - cum;
        state.prefix = prefix | ((unsigned)bin << shift);
      }
    }
    mask |= 255u << shift;
    __syncthreads();
  }
  return state.prefix;
}

// ---- 64-lane bitonic networks: lane = element ------------------------------------------------------------------------
// One sort and one merge; the compare-exchange step pick(x, y, low) leaves in x what a lane keeps of its own x and its
// partner's y: the lower of the two where `low`, the upper otherwise.  (gq_rerank's sort of (value, id) pairs keeps its
// own loop, grouped.hip: through this one it compiles to other code)
__device__ inline unsigned long long shfl_u64(unsigned long long x, int src) {
  const unsigned lo = (unsigned)__shfl((int)(unsigned)x, src), hi = (unsigned)__shfl((int)(unsigned)(x >> 32), src);
  return ((unsigned long long)hi << 32) | lo;
}
__device__ inline unsigned long long shfl_xor_u64(unsigned long long x, int m) {
  const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)x, m), hi = (unsigned)__shfl_xor((int)(unsigned)(x >> 32), m);
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ float lane_from(float x, int src) { return __shfl(x, src); }
__device__ __forceinline__ unsigned long long lane_from(unsigned long long x, int src) { return shfl_u64(x, src); }
__device__ __forceinline__ float lane_xor(float x, int j) { return __shfl_xor(x, j); }
__device__ __forceinline__ unsigned long long lane_xor(unsigned long long x, int j) { return shfl_xor_u64(x, j); }

template <class T, class Pick>
__device__ __forceinline__ T sort64(T x, int lane, Pick pick) {   // ascending
#pragma unroll
  for (int k = 2; k <= 64; k <<= 1)
#pragma unroll
    for (int j = k >> 1; j >= 1; j >>= 1) {
      const T y = lane_xor(x, j);
      const bool up = (lane & k) == 0, lower = (lane & j) == 0;
      pick(x, y, lower == up);
    }
  return x;
}
template <class T, class Pick>
__device__ __forceinline__ T merge64(T a, T b, int lane, Pick pick) {   // a, b ascending: the 64 smallest of both, ascending
  pick(a, lane_from(b, 63 - lane), true);   // bitonic sequence holding the 64 smallest
#pragma unroll
  for (int j = 32; j >= 1; j >>= 1) pick(a, lane_xor(a, j), (lane & j) == 0);
  return a;
}

struct PickF32 {   // fminf / fmaxf: what they do with a NaN is part of bound_tables' result
  __device__ __forceinline__ void operator()(float &x, float y, bool low) const { x = low ? fminf(x, y) : fmaxf(x, y); }
};
struct PickU64 {
  __device__ __forceinline__ void operator()(unsigned long long &x, unsigned long long y, bool low) const {
    x = low ? (x < y ? x : y) : (x < y ? y : x);
  }
};
__device__ __forceinline__ float sort64_asc(float x, int lane) { return sort64(x, lane, PickF32{}); }
__device__ __forceinline__ float merge64_asc(float a, float b, int lane) { return merge64(a, b, lane, PickF32{}); }
__device__ __forceinline__ unsigned long long sort64_u64(unsigned long long x, int lane) { return sort64(x, lane, PickU64{}); }
__device__ __forceinline__ unsigned long long merge64_u64(unsigned long long a, unsigned long long b, int lane) { return merge64(a, b, lane, PickU64{}); }

// ---- the survivor sub-queues of one query ---------------------------------------------------------------------------
// A filter kernel appends the rows a query keeps to one of the query's NSLOT sub-queues (enqueue_halves: workgroups of
// different chunks use different ones); the kernel that re-scores them reads the NSLOT queues as one flat list.
// Constructing it reads the fill levels (lane = sub-queue, in every wave); what a kernel does about an overflow and
// where its barriers stand is the kernel's.
template <int NSLOT>
struct SurvivorQueues {
  int *cnt;            // [queries][NSLOT] fill levels
  int q, lane, mine, start[NSLOT];
  __device__ __forceinline__ SurvivorQueues(int *cnt_, int q_, int lane_) : cnt(cnt_), q(q_), lane(lane_) {
    mine = lane < NSLOT ? cnt[q * NSLOT + lane] : 0;
  }
  __device__ __forceinline__ void clear(bool mine_to_clear) const {   // (one wave's job, after every wave has read)
    if (mine_to_clear && lane < NSLOT) cnt[q * NSLOT + lane] = 0;
  }
  __device__ __forceinline__ bool overflowed(int cap) const { return __ballot(mine > cap) != 0ull; }
  __device__ __forceinline__ void clamp(int cap) { mine = min(mine, cap); }
  // the number of survivors; fixes the flat numbering entry() goes by (call it once, after clamp)
  __device__ __forceinline__ int count() {
    int incl = mine;
#pragma unroll
    for (int o = 1; o < NSLOT; o <<= 1) {
      const int up = __shfl_up(incl, o);
      if (lane >= o) incl += up;
    }
    const int n = readlane_i(incl, NSLOT - 1);
#pragma unroll
    for (int sl = 0; sl < NSLOT; sl++) start[sl] = readlane_i(incl - mine, sl);
    return n;
  }
  __device__ __forceinline__ int entry(const int *queue, int q, int cap, int e) const {   // e-th survivor of query q, e < count()
    int sl = 0;
#pragma unroll
    for (int x = 1; x < NSLOT; x++) sl += e >= start[x];
    int off = start[0];
#pragma unroll
    for (int x = 1; x < NSLOT; x++) off = sl == x ? start[x] : off;
    return queue[((size_t)q * NSLOT + sl) * cap + (e - off)];
  }
};

// The tail of a filter kernel's row block: `l` holds what is left of two queries' budgets for the lane's row (low half:
// query q_lo, high half: q_lo + 2; non-zero: the query keeps the row).  A full sub-queue sets fb_word(query), the
// caller's flag for that query (looked up only then: its address arithmetic stays on the overflow path).
template <int NSLOT, class FbWord>
__device__ __forceinline__ void enqueue_halves(uint32_t l, int q_lo, int slot, int row, int *cnt, int *queue, int cap,
                                               FbWord fb_word) {
#pragma unroll
  for (int q = q_lo; q <= q_lo + 2; q += 2)
    if (q == q_lo ? l & 0xFFFFu : l >> 16) {
      const int sq = q * NSLOT + slot;
      const int pos = atomicAdd(&cnt[sq], 1);
      if (pos < cap) queue[(size_t)sq * cap + pos] = row;
      else fb_word(q) = 1;
    }
}

#ifdef GULON_TEST_HOOKS
// What the stage hooks (filter_query.hip, wide_filter.hip) hand back of the sub-queues a filter launch left on the device:
// counts_out [B][nslot], the fill counters, unclamped; rows_out [B][nslot * cap], a query's queued rows (entries beyond a
// full sub-queue are lost, as in production) plus row_base, ascending, padded with -1.  Host code; synchronous.
inline void export_survivor_queues(const int *d_cnt, const int *d_queue, int nslot, int Bq, int B, int cap, int row_base,
                                   int32_t *rows_out, int32_t *counts_out) {
  std::vector<int> cnt((size_t)Bq * nslot), queue((size_t)Bq * nslot * cap);
  HIP_CHECK(hipMemcpy(cnt.data(), d_cnt, sizeof(int) * cnt.size(), hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(queue.data(), d_queue, sizeof(int) * queue.size(), hipMemcpyDeviceToHost));
  for (int q = 0; q < B; q++) {
    int32_t *out = rows_out + (size_t)q * nslot * cap;
    size_t fill = 0;
    for (int sl = 0; sl < nslot; sl++) {
      const int c = cnt[(size_t)q * nslot + sl];
      counts_out[(size_t)q * nslot + sl] = c;
      for (int e = 0; e < std::min(c, cap); e++) out[fill++] = queue[((size_t)q * nslot + sl) * cap + e] + row_base;
    }
    std::sort(out, out + fill);
    for (size_t e = fill; e < (size_t)nslot * cap; e++) out[e] = -1;
  }
}
#endif

}  // namespace gulon
