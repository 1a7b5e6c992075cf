// KMeans.fromAssignment on gfx950 (KMeans.scala:198-226): the bucketed update.
//
//   update   KMeans.fromAssignment: order-dependent running mean  c += (x - c)/n.
//            Rows are bucketed by cluster with a STABLE counting sort, then every
//            (cluster, dim) chain runs sequentially in row order.
//            More than 10240 clusters: the order comes from a radix sort of (row, cluster) pairs (bigk_*).
// The streamed form that PQ training takes for k <= 1024 is kmeans_stream.hip; the driver kmeans.hip.
#include "kmeans.hpp"

#include <map>

namespace gulon {

// ---------------------------------------------------------------------------
// update: stable counting sort by cluster, then sequential chains
// ---------------------------------------------------------------------------
constexpr int CHUNK_ROWS = 1024;   // rows per workgroup-chunk of the counting sort (256 per wave)

// All update kernels take an array of per-problem descriptors and pick theirs with
// blockIdx.y (z for the group scan), so the m sub-quantizers of a ProductQuantizer are
// updated by ONE launch each: the sequential chains are latency-bound (k*s threads per
// problem), and only running all problems' chains side by side fills the GPU.

// per chunk histogram: hist[chunk][k]
__global__ __launch_bounds__(256) void sort_hist(const UpdDesc *__restrict__ descs, int n, int k) {
  const UpdDescG D = load_desc(descs, blockIdx.y);
  extern __shared__ unsigned sh[];  // k
  for (int c = threadIdx.x; c < k; c += 256) sh[c] = 0;
  __syncthreads();
  const long long chunk = blockIdx.x;
  const long long r0 = chunk * CHUNK_ROWS;
  const long long r1 = r0 + CHUNK_ROWS < n ? r0 + CHUNK_ROWS : n;
  for (long long r = r0 + threadIdx.x; r < r1; r += 256) atomicAdd(&sh[D.assign[r]], 1u);
  __syncthreads();
  for (int c = threadIdx.x; c < k; c += 256) D.hist[(size_t)chunk * k + c] = sh[c];
}

// two-level exclusive scan of the per-chunk histograms (per cluster, over chunks):
// level 1: one thread per (group of SCAN_GROUP chunks, cluster) scans its chunks in place
constexpr int SCAN_GROUP = 64;
__global__ void sort_scan_groups(const UpdDesc *__restrict__ descs, long long nchunks, int k) {
  const UpdDescG D = load_desc(descs, blockIdx.z);
  int c = blockIdx.y * blockDim.x + threadIdx.x;
  long long g = blockIdx.x;
  if (c >= k) return;
  long long c0 = g * SCAN_GROUP, c1 = c0 + SCAN_GROUP < nchunks ? c0 + SCAN_GROUP : nchunks;
  unsigned run = 0;
  for (long long ch = c0; ch < c1; ch++) {
    unsigned v = D.hist[(size_t)ch * k + c];
    D.hist[(size_t)ch * k + c] = run;
    run += v;
  }
  D.gtot[(size_t)g * k + c] = run;
}
// level 2: one thread per cluster scans the group totals; then cluster starts
__global__ void sort_scan_top(const UpdDesc *__restrict__ descs, long long ngroups, int k) {
  const UpdDescG D = load_desc(descs, blockIdx.y);
  extern __shared__ unsigned cnt[];  // k
  for (int c = threadIdx.x; c < k; c += blockDim.x) {
    unsigned run = 0;
    for (long long g = 0; g < ngroups; g++) {
      unsigned v = D.gtot[(size_t)g * k + c];
      D.gtot[(size_t)g * k + c] = run;
      run += v;
    }
    cnt[c] = run;
    D.count[c] = run;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned run = 0;
    for (int c = 0; c < k; c++) { D.start[c] = run; run += cnt[c]; }
  }
  // clusters by descending size: update_chains is as slow as its longest chain, and the workgroups holding the
  // longest ones should be the first to get a SIMD (rank by counting; k is small where this matters)
  if (D.corder) {
    for (int c = threadIdx.x; c < k; c += blockDim.x) {
      const unsigned mine = cnt[c];
      int rank = 0;
      for (int o = 0; o < k; o++) rank += cnt[o] > mine || (cnt[o] == mine && o < c);
      D.corder[rank] = c;
    }
  }
}

// Stable placement of a chunk's rows: bucket position start[c] + rank <- the row's slice, rank = rows of the
// same cluster before it (in row order).  The slices themselves move here -- xb[position] = slice of the row,
// sp = s rounded up to even floats so that every bucket row starts 8-byte aligned -- because the chains that
// follow are sequential per (cluster, dim): over row ids they were a random gather of 40-byte pieces (one
// 64-byte sector each, 320 M sectors per full-PQ iteration at BASELINE config 3: the bound of the round-1
// kernel); over the regrouped copy every chain streams contiguous memory.
//
// One workgroup per 1024-row chunk, wave w = rows [256 w, 256 w + 256) in four steps of 64:
//   A  per-wave cluster counts.  The lanes holding the same cluster are found without a loop: one ballot per
//      key bit, the AND of (bit set ? ballot : ~ballot) is the mask of lanes with an equal key;
//   B  chunk-local exclusive scan over (cluster, wave) -> every wave's first position per cluster;
//   C  placement: position = wave's running position + rank among the step's equal keys (popcount of the
//      mask below the lane); same-wave LDS accesses execute in program order, so every lane of a cluster
//      reads the running position before the cluster's first lane advances it;
//   D  (STAGED) the chunk's slices were written to LDS in sorted order; they leave as contiguous runs -- one
//      per cluster, chunk rows / k slices long -- instead of one scattered 40-byte store per row (12.8 GB in
//      21 ms against ~5 ms at BASELINE config 3: partial-line stores do not combine).
// STAGED needs k <= 1024 and sp <= 16 (LDS); otherwise the slices go straight to their positions.
// Measured and dropped (round 2, commit 0fb1c3a has the kernel): the same placement as a persistent stream -- as many
// workgroups as the chip holds, each requesting its NEXT chunk before sorting the current one.  Loads and sort alone
// then take 2.5 ms, but with the stores 8.6 ms against 5.9 ms for this kernel: the stores are what binds -- unaligned
// 160-byte runs leave at 3.4 TB/s at best (scripts/micro/store_runs.hip; whole aligned 128-byte lines: 5.7 TB/s) --
// and a workgroup that lives on has to wait for its own stores before it can trust its look-ahead loads (vmcnt counts
// both, in order), while a workgroup that ends leaves its stores to drain under the next one's loads.
// Also measured and dropped: stage D in 16-byte stores (a unit on an even address opens a pair with its successor, run
// heads and tails leave alone in 8-byte stores of their own): 7.2 ms against 5.9 -- a run then leaves in three
// instructions instead of one, and what the memory side is short of is requests per line, not bytes per request
// (WRITE_SIZE = the algorithmic 12.8 GB either way).
template <int SMAX /* 0: slices go straight to their positions; else staged, s <= SMAX */>
__global__ __launch_bounds__(256) void sort_place(const UpdDesc *__restrict__ descs, int n, int k, int key_bits,
                                                  int cpx /* > 0: chunks per XCD, 1-D grid */) {
  constexpr bool STAGED = SMAX > 0;
  constexpr int NV = STAGED ? SMAX : 1;
  // Which chunk: workgroups are dealt round-robin over the 8 XCDs (observed, for speed only), and a chunk's run of a
  // cluster continues where the previous chunk's ended -- two partial lines per 160-byte run at BASELINE config 3.
  // With consecutive chunks on the SAME XCD, at about the same time, the halves of a line meet in that XCD's L2 and
  // leave as one full line; dealt over eight L2s every run is written back as partial lines.
  int prob = blockIdx.y;
  long long chunk = blockIdx.x;
  if (cpx > 0) {
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    prob = slot / cpx;
    chunk = (long long)xcd * cpx + (slot - prob * cpx);
    if (chunk * CHUNK_ROWS >= n) return;
  }
  const UpdDescG D = load_desc(descs, prob);
  extern __shared__ unsigned sh[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned *wh = sh;                                  // [4][k] per-wave counts, then running positions
  unsigned *gpos = sh + 4 * k;                        // STAGED: [k] bucket position of chunk-local position 0
  int *dstrow = reinterpret_cast<int *>(sh + 5 * k);  // STAGED: [CHUNK_ROWS] bucket position of a local position
  unsigned short *lpos = reinterpret_cast<unsigned short *>(sh + 5 * k + CHUNK_ROWS);   // STAGED: [CHUNK_ROWS] local position of a chunk row
  float *sorted = reinterpret_cast<float *>(sh + ((5 * k + CHUNK_ROWS + CHUNK_ROWS / 2 + 1) & ~1));   // STAGED: [CHUNK_ROWS][sp], 8-byte aligned
  __shared__ unsigned wave_tot[4];
  const long long r0 = chunk * CHUNK_ROWS;
  const long long r1 = r0 + CHUNK_ROWS < n ? r0 + CHUNK_ROWS : n;
  const long long grp = chunk / SCAN_GROUP;
  const int s = D.s, sp = (s + 1) & ~1;
  // STAGED: the wave's 256 slices are 256 * s consecutive floats of the compact source = 64 * s float4: all of them
  // requested now (s loads of 16 bytes per lane), consumed after the positions are known
  f32x4 v[NV];
  const long long wr0 = r0 + wave * 256;                          // first row of this wave
  const int wrows = (int)max(0ll, min(256ll, r1 - wr0));          // its rows
  if (STAGED) {
    const auto src4 = reinterpret_cast<gptr<const f32x4>>(D.x + (size_t)wr0 * s);
    const int nf4 = wrows * s / 4, tail0 = nf4 * 4, total = wrows * s;   // whole float4s, then up to 3 floats
#pragma unroll
    for (int u = 0; u < NV; u++) {
      const int f = lane + 64 * u;
      v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (u < s) {
        if (f < nf4) v[u] = __builtin_nontemporal_load(&src4[f]);   // read once: keeps L2 for the partial lines of the stores (6.1 -> 5.9 ms; nt STORES: 9.2 ms)
        else if (f == nf4 && tail0 < total) {
          const auto tp = D.x + (size_t)wr0 * s + tail0;
          v[u].x = tp[0];
          if (tail0 + 1 < total) v[u].y = tp[1];
          if (tail0 + 2 < total) v[u].z = tp[2];
        }
      }
    }
  }
  for (int e = tid; e < 4 * k; e += 256) wh[e] = 0;
  __syncthreads();
  const unsigned long long lt = (1ull << lane) - 1ull;
  // A: keys of this lane's four rows, per-wave counts
  int keys[4];
  unsigned long long same[4];
#pragma unroll
  for (int t = 0; t < 4; t++) {
    const long long r = wr0 + t * 64 + lane;
    const bool valid = r < r1;
    keys[t] = valid ? D.assign[r] : 0;
  }
#pragma unroll
  for (int t = 0; t < 4; t++) {
    const bool valid = wr0 + t * 64 + lane < r1;
    unsigned long long sm = __ballot(valid);
    for (int bit = 0; bit < key_bits; bit++) {
      const unsigned long long bm = __ballot((keys[t] >> bit) & 1);
      sm &= ((keys[t] >> bit) & 1) ? bm : ~bm;
    }
    same[t] = valid ? sm : 0ull;
    if (valid && (sm & lt) == 0ull) wh[wave * k + keys[t]] += (unsigned)__popcll(sm);   // only this wave touches wh[wave]
  }
  __syncthreads();
  // B: first position of every (cluster, wave)
  if (STAGED) {
    // exclusive scan of the chunk's cluster totals: thread t owns clusters [t*per, t*per + per)
    const int per = (k + 255) / 256;
    unsigned mine = 0;
    for (int c = tid * per; c < min(k, tid * per + per); c++)
      mine += wh[c] + wh[k + c] + wh[2 * k + c] + wh[3 * k + c];
    unsigned incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned up = __shfl_up(incl, o);
      if (lane >= o) incl += up;
    }
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    unsigned base = incl - mine;
    for (int w = 0; w < wave; w++) base += wave_tot[w];
    for (int c = tid * per; c < min(k, tid * per + per); c++) {
      const unsigned t0 = wh[c], t1 = wh[k + c], t2 = wh[2 * k + c], t3 = wh[3 * k + c];
      gpos[c] = D.start[c] + D.gtot[(size_t)grp * k + c] + D.hist[(size_t)chunk * k + c] - base;
      wh[c] = base; wh[k + c] = base + t0; wh[2 * k + c] = base + t0 + t1; wh[3 * k + c] = base + t0 + t1 + t2;
      base += t0 + t1 + t2 + t3;
    }
  } else {
    for (int c = tid; c < k; c += 256) {
      const unsigned t0 = wh[c], t1 = wh[k + c], t2 = wh[2 * k + c];
      const unsigned base = D.start[c] + D.gtot[(size_t)grp * k + c] + D.hist[(size_t)chunk * k + c];
      wh[c] = base; wh[k + c] = base + t0; wh[2 * k + c] = base + t0 + t1; wh[3 * k + c] = base + t0 + t1 + t2;
    }
  }
  __syncthreads();
  // C: placement
#pragma unroll
  for (int t = 0; t < 4; t++) {
    const long long r = wr0 + t * 64 + lane;
    const bool valid = r < r1;
    const int key = keys[t];
    const unsigned b = valid ? wh[wave * k + key] : 0u;
    const unsigned pos = b + (unsigned)__popcll(same[t] & lt);
    if (valid && (same[t] & lt) == 0ull) wh[wave * k + key] = b + (unsigned)__popcll(same[t]);
    if (STAGED) {
      if (valid) { dstrow[pos] = (int)(gpos[key] + pos); lpos[wave * 256 + t * 64 + lane] = (unsigned short)pos; }
    } else if (valid) {
      const auto dst = D.xb + (size_t)pos * sp;
      const auto src = D.x + (size_t)r * D.ld + D.from;
      int j = 0;
      for (; j + 2 <= s; j += 2) *reinterpret_cast<gptr<f32x2>>(dst + j) = f32x2{src[j], src[j + 1]};
      if (j < s) *reinterpret_cast<gptr<f32x2>>(dst + j) = f32x2{src[j], src[j]};   // odd s: the padding column mirrors the last one
    }
  }
  if (!STAGED) return;
  // every prefetched element to the chunk-local position of its row (same-wave LDS order: lpos is written above)
  {
    const unsigned rdiv = (65536u + (unsigned)s - 1u) / (unsigned)s;   // e / s == (e * rdiv) >> 16 for e < 4096, s <= 16
    const int total = wrows * s;
#pragma unroll
    for (int u = 0; u < NV; u++) {
      if (u < s) {
        const float vv[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
        for (int c4 = 0; c4 < 4; c4++) {
          const int e = 4 * (lane + 64 * u) + c4;
          if (e < total) {
            const int row = (int)(((unsigned)e * rdiv) >> 16);
            const int j = e - row * s;
            float *dstp = sorted + (size_t)lpos[wave * 256 + row] * sp + j;
            dstp[0] = vv[c4];
            if (j + 1 == s && sp != s) dstp[1] = vv[c4];   // odd s: the padding column mirrors the last one (update_chains_pk)
          }
        }
      }
    }
  }
  __syncthreads();
  // D: sorted slices leave as float2 units; consecutive units of a cluster's run are consecutive in memory
  const int h = sp >> 1;
  const int units = (int)(r1 - r0) * h;
  const unsigned hdiv = ((1u << 20) + (unsigned)h - 1u) / (unsigned)h;   // u / h == (u * hdiv) >> 20 for u < 8192, h <= 8
  const f32x2 *src2 = reinterpret_cast<const f32x2 *>(sorted);
  const auto dst2 = reinterpret_cast<gptr<f32x2>>(D.xb);
  for (int u = tid; u < units; u += 256) {
    const int lp = (int)(((unsigned long long)(unsigned)u * hdiv) >> 20);
    const int part = u - lp * h;
    dst2[(size_t)dstrow[lp] * h + part] = src2[u];
  }
}

// ---- the running mean's division, off the critical path ---------------------------------------------------
// c <- c + (x - c)/n needs RN((x - c)/n), the correctly rounded quotient (what the JVM's float division gives).
// __fdiv_rn is ~11 dependent instructions; the chain has nothing else to overlap them with (k*s chains per
// problem: ~1.25 waves per SIMD at BASELINE config 3), so its latency IS the kernel's time.  With y = RN(1/n)
// (a table: n is the step number, wave-uniform) Markstein's correction gives the same quotient in three
// dependent operations:   q0 = RN(a y);  r = RN(a - n q0) (exact, one fma);  q = RN(q0 + r y)  ==  RN(a / n)
// whenever y is the correctly rounded reciprocal and nothing under- or overflows (a faithful q0 plus one
// fma-corrected step; Markstein 1990, Cornea-Harrison-Tang 2002).  mean_step_fast is only trusted for
// 2^-60 < |a| < 2^60 and n < 2^24 (every intermediate stays normal, every step number is a float); a batch in which
// any step falls outside is recomputed with __fdiv_rn.  gulon_selftest_mean_division checks the identity against __fdiv_rn for EVERY
// n in [1, 2^24) over random and near-halfway numerators (tests/test_gpu_kmeans.py).
__device__ __forceinline__ float mean_quotient_fast(float a, float nf, float y) {
  const float q0 = a * y;
  const float r = __builtin_fmaf(-nf, q0, a);
  return __builtin_fmaf(r, y, q0);
}
// The proofs of the corrected quotient single out divisors whose significand is all ones (for integers: n = 2^j - 1)
// as the ones for which a numerator can exist that the correction rounds the other way; the sampled self-test
// cannot rule such a numerator out, so these ~24 divisors never take the fast path: a batch of 32 steps, divisors
// 32 b + 1 .. 32 b + 32, holds one iff b + 1 is a power of two (b = 0: 1, 3, 7, 15, 31) -- two dozen batches of a
// chain's thousands go through __fdiv_rn.
__device__ __forceinline__ bool batch_has_all_ones_divisor(unsigned b) { return ((b + 1u) & b) == 0u; }
__device__ __forceinline__ bool mean_fast_ok(float a) {
  const float m = fabsf(a);
  return m > 8.673617379884035e-19f /* 2^-60 */ && m < 1.152921504606847e18f /* 2^60 */;
}

__global__ void rcp_table_kernel(float *__restrict__ out, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = __fdiv_rn(1.0f, (float)(int)(i + 1));
}

#ifdef GULON_TEST_HOOKS
// mismatches of mean_quotient_fast against __fdiv_rn: every divisor n in [1, n_max], `per` numerators each --
// random ones and ones built to sit next to a rounding boundary (n times a random quotient, one ulp up and down)
__global__ void mean_division_selftest(int n_max, int per, unsigned long long seed, unsigned long long *__restrict__ bad) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long total = (long long)n_max * per;
  unsigned long long mism = 0;
  for (long long w = t; w < total; w += (long long)gridDim.x * blockDim.x) {
    const int n = (int)(w / per) + 1;
    const int e = (int)(w % per);
    unsigned long long z = seed + (unsigned long long)w * 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL; z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL; z ^= z >> 31;
    const float nf = (float)n;
    // the reciprocal the streamed update computes in its loop (kmeans_stream.hip): every divisor it is used for
    if (e == 0 && __float_as_uint(rcp_rn_int(nf)) != __float_as_uint(__fdiv_rn(1.0f, nf))) mism++;
    // a random float with exponent in [-40, 40]
    const unsigned mant = (unsigned)(z & 0x7FFFFF), sgn = (unsigned)((z >> 23) & 1);
    const int ex = (int)((z >> 24) % 81) - 40;
    float a = __uint_as_float((sgn << 31) | ((unsigned)(ex + 127) << 23) | mant);
    if (e & 1) {   // a = RN(n * q) nudged by -1, 0, +1 ulp: quotients next to q and to its rounding boundaries
      const float q = a;
      a = nf * q;
      const int nudge = (int)((z >> 40) % 3) - 1;
      a = __uint_as_float(__float_as_uint(a) + (unsigned)nudge);
    }
    if (!mean_fast_ok(a)) continue;
    const float y = __fdiv_rn(1.0f, nf);
    const float fast = mean_quotient_fast(a, nf, y);
    const float ref = __fdiv_rn(a, nf);
    if (__float_as_uint(fast) != __float_as_uint(ref)) mism++;
  }
  // the divisors 2^j - 1 (the integers nearest to the all-ones significands the proofs single out): EVERY numerator
  // significand and sign of one binade -- the arithmetic is scale invariant between the under- and overflow ranges
  // the callers keep out of -- with the reciprocal of the streamed update (tests/test_markstein_exhaustive.py is the
  // same sweep on the CPU)
  for (long long w = t; w < (24ll << 24); w += (long long)gridDim.x * blockDim.x) {
    const int j = (int)(w >> 24) + 1;
    if ((1 << j) - 1 > n_max) break;
    const float nf = (float)((1 << j) - 1);
    const float a = __uint_as_float((((unsigned)w >> 23) & 1u) << 31 | 127u << 23 | ((unsigned)w & 0x7FFFFFu));
    const float fast = mean_quotient_fast(a, nf, rcp_rn_int(nf));
    if (__float_as_uint(fast) != __float_as_uint(__fdiv_rn(a, nf))) mism++;
  }
  if (mism) atomicAdd(bad, mism);
}
#endif

// one thread per (cluster, dim): c_j <- c_j + (x_j - c_j)/n over the cluster's rows
// in row order (KMeans.scala:211-224); int->float RNE, correctly rounded quotient (above).
// The cluster's slices are contiguous in xb (sort_place).  A three-deep software pipeline of 32-step batches
// keeps 64 steps of loads in flight per lane (no load depends on the chain).  The kernel is one wave per 64
// chains and there are barely more waves than SIMDs (1280 at BASELINE config 3, two on some SIMDs), so it is
// as fast as its instruction stream is short: the main loop runs clear of the cluster's end (no index clamps), and the
// range test of the fast quotient is one min and one max per step, looked at once per batch.  This is the form for
// problems of different bucket row strides; one shared stride up to 16 takes update_chains_pk.
__global__ __launch_bounds__(64) void update_chains(const UpdDesc *__restrict__ descs, int k,
                                                    const float *__restrict__ rcp /* scalar loads: see update_chains_pk */) {
  const UpdDescG D = load_desc(descs, blockIdx.x);           // x = problem, y = block of 64 chains: blocks are dispatched x-fastest,
  const int s = D.s, sp = (s + 1) & ~1;                      // so every problem's longest chains (block 0) come first
  int t = blockIdx.y * blockDim.x + threadIdx.x;
  if (t >= k * s) return;
  const int slot = t / s, j = t - slot * s;
  const int c = D.corder ? D.corder[slot] : slot;
  const unsigned len = D.count[c];
  float p = 0.f;
  if (len == 0) { D.cout[c * s + j] = 0.f; return; }
  const auto col = D.xb + (size_t)D.start[c] * sp + j;
  constexpr int U = 32;
  const unsigned last = len - 1;
  unsigned i = 0;
  if (len >= 3 * U) {
    float xa[U], xb[U], xc[U];
#pragma unroll
    for (int u = 0; u < U; u++) xa[u] = col[(size_t)u * sp];
#pragma unroll
    for (int u = 0; u < U; u++) xb[u] = col[(size_t)(U + u) * sp];
    auto nxt = col + (size_t)2 * U * sp;
    // batches whose look-ahead (two batches) stays inside the cluster
    for (; i + 3 * U <= len; i += U, nxt += (size_t)U * sp) {
#pragma unroll
      for (int u = 0; u < U; u++) xc[u] = nxt[(size_t)u * sp];
      const float p0 = p;
      float lo = INFINITY, hi = 0.f;
      float nf = (float)(int)(i + 1);
#pragma unroll
      for (int u = 0; u < U; u++) {
        const float a = xa[u] - p;
        lo = fminf(lo, fabsf(a));
        hi = fmaxf(hi, fabsf(a));
        p = p + mean_quotient_fast(a, nf, rcp[i + u]);
        nf += 1.0f;                                   // exact up to 2^24; a batch that reaches it is redone below
      }
      // a zero, tiny, huge or NaN numerator somewhere in the batch, a divisor whose significand is all ones
      // (2^j - 1: see mean_quotient_fast) among its 32, or a last step at or beyond 2^24 (the divisor is RN(count) there,
      // which `nf` above does not follow, and the corrected quotient is only checked below it; stream_chains has the same
      // rule): the plain division, from the batch's start
      if (!__all(lo > 8.673617379884035e-19f /* 2^-60 */ && hi < 1.152921504606847e18f /* 2^60 */) ||
          batch_has_all_ones_divisor(i / U) || i + U >= (1u << 24)) {
        p = p0;
#pragma unroll
        for (int u = 0; u < U; u++) p = p + __fdiv_rn(xa[u] - p, (float)(int)(i + u + 1));
      }
#pragma unroll
      for (int u = 0; u < U; u++) { xa[u] = xb[u]; xb[u] = xc[u]; }
    }
    // the two batches already in registers
#pragma unroll
    for (int u = 0; u < U; u++) p = p + __fdiv_rn(xa[u] - p, (float)(int)(i + u + 1));
    i += U;
#pragma unroll
    for (int u = 0; u < U; u++) p = p + __fdiv_rn(xb[u] - p, (float)(int)(i + u + 1));
    i += U;
  }
  for (; i <= last; i++) p = p + __fdiv_rn(col[(size_t)i * sp] - p, (float)(int)(i + 1));
  D.cout[c * s + j] = p;
}

// Two chains per lane on the packed fp32 pipe.  The chain kernel is latency bound -- five dependent operations per
// step, nothing to overlap them with -- and with one (cluster, dim) per lane BASELINE config 3 needs 1280 waves for
// 1024 SIMDs: the SIMDs holding two pay every step twice.  v_pk_add/mul/fma_f32 carry two IEEE binary32 lanes per
// register pair at the cost of one instruction, so lane = (cluster, PAIR of dims): 640 waves, one per SIMD, and the
// per-step instruction stream (5 packed + min3 + max3 + one 8-byte load) is no longer than the scalar one was.
// The bucket row stride is even (sort_place), so the pair is one aligned 8-byte load; the second half of the last
// pair of an odd s walks the padding column, which sort_place fills with a copy of the last real column: a chain
// that behaves exactly like its neighbour (same range checks, same path) and is never stored.  (Mirroring it here,
// one v_cndmask per loaded value, made every load wait for its data at once.)
// The wave walks its batches in LOCKSTEP: the trip count is the maximum over its lanes and every lane stays active
// to the end -- a lane whose cluster is exhausted keeps its result aside, re-reads its last batch (in bounds, cached)
// and is left out of the range test.  That makes the step number wave-uniform with all 64 lanes alive, so the 32
// reciprocals of a batch can travel like a 33rd column: lane u of `ycur` holds RN(1 / (i + u + 1)), requested two
// batches ahead by one coalesced load, and every step reads its own with v_readlane; the divisors are converted once
// per batch the same way.  (As scalar loads they were requested at the top of the batch that needs them and waited
// for three times per batch -- a third of the time of a wave that has its SIMD to itself; as per-lane vector loads,
// round 1, they sat behind the look-ahead loads in vmcnt order: 3 of the first update's 8.4 ms at BASELINE config 3.)
// What the batches leave of a cluster (fewer than three batches) is walked with the plain division at the end.
template <int SP /* bucket row stride in floats (even) */>
__global__ __launch_bounds__(64) void update_chains_pk(const UpdDesc *__restrict__ descs, int k,
                                                       const float *__restrict__ rcp) {
  static_assert(SP % 2 == 0 && SP >= 2, "even stride");
  constexpr int HP = SP / 2;
  constexpr int U = 32;
  const UpdDescG D = load_desc(descs, blockIdx.x);           // x = problem, y = block of 64 lanes: every problem's longest chains first
  const int s = D.s;
  const int t = blockIdx.y * blockDim.x + threadIdx.x;
  const int slot = t / HP, jp = t - slot * HP, j = 2 * jp;
  const bool valid = t < k * HP && j < s;          // (j >= s: a problem narrower than the launch's stride)
  const bool pad = j + 1 >= s;
  const int c = valid ? (D.corder ? D.corder[slot] : slot) : 0;
  const unsigned len = valid ? D.count[c] : 0u;
  const auto col = reinterpret_cast<gptr<const f32x2>>(D.xb + (valid ? (size_t)D.start[c] * SP + j : (size_t)0));
  auto slow = [](f32x2 p, f32x2 x, unsigned n1) {
    const float nf = (float)(int)n1;
    p.x = p.x + __fdiv_rn(x.x - p.x, nf);
    p.y = p.y + __fdiv_rn(x.y - p.y, nf);
    return p;
  };
  // batches of this lane (the look-ahead of two batches stays inside the cluster), and of the wave
  const unsigned nb = len >= 3 * U ? (len - 3 * U) / U + 1 : 0u;
  unsigned nb_wave = nb;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) nb_wave = max(nb_wave, (unsigned)__shfl_xor((int)nb_wave, o));
  nb_wave = (unsigned)__builtin_amdgcn_readfirstlane((int)nb_wave);
  f32x2 p = {0.f, 0.f}, p_keep = {0.f, 0.f};
  if (nb_wave > 0) {       // some cluster of the wave has >= 96 rows, so 96 rows from the bucket's base are in bounds
    const int l32 = threadIdx.x & 31;
    auto nxt = nb > 0 ? col : reinterpret_cast<gptr<const f32x2>>(D.xb);   // lanes without batches read the base rows
    unsigned i = 0, b = 0;
    // one batch: the look-ahead loads of the batch after next into `ld`, then the 32 steps of `cur`
    auto batch = [&](const f32x2 (&cur)[U], float ycur, f32x2 (&ld)[U], float &yld) {
      const bool live = b < nb;                    // this lane's cluster still has this batch
      const auto src = nxt + (size_t)(live ? 2 * U * HP : 0);   // (a finished lane re-reads where it stands: inside its cluster)
#pragma unroll
      for (int u = 0; u < U; u++) ld[u] = src[(size_t)u * HP];
      yld = rcp[i + 2 * U + l32];
      const f32x2 p0 = p;
      float lo = INFINITY, hi = 0.f;
      const float nfv = (float)(int)(i + 1 + l32);
#pragma unroll
      for (int u = 0; u < U; u++) {
        const f32x2 a = cur[u] - p;
        lo = fminf(fminf(lo, fabsf(a.x)), fabsf(a.y));
        hi = fmaxf(fmaxf(hi, fabsf(a.x)), fabsf(a.y));
        const float y = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ycur), u));
        const float nf = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(nfv), u));
        const f32x2 y2 = {y, y}, nn = {-nf, -nf};
        const f32x2 q0 = a * y2;
        const f32x2 r = __builtin_elementwise_fma(nn, q0, a);
        p = p + __builtin_elementwise_fma(r, y2, q0);
      }
      // a zero, tiny, huge or NaN numerator somewhere in a live lane's batch, a divisor whose significand is all ones
      // (2^j - 1: see mean_quotient_fast) among its 32, or a last step at or beyond 2^24 (where the corrected quotient
      // is not checked): the plain division, from the batch's start
      if (!__all(!live || (lo > 8.673617379884035e-19f /* 2^-60 */ && hi < 1.152921504606847e18f /* 2^60 */)) ||
          batch_has_all_ones_divisor(b) || i + U >= (1u << 24)) {
        p = p0;
#pragma unroll
        for (int u = 0; u < U; u++) p = slow(p, cur[u], i + u + 1);
      }
      if (live) { p_keep = p; nxt += (size_t)U * HP; }
      i += U;
      b++;
    };
    f32x2 xa[U], xb[U], xc[U];
    float ya, yb, yc;
#pragma unroll
    for (int u = 0; u < U; u++) xa[u] = nxt[(size_t)u * HP];
    ya = rcp[l32];
#pragma unroll
    for (int u = 0; u < U; u++) xb[u] = nxt[(size_t)(U + u) * HP];
    yb = rcp[U + l32];
    // three batches per trip, the buffers taking turns (no register copies)
    while (b + 3 <= nb_wave) { batch(xa, ya, xc, yc); batch(xb, yb, xa, ya); batch(xc, yc, xb, yb); }
    if (b < nb_wave) batch(xa, ya, xc, yc);
    if (b < nb_wave) batch(xb, yb, xa, ya);
  }
  // what the batches left of the cluster: fewer than three batches' worth, from memory, the plain division
  p = p_keep;
  for (unsigned i = nb * U; i < len; i++) p = slow(p, col[(size_t)i * HP], i + 1);
  if (valid) {
    D.cout[c * s + j] = p.x;
    if (!pad) D.cout[c * s + j + 1] = p.y;
  }
}

// ---- more clusters than the counting sort's LDS counters hold (k > 10240, up to the 65536 of
// ProductQuantizer.coderFactory, ProductQuantizer.scala:11-16): the stable order comes from a two-pass LSD radix
// sort of (row, cluster) pairs -- each pass is the counting sort above with 256 buckets (one byte of the cluster
// id as the key, the 8-byte pair as the "slice") -- and the chains read their rows through the sorted row ids.
__global__ void bigk_pairs(const int *__restrict__ assign, int n, int2 *__restrict__ pairs, int *__restrict__ digit) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const int a = assign[r];
  pairs[r] = make_int2(r, a);
  digit[r] = a & 255;
}
__global__ void bigk_digit2(const int2 *__restrict__ pairs, int n, int *__restrict__ digit) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) digit[i] = (pairs[i].y >> 8) & 255;
}
__global__ void bigk_count(const int *__restrict__ assign, int n, unsigned *__restrict__ count) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n) atomicAdd(&count[assign[r]], 1u);
}
__global__ __launch_bounds__(1024) void bigk_starts(const unsigned *__restrict__ count, int k, unsigned *__restrict__ start) {
  __shared__ unsigned part[1024];
  const int per = (k + 1023) / 1024, t = threadIdx.x;
  unsigned sum = 0;
  for (int c = t * per; c < min(k, t * per + per); c++) sum += count[c];
  part[t] = sum;
  __syncthreads();
  if (t == 0) { unsigned run = 0; for (int i = 0; i < 1024; i++) { const unsigned v = part[i]; part[i] = run; run += v; } }
  __syncthreads();
  unsigned run = part[t];
  for (int c = t * per; c < min(k, t * per + per); c++) { start[c] = run; run += count[c]; }
}
// one thread per (cluster, dim), rows through the sorted pairs (KMeans.scala:211-224; IEEE division)
__global__ void update_chains_indirect(const int2 *__restrict__ pairs, const unsigned *__restrict__ count,
                                       const unsigned *__restrict__ start, const float *__restrict__ X, int ld, int from,
                                       int s, int k, float *__restrict__ cout) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)k * s) return;
  const int c = (int)(t / s), j = (int)(t - (long long)c * s);
  const unsigned len = count[c];
  const int2 *ord = pairs + start[c];
  float p = 0.f;
  constexpr int U = 8;
  unsigned i = 0;
  for (; i + U <= len; i += U) {
    float x[U];
#pragma unroll
    for (int u = 0; u < U; u++) x[u] = X[(size_t)ord[i + u].x * ld + from + j];
#pragma unroll
    for (int u = 0; u < U; u++) p = p + __fdiv_rn(x[u] - p, (float)(int)(i + u + 1));
  }
  for (; i < len; i++) p = p + __fdiv_rn(X[(size_t)ord[i].x * ld + from + j] - p, (float)(int)(i + 1));
  cout[t] = p;
}

void KmeansWorkspace::ensure_update(int n, int k, int s) {
  long long nchunks = ceil_div(std::max(n, 1), CHUNK_ROWS);
  const bool bigk = sizeof(unsigned) * 4 * (size_t)k > 160 * 1024;   // radix path: its scratch lives in the call
  if (!bigk) {
    hist.ensure((size_t)nchunks * k);
    gtot.ensure((size_t)ceil_div(nchunks, SCAN_GROUP) * k);
  }
  count.ensure(k);
  start.ensure(k);
  if (!bigk) xb.ensure((size_t)std::max(n, 1) * (size_t)((s + 1) & ~1));
  corder.ensure(k);
}

static void launch_counting_sort(UpdDesc *d_descs, int np, int n, int k, int smax, bool compact, hipStream_t st) {
  long long nchunks = ceil_div(n, CHUNK_ROWS);
  long long ngroups = ceil_div(nchunks, SCAN_GROUP);
  const int sp_max = (smax + 1) & ~1;
  const bool staged = compact && k <= 1024 && sp_max <= 16;
  const size_t shm_hist = sizeof(unsigned) * (size_t)k;
  const size_t shm_place = staged ? sizeof(unsigned) * (5 * (size_t)k + CHUNK_ROWS + CHUNK_ROWS / 2 + 8) + sizeof(float) * CHUNK_ROWS * (size_t)sp_max
                                  : sizeof(unsigned) * 4 * (size_t)k;
  GULON_UNSUPPORTED(shm_place > 160 * 1024, "internal: counting sort with k = %d needs %zu B of LDS", k, shm_place);
  HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(sort_hist), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)shm_hist));
  hipLaunchKernelGGL(sort_hist, dim3((unsigned)nchunks, np), dim3(256), shm_hist, st, d_descs, n, k);
  hipLaunchKernelGGL(sort_scan_groups, dim3((unsigned)ngroups, ceil_div(k, 256), np), dim3(256), 0, st, d_descs,
                     nchunks, k);
  hipLaunchKernelGGL(sort_scan_top, dim3(1, np), dim3(256), sizeof(unsigned) * (size_t)k, st, d_descs, ngroups, k);
  int key_bits = 0;
  while ((1 << key_bits) < k) key_bits++;
  auto place = !staged ? sort_place<0> : smax <= 4 ? sort_place<4> : smax <= 8 ? sort_place<8> : smax <= 12 ? sort_place<12>
                                                                                                       : sort_place<16>;
  HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(place), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)shm_place));
  const int cpx = staged ? (int)ceil_div(nchunks, 8LL) : 0;
  if (cpx > 0)
    hipLaunchKernelGGL(place, dim3((unsigned)(8LL * cpx * np)), dim3(256), shm_place, st, d_descs, n, k, key_bits, cpx);
  else
    hipLaunchKernelGGL(place, dim3((unsigned)nchunks, np), dim3(256), shm_place, st, d_descs, n, k, key_bits, 0);
  HIP_CHECK(hipGetLastError());
}

static void kmeans_update_bigk(const UpdDesc &D, UpdDesc *d_desc, int n, int k, hipStream_t st) {
  // scratch of this rare path lives for the call (synchronised before it goes)
  DevBuf<int2> p0((size_t)n), p1((size_t)n), p2((size_t)n);
  DevBuf<int> digit((size_t)n);
  const long long nchunks = ceil_div(n, CHUNK_ROWS);
  DevBuf<unsigned> hist((size_t)nchunks * 256), gtot((size_t)ceil_div(nchunks, SCAN_GROUP) * 256), c256(256), s256(256);
  hipLaunchKernelGGL(bigk_pairs, dim3(ceil_div(n, 256)), dim3(256), 0, st, D.assign, n, p0.p, digit.p);
  for (int pass = 0; pass < 2; pass++) {
    UpdDesc S{};
    S.assign = digit.p; S.hist = hist.p; S.gtot = gtot.p; S.count = c256.p; S.start = s256.p;
    S.x = reinterpret_cast<const float *>(pass == 0 ? p0.p : p1.p); S.ld = 2; S.from = 0; S.s = 2;
    S.xb = reinterpret_cast<float *>(pass == 0 ? p1.p : p2.p);
    S.cout = nullptr; S.rcp = nullptr; S.corder = nullptr;
    HIP_CHECK(hipMemcpyAsync(d_desc, &S, sizeof(UpdDesc), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));   // S is a stack object
    launch_counting_sort(d_desc, 1, n, 256, 2, true, st);
    if (pass == 0) hipLaunchKernelGGL(bigk_digit2, dim3(ceil_div(n, 256)), dim3(256), 0, st, p1.p, n, digit.p);
  }
  HIP_CHECK(hipMemsetAsync(D.count, 0, sizeof(unsigned) * (size_t)k, st));
  hipLaunchKernelGGL(bigk_count, dim3(ceil_div(n, 256)), dim3(256), 0, st, D.assign, n, D.count);
  hipLaunchKernelGGL(bigk_starts, dim3(1), dim3(1024), 0, st, D.count, k, D.start);
  hipLaunchKernelGGL(update_chains_indirect, dim3((unsigned)ceil_div((long long)k * D.s, 256LL)), dim3(256), 0, st, p2.p,
                     D.count, D.start, D.x, D.ld, D.from, D.s, k, D.cout);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(st));
}

void kmeans_update_batch(const std::vector<UpdDesc> &descs, UpdDesc *d_descs, int n, int k, hipStream_t st) {
  const int np = (int)descs.size();
  if (np == 0) return;
  if (n <= 0) {
    for (const UpdDesc &D : descs) HIP_CHECK(hipMemsetAsync(D.cout, 0, sizeof(float) * (size_t)k * D.s, st));
    return;
  }
  if (sizeof(unsigned) * 4 * (size_t)k > 160 * 1024) {   // k > 10240: radix-sorted row ids, one problem at a time
    GULON_UNSUPPORTED(k > 65536, "too many clusters: %d", k);
    for (const UpdDesc &D : descs) kmeans_update_bigk(D, d_descs, n, k, st);
    return;
  }
  HIP_CHECK(hipMemcpyAsync(d_descs, descs.data(), sizeof(UpdDesc) * np, hipMemcpyHostToDevice, st));
  int smax = 1;
  for (const UpdDesc &D : descs) smax = std::max(smax, D.s);
  bool compact = true;   // every problem reads a compact copy of its slice (ld == s): the staged placement's coalesced loads
  for (const UpdDesc &D : descs) compact = compact && D.ld == D.s && D.from == 0;
  const int sp_max = (smax + 1) & ~1;
  launch_counting_sort(d_descs, np, n, k, smax, compact, st);
  bool one_stride = true;   // every problem with the same bucket row stride: the chains take it as a constant
  for (const UpdDesc &D : descs) one_stride = one_stride && ((D.s + 1) & ~1) == sp_max;
  // one wave per workgroup; with more workgroups than SIMDs, 40 KiB of (unused) LDS each keeps four per CU -- one per
  // SIMD at full issue rate -- and the rest, the SHORTEST chains (size order), start as the first ones finish
  // two chains per lane on the packed pipe wherever the stride is a compile-time constant, else one
  const bool pk = one_stride && sp_max <= 16;
  static constexpr decltype(&update_chains) packed[8] = {update_chains_pk<2>,  update_chains_pk<4>,  update_chains_pk<6>,
                                                          update_chains_pk<8>,  update_chains_pk<10>, update_chains_pk<12>,
                                                          update_chains_pk<14>, update_chains_pk<16>};
  const auto chains = pk ? packed[sp_max / 2 - 1] : update_chains;
  const int chain_blocks = pk ? ceil_div((long long)k * (sp_max / 2), 64) : ceil_div((long long)k * smax, 64);
  int cus = 256;
  { int dev = 0; HIP_CHECK(hipGetDevice(&dev)); HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev)); }
  constexpr int per_cu = 4;
  size_t chain_lds = 0;
  if ((long long)chain_blocks * np > (long long)per_cu * cus) chain_lds = (size_t)(160 * 1024) / per_cu;
  HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(chains), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)std::max<size_t>(chain_lds, 1)));
  hipLaunchKernelGGL(chains, dim3(np, chain_blocks), dim3(64), chain_lds, st, d_descs, k, descs[0].rcp);
  HIP_CHECK(hipGetLastError());
}

// RN(1/i) for i = 1 .. n: shared by every problem on this device (grown on demand, never shrunk)
static const float *rcp_table(int n) {
  struct Tab { DevBuf<float> buf; };
  static std::mutex mu;
  static std::map<int, Tab> tabs;
  std::lock_guard<std::mutex> lock(mu);
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  Tab &t = tabs[dev];
  if ((size_t)n > t.buf.n) {
    const long long want = std::max<long long>(n, 1024);
    HIP_CHECK(hipDeviceSynchronize());   // nothing in flight may still read the table about to be replaced
    t.buf.alloc((size_t)want);
    hipLaunchKernelGGL(rcp_table_kernel, dim3((unsigned)ceil_div(want, 256)), dim3(256), 0, 0, t.buf.p, want);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
  }
  return t.buf.p;
}

UpdDesc make_upd_desc(KmeansWorkspace &ws, const float *x, int ld, int n, int k, int from, int s, const int *d_assign,
                      float *dC) {
  ws.ensure_update(n, k, s);
  UpdDesc D;
  D.x = x; D.ld = ld;
  D.assign = d_assign; D.hist = ws.hist.p; D.gtot = ws.gtot.p; D.count = ws.count.p; D.start = ws.start.p;
  D.xb = ws.xb.p; D.cout = dC; D.from = from; D.s = s;
  D.rcp = rcp_table(n);
  D.corder = k <= 2048 ? ws.corder.p : nullptr;
  return D;
}

// single-problem form
void kmeans_update_dev(KmeansWorkspace &ws, const float *dX, int n, int ld, int from, int s, int k,
                       const int *d_assign, float *dC, hipStream_t st) {
  std::vector<UpdDesc> descs{make_upd_desc(ws, dX, ld, n, k, from, s, d_assign, dC)};
  ws.descs.ensure(1);
  kmeans_update_batch(descs, ws.descs.p, n, k, st);
  // descs is read by hipMemcpyAsync from pageable memory: staged before the call returns
}

}  // namespace gulon

#ifdef GULON_TEST_HOOKS
using namespace gulon;
GULON_API int32_t gulon_selftest_mean_division(int32_t n_max, int32_t numerators_per_divisor, uint64_t seed,
                                               int64_t *mismatches) {
  return guarded([&] {
    GULON_REQUIRE(mismatches != nullptr && n_max >= 1 && n_max < (1 << 24) && numerators_per_divisor >= 1, "bad arguments");
    DevBuf<unsigned long long> bad(1);
    HIP_CHECK(hipMemset(bad.p, 0, sizeof(unsigned long long)));
    hipLaunchKernelGGL(mean_division_selftest, dim3(8192), dim3(256), 0, 0, n_max, numerators_per_divisor,
                       (unsigned long long)seed, bad.p);
    HIP_CHECK(hipGetLastError());
    unsigned long long h = 0;
    HIP_CHECK(hipMemcpy(&h, bad.p, sizeof(h), hipMemcpyDeviceToHost));
    *mismatches = (int64_t)h;
  });
}
#endif
