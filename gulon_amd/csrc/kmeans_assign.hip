// KMeans.assign / parAssign on gfx950 (KMeans.scala:24-98): the exact half of the assign.
//
//   assign   exact argmin of  offsets[c] - 2*(x . c)  in the JVM's unfused, sequential
//            binary32 order, including the  d == min && rng.nextBoolean()  tie-break:
//            pass 1 computes the draw-free argmin and the number of RNG draws each row
//            makes; a segmented prefix sum places every row in its java.util.Random
//            stream (one stream per rng_batch rows); pass 2 replays only the rows that
//            draw, after an O(log) LCG jump-ahead.
// The MFMA filter in front of it is kmeans_mfma.hip; the update kmeans_update.hip / kmeans_stream.hip; the training
// driver and the C ABI kmeans.hip.
#include "kmeans.hpp"

namespace gulon {

// ---------------------------------------------------------------------------
// centroid prep: KMeans.apply offsets (KMeans.scala:170-186) + zero-padded copy.
// Zero padding is exact: d + 0*0 == d for every binary32 d (a -0 partial sum may
// become +0, which no comparison or later operation here can observe).
// ---------------------------------------------------------------------------
__global__ void prep_centroids(const float *__restrict__ C, int k, int s, int smax, float *__restrict__ Cpad,
                               float *__restrict__ off) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= k) return;
  float acc = 0.f;
  for (int j = 0; j < s; j++) {
    float x = C[(size_t)c * s + j];
    acc += x * x;
    Cpad[(size_t)c * smax + j] = x;
  }
  for (int j = s; j < smax; j++) Cpad[(size_t)c * smax + j] = 0.f;
  off[c] = acc;
}

// ---------------------------------------------------------------------------
// pass 1: draw-free argmin + number of draws (KMeans.scala:33-54 / :76-97 with
// rng.nextBoolean() read as false).  assign[] is written only when some centroid
// won, exactly like the reference (NaN distances never win).
// ---------------------------------------------------------------------------
// STAGE: the padded centroids and their offsets are copied to LDS first (k * (SMAX + 1) floats <= 64 KiB), pairs of
// centroids interleaved per dimension.  Every
// lane reads the same centroid, so from global memory these are scalar loads that the loop waits for centroid by
// centroid (the re-check of 120 K flagged rows: 125 us, a few hundred cycles of load latency per centroid); from LDS
// they are broadcast reads the compiler can request several centroids ahead.
template <int SMAX, bool STAGE>
__global__ __launch_bounds__(256) void assign_exact(const float *__restrict__ X, int n, int ld, int from, int s,
                                                    const float *__restrict__ Cpad, const float *__restrict__ off,
                                                    int k, const int *__restrict__ rows, int nrows,
                                                    int *__restrict__ assign, unsigned *__restrict__ ties,
                                                    unsigned long long *__restrict__ tie_total) {
  extern __shared__ float exact_lds[];   // STAGE: [ceil(k/2)][SMAX][2] centroid PAIRS (c, c+1 interleaved per dim), then [k] offsets
  const int kp = (k + 1) / 2;
  if (STAGE) {
    for (int e = threadIdx.x; e < kp * SMAX * 2; e += 256) {
      const int cp = e / (2 * SMAX), r = e - cp * 2 * SMAX, j = r >> 1, c = 2 * cp + (r & 1);
      exact_lds[e] = c < k ? Cpad[(size_t)c * SMAX + j] : 0.f;
    }
    for (int e = threadIdx.x; e < 2 * kp; e += 256) exact_lds[kp * SMAX * 2 + e] = e < k ? off[e] : 0.f;
    __syncthreads();
  }
  int t = blockIdx.x * 256 + threadIdx.x;
  int i = -1;
  if (t < nrows) i = rows ? rows[t] : t;
  float x[SMAX];
#pragma unroll
  for (int j = 0; j < SMAX; j++) x[j] = 0.f;
  if (i >= 0) {
    const float *row = X + (size_t)i * ld + from;
#pragma unroll
    for (int j = 0; j < SMAX; j++)
      if (j < s) x[j] = row[j];
  }
  float mn = FLT_MAX;
  int best = -1;
  unsigned nt = 0;
  if (STAGE) {
    // two centroids per step on the packed fp32 pipe: each component is the reference's own sequential, unfused chain
    // (v_pk_mul_f32 / v_pk_add_f32 round every component like their scalar forms); the comparisons stay in centroid
    // order.  The kernel is bound by its arithmetic (k * s products per row), so this halves it.
    const f32x2 *pairs = reinterpret_cast<const f32x2 *>(exact_lds);
    const f32x2 *offs = reinterpret_cast<const f32x2 *>(exact_lds + kp * SMAX * 2);
#pragma unroll 2
    for (int cp = 0; cp < kp; cp++) {
      const f32x2 *cc = pairs + (size_t)cp * SMAX;
      f32x2 d = {0.f, 0.f};
#pragma unroll
      for (int j = 0; j < SMAX; j++) {
        const f32x2 xx = {x[j], x[j]};
        d = d + xx * cc[j];
      }
      const f32x2 two = {2.f, 2.f};
      d = offs[cp] - two * d;
      if (d.x < mn) { mn = d.x; best = 2 * cp; }
      else if (d.x == mn) nt++;
      if (2 * cp + 1 < k) {
        if (d.y < mn) { mn = d.y; best = 2 * cp + 1; }
        else if (d.y == mn) nt++;
      }
    }
  } else {
    for (int c = 0; c < k; c++) {
      const float *cc = Cpad + (size_t)c * SMAX;
      float d = 0.f;
#pragma unroll
      for (int j = 0; j < SMAX; j++) d += x[j] * cc[j];
      d = off[c] - 2 * d;
      if (d < mn) { mn = d; best = c; }
      else if (d == mn) nt++;
    }
  }
  if (i >= 0) {
    if (best >= 0) assign[i] = best;
    ties[i] = nt;
  } else {
    nt = 0;
  }
  // any draws in this launch?
  unsigned long long wsum = nt;
  for (int o = 32; o > 0; o >>= 1) wsum += __shfl_down(wsum, o);
  if ((threadIdx.x & 63) == 0 && wsum) atomicAdd(tie_total, wsum);
}

// generic dimension (s > 128): x re-read from memory for every centroid
__global__ __launch_bounds__(256) void assign_exact_generic(const float *__restrict__ X, int n, int ld, int from,
                                                            int s, const float *__restrict__ Cpad, int smax,
                                                            const float *__restrict__ off, int k,
                                                            const int *__restrict__ rows, int nrows,
                                                            int *__restrict__ assign, unsigned *__restrict__ ties,
                                                            unsigned long long *__restrict__ tie_total) {
  int t = blockIdx.x * 256 + threadIdx.x;
  int i = -1;
  if (t < nrows) i = rows ? rows[t] : t;
  unsigned nt = 0;
  if (i >= 0) {
    const float *row = X + (size_t)i * ld + from;
    float mn = FLT_MAX;
    int best = -1;
    for (int c = 0; c < k; c++) {
      const float *cc = Cpad + (size_t)c * smax;
      float d = 0.f;
      for (int j = 0; j < s; j++) d += row[j] * cc[j];
      d = off[c] - 2 * d;
      if (d < mn) { mn = d; best = c; }
      else if (d == mn) nt++;
    }
    if (best >= 0) assign[i] = best;
    ties[i] = nt;
  }
  unsigned long long wsum = nt;
  for (int o = 32; o > 0; o >>= 1) wsum += __shfl_down(wsum, o);
  if ((threadIdx.x & 63) == 0 && wsum) atomicAdd(tie_total, wsum);
}

// ---------------------------------------------------------------------------
// segmented exclusive prefix sum of ties[] (segments = rng_batch rows): where each
// row's draws sit in its java.util.Random stream.
// ---------------------------------------------------------------------------
__device__ inline unsigned block_exclusive_scan_1024(unsigned v, unsigned *total, unsigned *lds /*>=16*/) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned inc = v;
  for (int o = 1; o < 64; o <<= 1) {
    unsigned u = __shfl_up(inc, o);
    if (lane >= o) inc += u;
  }
  if (lane == 63) lds[wave] = inc;
  __syncthreads();
  if (wave == 0) {
    unsigned w = lane < 16 ? lds[lane] : 0;
    unsigned winc = w;
    for (int o = 1; o < 16; o <<= 1) {
      unsigned u = __shfl_up(winc, o);
      if (lane >= o) winc += u;
    }
    if (lane < 16) lds[lane] = winc - w;   // exclusive wave offsets
    if (lane == 15) lds[16] = winc;
  }
  __syncthreads();
  unsigned res = inc - v + lds[wave];
  *total = lds[16];
  __syncthreads();
  return res;
}

// grid (blocks_per_seg, nseg), 1024 threads
__global__ __launch_bounds__(1024) void tie_block_sums(const unsigned *__restrict__ ties, int n, int seg_len,
                                                       int bps, unsigned *__restrict__ local,
                                                       unsigned *__restrict__ block_tot) {
  __shared__ unsigned lds[32];
  int seg = blockIdx.y, blk = blockIdx.x;
  long long seg_begin = (long long)seg * seg_len;
  long long seg_end = seg_begin + seg_len < n ? seg_begin + seg_len : n;
  long long idx = seg_begin + (long long)blk * 1024 + threadIdx.x;
  unsigned v = idx < seg_end ? ties[idx] : 0u;
  unsigned tot;
  unsigned ex = block_exclusive_scan_1024(v, &tot, lds);
  if (idx < seg_end) local[idx] = ex;
  if (threadIdx.x == 0) block_tot[(size_t)seg * bps + blk] = tot;
}

// one block per segment: exclusive scan of that segment's block totals
__global__ __launch_bounds__(1024) void tie_block_scan(const unsigned *__restrict__ block_tot, int bps,
                                                       unsigned long long *__restrict__ block_off) {
  __shared__ unsigned lds[32];
  __shared__ unsigned long long carry;
  int seg = blockIdx.x;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < bps; base += 1024) {
    int b = base + threadIdx.x;
    unsigned v = b < bps ? block_tot[(size_t)seg * bps + b] : 0u;
    unsigned tot;
    unsigned ex = block_exclusive_scan_1024(v, &tot, lds);
    unsigned long long c0 = carry;
    if (b < bps) block_off[(size_t)seg * bps + b] = c0 + ex;
    __syncthreads();
    if (threadIdx.x == 0) carry = c0 + tot;
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// pass 2: replay the rows that draw, with the RNG jumped to their stream position.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void assign_resolve(const float *__restrict__ X, int n, int ld, int from, int s,
                                                      const float *__restrict__ Cpad, int smax,
                                                      const float *__restrict__ off, int k,
                                                      const unsigned *__restrict__ ties,
                                                      const unsigned *__restrict__ local,
                                                      const unsigned long long *__restrict__ block_off, int seg_len,
                                                      int bps, const int *__restrict__ rows, int nrows,
                                                      int *__restrict__ assign) {
  int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= nrows) return;
  int i = rows ? rows[t] : t;          // only the flagged rows can draw when the MFMA filter ran
  if (ties[i] == 0) return;
  int seg = i / seg_len;
  int blk = (i - seg * seg_len) / 1024;
  unsigned long long pos = block_off[(size_t)seg * bps + blk] + local[i];
  JRandom rng(0);
  rng.skip(pos);
  const float *row = X + (size_t)i * ld + from;
  float mn = FLT_MAX;
  int best = -1;
  for (int c = 0; c < k; c++) {
    const float *cc = Cpad + (size_t)c * smax;
    float d = 0.f;
    for (int j = 0; j < s; j++) d += row[j] * cc[j];
    d = off[c] - 2 * d;
    if (d < mn || (d == mn && rng.next_boolean())) { best = c; mn = d; }
  }
  if (best >= 0) assign[i] = best;
}

// The same replay with one WAVE per drawing row (for many centroids / long sub-vectors, where one
// thread walking k * s products is a 100-ms latency chain): rows with draws are compacted first;
// the lanes compute 64 centroids' distances at a time (each lane its centroid's sequential,
// unfused chain -- the reference's arithmetic), then the scan over those 64 runs in centroid order
// on the candidates that can change the minimum or draw (d <= running minimum).
__global__ void collect_tie_rows(const unsigned *__restrict__ ties, const int *__restrict__ rows, int nrows,
                                 int *__restrict__ list, unsigned *__restrict__ count) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nrows) return;
  int i = rows ? rows[t] : t;
  if (ties[i] != 0) list[atomicAdd(count, 1u)] = i;
}

// Stream positions of a FEW drawing rows without the dense per-row arrays: row i's draws start after those of the
// drawing rows before it in its segment.  (The dense form -- zero a 40 MB array, scatter the flagged rows' counts,
// copy, block sums, block scan -- moves 120 MB per problem and iteration for, typically, 70 drawing rows.)
__global__ void tie_positions_sparse(const unsigned *__restrict__ ties, const int *__restrict__ list,
                                     const unsigned *__restrict__ count, int seg_len,
                                     unsigned long long *__restrict__ pos) {
  const unsigned total = *count;
  const unsigned e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int i = list[e], seg = i / seg_len;
  unsigned long long p = 0;
  for (unsigned o = 0; o < total; o++) {
    const int r = list[o];
    if (r < i && r / seg_len == seg) p += ties[r];
  }
  pos[e] = p;
}

// pos != null: the stream position of list[e] is pos[e] (tie_positions_sparse); else block_off / local (dense form)
__global__ __launch_bounds__(64) void assign_resolve_wave(const float *__restrict__ X, int ld, int from, int s,
                                                          const float *__restrict__ Cpad, int smax,
                                                          const float *__restrict__ off, int k,
                                                          const unsigned *__restrict__ local,
                                                          const unsigned long long *__restrict__ block_off,
                                                          int seg_len, int bps, const int *__restrict__ list,
                                                          const unsigned *__restrict__ count,
                                                          int *__restrict__ assign,
                                                          const unsigned long long *__restrict__ pos) {
  extern __shared__ float rowv[];   // s
  const int lane = threadIdx.x;
  const unsigned total = *count;
  for (unsigned e = blockIdx.x; e < total; e += gridDim.x) {
    const int i = list[e];
    __syncthreads();
    for (int j = lane; j < s; j += 64) rowv[j] = X[(size_t)i * ld + from + j];
    __syncthreads();
    const int seg = i / seg_len;
    const int blk = (i - seg * seg_len) / 1024;
    JRandom rng(0);
    rng.skip(pos ? pos[e] : block_off[(size_t)seg * bps + blk] + local[i]);
    float mn = FLT_MAX;
    int best = -1;
    for (int c0 = 0; c0 < k; c0 += 64) {
      const int c = c0 + lane;
      float d = 0.f;
      if (c < k) {
        const float *cc = Cpad + (size_t)c * smax;
        for (int j = 0; j < s; j++) d += rowv[j] * cc[j];
        d = off[c] - 2 * d;
      }
      // in centroid order: only d < mn or d == mn can act (NaN never does)
      unsigned long long mk = __ballot(c < k && d <= mn);
      while (mk) {
        const int l = __ffsll((long long)mk) - 1;
        mk &= mk - 1;
        const float dv = readlane_f(d, l);
        if (dv < mn || (dv == mn && rng.next_boolean())) { best = c0 + l; mn = dv; }
      }
    }
    if (lane == 0 && best >= 0) assign[i] = best;
  }
}

__global__ void scatter_ties(const int *__restrict__ rows, int nrows, const unsigned *__restrict__ ties,
                             unsigned *__restrict__ dense) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < nrows) dense[rows[t]] = ties[rows[t]];
}

// ---------------------------------------------------------------------------
// host drivers
// ---------------------------------------------------------------------------
static int pick_smax(int s) {
  if (s <= 4) return 4;
  if (s <= 8) return 8;
  if (s <= 10) return 10;   // (BASELINE config 3's sub-vectors are 9 and 10 wide: padded to 16 the exact re-check did 60-78 %
  if (s <= 12) return 12;   //  more products than it had to)
  if (s <= 16) return 16;
  if (s <= 32) return 32;
  if (s <= 64) return 64;
  if (s <= 128) return 128;
  return s;
}

KmeansWorkspace::~KmeansWorkspace() { if (host) (void)hipHostFree(host); }

void KmeansWorkspace::ensure_assign(int n, int k, int s) {
  if (!host) HIP_CHECK(hipHostMalloc((void **)&host, sizeof(HostWords)));
  int smax = pick_smax(s);
  cpad.ensure((size_t)k * smax);
  off.ensure(k);
  ties.ensure((size_t)std::max(n, 1));
  local.ensure((size_t)std::max(n, 1));
  tie_total.ensure(1);
}

// ---------------------------------------------------------------------------
// KMeans.assign / parAssign on device arrays, as three enqueue stages separated by stream
// synchronisations (the host needs two counters: #flagged rows, #RNG draws).  The stages
// let the trainer run many independent problems on their own streams and pay the
// synchronisations once per iteration instead of once per problem.
// d_assign is written only where a centroid won (caller initialises it).
// rng_batch <= 0: one java.util.Random stream over all rows.
// ---------------------------------------------------------------------------
// centroids + offsets in LDS when they fit 64 KiB (k = 256: 17 KiB at s <= 16)
template <int S>
static void launch_exact_padded(AssignJob &j, int grid) {
  KmeansWorkspace &ws = *j.ws;
  const size_t lds = sizeof(float) * (size_t)((j.k + 1) / 2) * 2 * (S + 1);
  if (lds <= 64 * 1024) {
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(assign_exact<S, true>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((assign_exact<S, true>), dim3(grid), dim3(256), lds, j.st, j.dX, j.n, j.ld, j.from, j.s,
                       ws.cpad.p, ws.off.p, j.k, j.rows, j.nrows, j.d_assign, ws.ties.p, ws.tie_total.p);
  } else {
    hipLaunchKernelGGL((assign_exact<S, false>), dim3(grid), dim3(256), 0, j.st, j.dX, j.n, j.ld, j.from, j.s,
                       ws.cpad.p, ws.off.p, j.k, j.rows, j.nrows, j.d_assign, ws.ties.p, ws.tie_total.p);
  }
}

static void launch_exact(AssignJob &j) {
  KmeansWorkspace &ws = *j.ws;
  const int smax = pick_smax(j.s);
  const int grid = ceil_div(j.nrows, 256);
  switch (smax) {
    case 4: launch_exact_padded<4>(j, grid); break;
    case 8: launch_exact_padded<8>(j, grid); break;
    case 10: launch_exact_padded<10>(j, grid); break;
    case 12: launch_exact_padded<12>(j, grid); break;
    case 16: launch_exact_padded<16>(j, grid); break;
    case 32: launch_exact_padded<32>(j, grid); break;
    case 64: launch_exact_padded<64>(j, grid); break;
    case 128: launch_exact_padded<128>(j, grid); break;
    default:
      hipLaunchKernelGGL(assign_exact_generic, dim3(grid), dim3(256), 0, j.st, j.dX, j.n, j.ld, j.from, j.s, ws.cpad.p,
                         smax, ws.off.p, j.k, j.rows, j.nrows, j.d_assign, ws.ties.p, ws.tie_total.p);
  }
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(&ws.host->total, ws.tie_total.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, j.st));
}

// stage 1: centroid prep, then either the MFMA filter (+ flagged-row count) or the exact
// scan of every row (+ draw count)
void assign_stage1(AssignJob &j) {
  j.done = j.n <= 0;
  if (j.done) return;
  KmeansWorkspace &ws = *j.ws;
  ws.ensure_assign(j.n, j.k, j.s);
  ws.last_draws = 0;
  ws.last_flagged = 0;
  const int smax = pick_smax(j.s);
  hipLaunchKernelGGL(prep_centroids, dim3(ceil_div(j.k, 64)), dim3(64), 0, j.st, j.dC, j.k, j.s, smax, ws.cpad.p,
                     ws.off.p);
  HIP_CHECK(hipMemsetAsync(ws.tie_total.p, 0, sizeof(unsigned long long), j.st));
  j.filtered = j.ps != nullptr && mfma_assign_supported(j.s, j.k);
  if (j.filtered) {
    assign_mfma_filter(ws, *j.ps, j.dC, j.k, j.d_assign, j.st);
    HIP_CHECK(hipMemcpyAsync(&ws.host->flagged, ws.flag_count.p, sizeof(unsigned), hipMemcpyDeviceToHost, j.st));
  } else {
    j.rows = nullptr;
    j.nrows = j.n;
    launch_exact(j);
  }
}

// stage 2 (after a stream sync): exact scan of the flagged rows, or -- unfiltered -- the
// tie replay
constexpr unsigned long long SPARSE_TIE_DRAWS = 8192;   // up to this many draws the positions come from the drawing rows alone

static void launch_tie_replay(AssignJob &j, bool sparse = false) {
  KmeansWorkspace &ws = *j.ws;
  const int n = j.n, smax = pick_smax(j.s);
  const int seg_len = j.rng_batch > 0 ? j.rng_batch : n;
  if (sparse) {   // (filtered jobs, wave-per-row replay: ws.ties holds the flagged rows' counts, indexed by row)
    ws.tie_rows.ensure((size_t)std::max(j.nrows, 1));
    ws.tie_count.ensure(1);
    ws.tie_pos.ensure((size_t)SPARSE_TIE_DRAWS);
    HIP_CHECK(hipMemsetAsync(ws.tie_count.p, 0, sizeof(unsigned), j.st));
    hipLaunchKernelGGL(collect_tie_rows, dim3(ceil_div(j.nrows, 256)), dim3(256), 0, j.st, ws.ties.p, j.rows, j.nrows,
                       ws.tie_rows.p, ws.tie_count.p);
    hipLaunchKernelGGL(tie_positions_sparse, dim3((unsigned)ceil_div((long long)SPARSE_TIE_DRAWS, 256LL)), dim3(256), 0, j.st,
                       ws.ties.p, ws.tie_rows.p, ws.tie_count.p, seg_len, ws.tie_pos.p);
    hipLaunchKernelGGL(assign_resolve_wave, dim3(256), dim3(64), sizeof(float) * (size_t)j.s, j.st, j.dX, j.ld, j.from,
                       j.s, ws.cpad.p, smax, ws.off.p, j.k, (const unsigned *)nullptr, (const unsigned long long *)nullptr,
                       seg_len, 0, ws.tie_rows.p, ws.tie_count.p, j.d_assign, ws.tie_pos.p);
    HIP_CHECK(hipGetLastError());
    return;
  }
  const int nseg = ceil_div(n, seg_len);
  const int bps = ceil_div(seg_len < n ? seg_len : n, 1024);
  ws.block_tot.ensure((size_t)nseg * bps);
  ws.block_off.ensure((size_t)nseg * bps);
  hipLaunchKernelGGL(tie_block_sums, dim3(bps, nseg), dim3(1024), 0, j.st, ws.ties.p, n, seg_len, bps, ws.local.p,
                     ws.block_tot.p);
  hipLaunchKernelGGL(tie_block_scan, dim3(nseg), dim3(1024), 0, j.st, ws.block_tot.p, bps, ws.block_off.p);
  const int *rows = j.filtered ? j.rows : nullptr;
  const int nrows = j.filtered ? j.nrows : n;
  if ((long long)j.k * j.s >= 1024) {   // (all but tiny problems) one wave per drawing row: a thread walking k * s products is a long latency chain
    ws.tie_rows.ensure((size_t)std::max(nrows, 1));
    ws.tie_count.ensure(1);
    HIP_CHECK(hipMemsetAsync(ws.tie_count.p, 0, sizeof(unsigned), j.st));
    hipLaunchKernelGGL(collect_tie_rows, dim3(ceil_div(nrows, 256)), dim3(256), 0, j.st, ws.ties.p, rows, nrows,
                       ws.tie_rows.p, ws.tie_count.p);
    hipLaunchKernelGGL(assign_resolve_wave, dim3(1024), dim3(64), sizeof(float) * (size_t)j.s, j.st, j.dX, j.ld, j.from,
                       j.s, ws.cpad.p, smax, ws.off.p, j.k, ws.local.p, ws.block_off.p, seg_len, bps, ws.tie_rows.p,
                       ws.tie_count.p, j.d_assign, (const unsigned long long *)nullptr);
    HIP_CHECK(hipGetLastError());
    return;
  }
  hipLaunchKernelGGL(assign_resolve, dim3(ceil_div(nrows, 256)), dim3(256), 0, j.st, j.dX, n, j.ld, j.from, j.s,
                     ws.cpad.p, smax, ws.off.p, j.k, ws.ties.p, ws.local.p, ws.block_off.p, seg_len, bps, rows, nrows,
                     j.d_assign);
  HIP_CHECK(hipGetLastError());
}

void assign_stage2(AssignJob &j) {
  if (j.done) return;
  KmeansWorkspace &ws = *j.ws;
  if (j.filtered) {
    ws.last_flagged = ws.host->flagged;
    if (ws.host->flagged == 0) { j.done = true; return; }
    j.rows = ws.flag_rows.p;
    j.nrows = (int)ws.host->flagged;
    launch_exact(j);
  } else {
    ws.last_draws = ws.host->total;
    if (ws.host->total) launch_tie_replay(j);
    j.done = true;
  }
}

// stage 3 (after a stream sync; filtered jobs only): tie replay over the flagged rows
void assign_stage3(AssignJob &j) {
  if (j.done) return;
  KmeansWorkspace &ws = *j.ws;
  ws.last_draws = ws.host->total;
  if (ws.host->total && ws.host->total <= SPARSE_TIE_DRAWS && (long long)j.k * j.s >= 1024) {
    launch_tie_replay(j, true);     // few draws: positions from the drawing rows themselves
  } else if (ws.host->total) {
    // draw counts exist only for the flagged rows: build the dense per-row array (0 elsewhere)
    HIP_CHECK(hipMemsetAsync(ws.local.p, 0, sizeof(unsigned) * (size_t)j.n, j.st));
    hipLaunchKernelGGL(scatter_ties, dim3(ceil_div(j.nrows, 256)), dim3(256), 0, j.st, j.rows, j.nrows, ws.ties.p,
                       ws.local.p);
    HIP_CHECK(hipMemcpyAsync(ws.ties.p, ws.local.p, sizeof(unsigned) * (size_t)j.n, hipMemcpyDeviceToDevice, j.st));
    launch_tie_replay(j);
  }
  j.done = true;
}

void kmeans_assign_dev(KmeansWorkspace &ws, const float *dX, int n, int ld, int from, int s, const float *dC, int k,
                       int rng_batch, int *d_assign, hipStream_t st, const PackedSlice *ps) {
  AssignJob j(ws, dX, n, ld, from, s, dC, k, rng_batch, d_assign, st, ps);
  assign_stage1(j);
  if (!j.done) { HIP_CHECK(hipStreamSynchronize(st)); assign_stage2(j); }
  if (!j.done) { HIP_CHECK(hipStreamSynchronize(st)); assign_stage3(j); }
}

// One quantizer of ProductQuantizer.encode (ProductQuantizer.scala:25-35): the serial KMeans.assign of every row's slice
// [from, from + s) against dC [k][s], its Random(0) stream over the rows in order, into d_assign [n].
void pq_assign_quantizer(KmeansWorkspace &ws, PackedSlice &packed, const float *dX, int n, int ld, int from, int s,
                         const float *dC, int k, int *d_assign) {
  HIP_CHECK(hipMemset(d_assign, 0, sizeof(int) * (size_t)n));
  kmeans_assign_dev(ws, dX, n, ld, from, s, dC, k, 0, d_assign, nullptr,
                    pack_slice_if_filtered(dX, n, ld, from, s, k, packed, nullptr));   // serial assign
}

}  // namespace gulon
