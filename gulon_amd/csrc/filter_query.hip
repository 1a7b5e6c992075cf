// The host side of the quantized lower-bound filter (kernels and launchers: filter.hip): the query driver
// run_filter_query as named steps on a FilterBatch, level 2 of the tie replay through the filter, and the stage hook of
// tests/test_gpu_filter_stage.py, which is built from the same steps.
#include <vector>

#include "scan.hpp"
#include "select.hpp"

namespace gulon {

namespace {

// ---- level 2 of the tie replay through the filter (replay_level2_filtered below) ---------------------------------
// One workgroup: the flagged queries in the order the long level serves them.  Compact position c -> slot order[c]:
// the live ones (finite K-th distance over the earlier rows, not served by rp_shortcut, enough flagged queries for a
// launch) first, by the last row that can still insert (`rlast`, replay.hip) -- a query tile then walks the rows up to
// ITS largest such row only, and tiles of queries that need no rows at all are skipped -- then the ones left to the
// segment scan (fb = 1) and the served ones (fb = 2).  tau / fb / fin in compact order; lim[tile] = last row block.
__global__ __launch_bounds__(1024) void rp_filter_order(const int *__restrict__ count, int F, int min_flagged, int K,
                                                        const float *__restrict__ prefix_v, const int *__restrict__ prefix_c,
                                                        const int *__restrict__ done, const int *__restrict__ rlast,
                                                        int row_base, int n_pad, int tile_q, int ntiles, int *__restrict__ order,
                                                        float *__restrict__ tau, int *__restrict__ fb,
                                                        float *__restrict__ fin_v, int *__restrict__ fin_i,
                                                        int *__restrict__ lim /* [n_pad / tile_q] */) {
  __shared__ unsigned long long key[1024];
  const int t = threadIdx.x;
  const int nf = min(*count, F);
  {
    // class 0: live, by last row block; 1: left to the scan; 2: served; 3: not a flagged query
    unsigned long long cls = 3, sub = 0;
    if (t < nf) {
      const bool served = done && done[t] != 0;
      const bool live = !served && nf >= min_flagged && prefix_c[t] >= K && prefix_v[(size_t)t * K + K - 1] < INFINITY;
      cls = live ? 0 : served ? 2 : 1;
      if (live) {
        const int last = rlast ? rlast[t] : INT_MAX;
        sub = last == INT_MAX ? 0x3FFFFFFFull : (unsigned long long)max(0, (last - row_base) >> 6);   // (no result at hand: every row)
      }
    }
    key[t] = (cls << 60) | (sub << 12) | (unsigned long long)t;
  }
  __syncthreads();
  for (int k2 = 2; k2 <= 1024; k2 <<= 1)
    for (int j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
      const int o = t ^ j2;
      if (o > t) {
        const unsigned long long a = key[t], b = key[o];
        const bool up = (t & k2) == 0;
        if ((a > b) == up) { key[t] = b; key[o] = a; }
      }
      __syncthreads();
    }
  if (t < n_pad) {
    const unsigned long long kk = key[t];
    const int cls = (int)(kk >> 60), f = (int)(kk & 0xFFF);
    const bool live = cls == 0;
    order[t] = cls == 3 ? 0 : f;
    tau[t] = live ? prefix_v[(size_t)f * K + K - 1] : INFINITY;
    fb[t] = live ? 0 : cls == 2 ? 2 : 1;       // (padding slots: 1, but no query behind them)
    fin_v[t] = INFINITY;                       // a one-entry "running list" that never tightens the bound
    fin_i[t] = INT_MAX;
  }
  if (t < ntiles) {                            // the tile's largest limit = that of its last live entry (sorted)
    int l = -1;
    for (int c = t * tile_q; c < min(n_pad, (t + 1) * tile_q); c++) {
      const unsigned long long kk = key[c];
      if ((kk >> 60) == 0) l = (int)min((unsigned long long)INT_MAX, (kk >> 12) & 0xFFFFFFFFFFFFull);
    }
    lim[t] = l;
  }
}

// the survivors of flagged query f, exactly (the reference's j-ordered unfused sum from the query's fp32 table):
// those below the bound go to the candidate pool of the literal heap.  A query whose queue overflowed emits nothing
// and is left to the segment scan.
template <int VEC>
__global__ __launch_bounds__(256) void rp_filter_emit(const uint8_t *__restrict__ codes, int ng, int m_pad,
                                                      const float *__restrict__ tables /*[f][m_pad][256]*/, int row_base,
                                                      int *__restrict__ cnt, const int *__restrict__ queue, int cap,
                                                      const int *__restrict__ count, int F, const float *__restrict__ tau,
                                                      int *__restrict__ fb, float *__restrict__ evv, int *__restrict__ evi,
                                                      int *__restrict__ evcnt, int pool, const int *__restrict__ order,
                                                      int *__restrict__ scanme /* [slot]: 1 = left to the segment scan */) {
  using Word = typename CodeWord<VEC>::type;
  // compact position fc (queues, bounds, flags) -> slot f (tables, candidate pool)
  const int fc = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  SurvivorQueues<NSLOT> sq(cnt, fc, lane);
  __syncthreads();                                  // every wave has read the counters
  sq.clear(tid < NSLOT);
  if (fc >= min(*count, F)) return;
  const int f = order[fc];
  if (fb[fc] != 0) {
    if (tid == 0) scanme[f] = fb[fc] == 1;
    return;
  }
  if (sq.overflowed(cap)) {
    if (tid == 0) { fb[fc] = 1; scanme[f] = 1; }    // a sub-queue overflowed
    return;
  }
  if (tid == 0) scanme[f] = 0;
  const int n = sq.count();
  auto entry = [&](int e) { return sq.entry(queue, fc, cap, e); };
  const float bound = tau[fc];
  const float *tq = tables + (size_t)f * m_pad * 256;
  const Word *cw = reinterpret_cast<const Word *>(codes);
  for (int e = tid; e - lane < n; e += 256) {
    const bool have = e < n;
    const int row = have ? entry(e) : 0;
    float d = 0.f;
    for (int g = 0; g < ng; g++) {
      const Word w = cw[((size_t)(row >> 6) * ng + g) * 64 + (row & 63)];
#pragma unroll
      for (int b = 0; b < VEC; b++) d += tq[(size_t)(g * VEC + b) * 256 + code_byte<VEC>(w, b)];
    }
    const bool emit = have && d < bound;            // TopKHeap.update inserts only below its root (strict)
    const unsigned long long mk = __ballot(emit);
    if (mk) {
      int base = 0;
      if (lane == 0) base = atomicAdd(&evcnt[f], (int)__popcll(mk));
      base = readlane_i(base, 0);
      const int pos = base + (int)__popcll(mk & ((1ull << lane) - 1ull));
      if (emit && pos < pool) { evv[(size_t)f * pool + pos] = d; evi[(size_t)f * pool + pos] = row + row_base; }
    }
  }
}

// One batch through the filter: what run_filter_query works out once (plan) and the launches of its steps.  The stage
// hook below runs the same plan / filter_workspace / sample_bounds / quantize / filter with a bound, a stage and a chunk
// rule of its own.
struct FilterBatch {
  gulon_index *ix;
  const ScanTuning &t;
  const float *dQ;
  int B, keff, from, until;
  hipStream_t st;
  // plan
  int W, QT, ntiles, Bp;            // fp32 table interleave of the exact kernels, queries per tile flag, tiles, padded batch
  FilterShape fs;
  int cap;                          // entries per survivor sub-queue (fs.cap; the hook: its caller's)
  int ftiles, Bq;                   // filter tiles; the batch as whole 16-query quantisation groups
  int rb_begin, rb_total;           // the row blocks of [from, until) ...
  int frb_begin, frb_total;         // ... and what the filter launches scan (whole ordering windows)
  bool sorted;                      // the stages read the key-sorted copy
  RbMap stages[3];
  int NW, srows;
  int fb_tiles, pfb, cfb_n;         // the fallback scan: tiles, row blocks per chunk, chunks

  explicit FilterBatch(const FlatCall &c)
      : ix(c.ix), t(tuning_of(c.ix)), dQ(c.dQ), B(c.B), keff(c.K + 1), from(c.from), until(c.until), st(c.st) {}
  void plan(const SharedBounds *sb);
  void filter_workspace(bool fallback_too);
  void sample_bounds(float *bounds_out);
  void chunking(int e_count, int &nchunks, int &per) const;
  void quantize();
  void filter(RbMap mp, int en, int nchunks, int per, bool main_stage);
  void stage(int sidx, bool stats);
  void fallback_scan();
  void print_stage_stats(int sidx, int en, int nc) const;
  void print_fallback_stats() const;
};

void FilterBatch::plan(const SharedBounds *sb) {
  W = ix->w;
  QT = W * ix->nsub;
  ntiles = ceil_div(B, QT);
  Bp = ntiles * QT;
  fs = filter_shape(ix);
  cap = fs.cap;
  ftiles = ceil_div(B, fs.qw * fs.nqg);
  Bq = ceil_div(ftiles * fs.nqg * fs.qw, 16) * 16;
  rb_begin = from / 64;
  rb_total = ceil_div(until, 64) - rb_begin;
  frb_begin = rb_begin, frb_total = rb_total;
  filter_block_range(ix, fs.qw, fs.nqg, fs.nadd, from, until, frb_begin, frb_total);
  // the stages of a query over every row of the index read the key-sorted copy, whole 256-row windows of it
  sorted = ix->scodes.p && ix->sids.p && t.filter_sort > 0 && ix->ng == 1 && ix->vec == 16 && fs.qw == 16 &&
           fs.nqg == 1 && fs.nadd == 4 && from == 0 && until == ix->n;
  if (sorted) {
    frb_begin = 0;
    frb_total = ceil_div(ix->n, 256) * 4;
  }
  const int P = t.filter_period;
  const int s0 = std::min(std::max(t.filter_stage0, 0), P - 2);
  const int s1 = std::min(std::max(t.filter_stage1, 1), P - 1 - s0);
  stages[0] = RbMap{P, 0, s0};
  stages[1] = RbMap{P, s0, s1};
  stages[2] = RbMap{P, s0 + s1, P - s0 - s1};
  NW = t.threads / 64;
  srows = filter_sample_rows(t, rb_total);
  if (sb && sb->phase == 2) {
    // bounds shared by `lists` shards: their union is a sample `lists` times this shard's; once that
    // is about half the rows of the short stages, these stages cost more launches than they save survivors
    // (one rank of 2 / 4 / 8 on the bench index: 1.950 / 1.136 / 0.526 ms with them, 1.944 / 1.074 / 0.496 without)
    const long long early = ((long long)rbmap_count(frb_total, stages[0]) + rbmap_count(frb_total, stages[1])) * 64;
    const bool keep = t.filter_shared_stage1 < 0 ? 2LL * sb->lists * srows < early : t.filter_shared_stage1 != 0;
    if (!keep) {
      stages[0].width = 0;
      stages[1].width = 0;
      stages[2] = RbMap{P, 0, P};
    }
  }
  // fallback launch: W-query tiles with ONE sub-table (<= 64 KiB of LDS, like a filter workgroup).  The index's
  // preferred two-sub-table workgroup needs both LDS halves of a CU at once, which another batch's filter
  // kernel never leaves free: the (normally empty) launch then waited for that whole kernel -- up to 3 ms
  // of its batch's critical path (rocprofv3: 1.31 ms on average for a launch that takes 4.7 us)
  fb_tiles = ntiles * ix->nsub;
  const int cfb = std::max(1, ceil_div(256, fb_tiles));   // one workgroup per CU when everything is redone
  pfb = ceil_div(rb_total, cfb);
  cfb_n = ceil_div(rb_total, pfb);
}

// (the allocation sequence decides where the buffers lie: one order, with or without the fallback's partial lists)
void FilterBatch::filter_workspace(bool fallback_too) {
  ix->tables.ensure((size_t)Bp * ix->m_pad * 256);
  if (fallback_too) {
    ix->part_v.ensure((size_t)Bp * cfb_n * keff);
    ix->part_i.ensure((size_t)Bp * cfb_n * keff);
  }
  ix->gtau.ensure((size_t)Bp);
  ix->fin_v.ensure((size_t)Bq * keff);
  ix->fin_i.ensure((size_t)Bq * keff);
  ix->qmins.ensure((size_t)Bq * ix->m_pad);
  ix->qtab.ensure((size_t)Bq * ix->m_pad * 256);
  ix->sv_cnt.ensure((size_t)Bq * NSLOT);
  ix->sv_queue.ensure((size_t)Bq * NSLOT * cap);
  ix->fb_tile.ensure((size_t)ntiles);
  ix->tau0.ensure((size_t)Bp);
}

void FilterBatch::sample_bounds(float *bounds_out) {
  launch_bound_tables(ix, dQ, B, Bp, Bq, ntiles, keff, from, until, rb_begin, rb_total, bounds_out, st);
}

// chunks per query tile: enough workgroups to fill the chip, but every workgroup stages its
// 64-128 KiB of tables once (268 MB through L2 for 4096 workgroups), so it should get >= 768 row blocks
// (48 per wave) where the range allows; the launch is a whole number of rounds of what the chip holds
// at once (CUs x resident workgroups) where that is possible
void FilterBatch::chunking(int e_count, int &nchunks, int &per) const {
  const int most = std::max(1, ceil_div(t.filter_blocks, ftiles));   // launch-size cap
  const int fill = std::max(1, ceil_div(fs.slots, ftiles));          // every slot of the chip taken once
  int nc = std::max(fill, std::min(most, e_count / 768));
  if (nc > fill) nc -= nc % fill;                                    // whole rounds
  nc = std::min(nc, std::max(1, e_count / NW));                      // at least one block per wave
  per = ceil_div(e_count, nc);
  nchunks = ceil_div(e_count, per);
}

void FilterBatch::quantize() {   // the tables against the current bounds: the sample's, or a full running list's last entry
  launch_qt_quantize(ix, ix->tables.p, W, Bp, B, Bq, ix->qmins.p, ix->fin_v.p, ix->fin_i.p, ix->tau0.p, keff, fs.qmax,
                     fs.qw, ix->fb_tile.p, QT, nullptr, st);
}

void FilterBatch::filter(RbMap mp, int en, int nchunks, int per, bool main_stage) {
  launch_filter(ix, fs.qw, fs.nqg, fs.nadd, ftiles, nchunks, frb_begin, en, per, mp, from, until, cap, main_stage ? 1 : 0,
                B, st, nullptr, 1, sorted, sorted ? t.filter_prefix : 0);
}

// one stage: quantize -> filter (the main stage in its turn on the device, and timed where the handle profiles) ->
// survivors
void FilterBatch::stage(int sidx, bool stats) {
  const RbMap mp = stages[sidx];
  const int en = rbmap_count(frb_total, mp);
  if (en <= 0) return;
  int nc = 1, per = 1;
  chunking(en, nc, per);
  quantize();
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  const bool main_stage = sidx == 2;
  // a first stage that keeps more than ~3 % of its (query, row) pairs means the bounds do not
  // separate anything for this query: give up on it before the main stage
  const int give_up = main_stage ? 0 : std::max(256, (int)std::min<long long>((long long)en * 64 * 3 / 100, 1 << 30));
  const bool timed = ix->profile && main_stage;   // the roofline line is about the main-stage kernel
  if (timed) {
    ev0 = ix->take_event();
    ev1 = ix->take_event();
  }
  {
    int dev = 0;
    HIP_CHECK(hipGetDevice(&dev));
    bool fresh = false;
    const hipEvent_t lane_ev = filter_lane_event(dev, fresh);
    // only the main stage takes turns.  (Two host threads enqueueing at the same instant may both wait for the SAME
    // earlier launch and then share the chip once: the event orders launches for throughput, never for results.)
    // (ranges below ~2 M rows -- a shard of an 8-GPU index -- do better without the turn-taking: 0.413 against 0.430 ms
    // per batch at 1.25 M rows, three batches in flight; 10 M rows: 2.36 against 2.38, within the noise, and the
    // kernel durations the bench reports stay those of one kernel at a time)
    const bool turns = (long long)rb_total * 64 >= (2ll << 20);
    if (main_stage && !fresh && turns) HIP_CHECK(hipStreamWaitEvent(st, lane_ev, 0));
    if (timed) HIP_CHECK(hipEventRecord(ev0, st));         // after the wait: the kernel's own duration
    filter(mp, en, nc, per, main_stage);
    if (main_stage) HIP_CHECK(hipEventRecord(lane_ev, st));
  }
  if (stats) print_stage_stats(sidx, en, nc);
  if (timed) {
    HIP_CHECK(hipEventRecord(ev1, st));
    ix->events.emplace_back(ev0, ev1);
    ix->prof_rows += std::min<long long>((long long)en * 64, (long long)until - from);
  }
  launch_survivors(ix, B, Bq, keff, cap, give_up, st);
}

// fallback (device-side decision): flagged query tiles are rescanned exactly over all rows
void FilterBatch::fallback_scan() {
  if (!ix->fb_hint_h) {
    HIP_CHECK(hipHostMalloc(reinterpret_cast<void **>(&ix->fb_hint_h), sizeof(int), hipHostMallocMapped));
    *ix->fb_hint_h = 0;
    HIP_CHECK(hipHostGetDevicePointer(reinterpret_cast<void **>(&ix->fb_hint_d), ix->fb_hint_h, 0));
  }
  // a hint, read without synchronisation: did a recent fallback launch of this index find work?
  // (launches are enqueued ahead of their execution, so the word lags by the batches in flight: once seen,
  // it keeps the next 8 launches wide, and every launch that finds work arms it again)
  volatile int *hint = ix->fb_hint_h;
  if (*hint != 0) { *hint = 0; ix->fb_wide_left = 8; }
  const bool wide = ix->fb_wide_left > 0;
  if (wide) ix->fb_wide_left--;
  launch_scan(ix, fb_tiles, cfb_n, rb_begin, rb_total, pfb, RbMap{1, 0, 1}, from, until, keff, st, nullptr, nullptr,
              ix->fb_tile.p, true, wide ? fb_tiles : 8, ix->fb_hint_d);
  launch_merge_enabled(ix->part_v.p, ix->part_i.p, cfb_n, (long long)keff, (long long)cfb_n * keff, B, keff - 1,
                       ix->fin_v.p, ix->fin_i.p, ix->fb_tile.p, QT, st);
}

// debugging aid (GULON_FILTER_STATS=1): synchronous survivor statistics of a stage ...
void FilterBatch::print_stage_stats(int sidx, int en, int nc) const {
  HIP_CHECK(hipStreamSynchronize(st));
  std::vector<int> h((size_t)Bq * NSLOT);
  HIP_CHECK(hipMemcpy(h.data(), ix->sv_cnt.p, sizeof(int) * h.size(), hipMemcpyDeviceToHost));
  long long tot = 0; int mx = 0;
  for (int v : h) { tot += v; mx = std::max(mx, v); }
  fprintf(stderr, "[filter] stage %d: %d row blocks, %d x %d workgroups, survivors total %lld (%.3g of pairs), "
          "max per sub-queue %d (cap %d)\n", sidx + 1, en, ftiles, nc, tot, (double)tot / ((double)en * 64 * B), mx, cap);
}
// ... and how many query tiles the exact scan redid
void FilterBatch::print_fallback_stats() const {
  HIP_CHECK(hipStreamSynchronize(st));
  std::vector<int> h((size_t)ntiles);
  HIP_CHECK(hipMemcpy(h.data(), ix->fb_tile.p, sizeof(int) * h.size(), hipMemcpyDeviceToHost));
  int nfb = 0;
  for (int v : h) nfb += v != 0;
  fprintf(stderr, "[filter] %d of %d query tiles redone by the exact scan\n", nfb, ntiles);
}

}  // namespace

void run_filter_query(const FlatCall &c) {
  gulon_index *ix = c.ix;
  const SharedBounds *sb = c.sb;
  const int phase = sb ? sb->phase : 0;
  FilterBatch fb(c);
  fb.plan(sb);
  fb.filter_workspace(true);
  ix->last_filter_tiles = fb.ntiles;
  if (phase != 2) fb.sample_bounds(phase == 1 ? sb->bounds_out : nullptr);
  if (phase == 1) return;     // the caller exchanges the bounds and comes back with phase 2
  if (phase == 2) launch_shared_tau(ix, sb->all_bounds, sb->lists, c.B, fb.keff, c.st);
  const bool stats = getenv("GULON_FILTER_STATS") != nullptr;
  for (int sidx = 0; sidx < 3; sidx++) fb.stage(sidx, stats);
  fb.fallback_scan();
  if (stats) fb.print_fallback_stats();
  finish_query(c, ix->fin_v.p, ix->fin_i.p, 1, 0LL, (long long)fb.keff, true);
}

bool replay_level2_filtered(gulon_index *ix, int F, int K, int rb_lo, int rb_hi, int from, int until,
                            const float *tables, const float *mins, const float *prefix_v, const int *prefix_c,
                            const int *count, float *evv, int *evi, int *evcnt, int pool, int **only, hipStream_t st,
                            const int *done, const int *rlast, int *scanme /* [F]: written for every flagged slot */) {
  const ScanTuning &t = tuning_of(ix);
  const int level_from = std::max(from, rb_lo * 64);     // the level's rows: nothing of the earlier levels is emitted again
  int e_count = rb_hi - rb_lo;
  // (the same conditions as filter_eligible; the byte-code kernels only)
  if (!t.filter || ix->wide || (size_t)ix->m_pad * 256 * 4 > FILTER_LDS_BUDGET || e_count < t.filter_min_rb || K < 1)
    return false;
  const FilterShape fs = filter_shape(ix);
  const int qw = fs.qw, nqg = fs.nqg, nadd = fs.nadd, cap = fs.cap;
  filter_block_range(ix, qw, nqg, nadd, rb_lo * 64, std::min(until, rb_hi * 64), rb_lo, e_count);   // whole ordering windows
  const int ftiles = ceil_div(F, qw * nqg);
  const int Fq = ceil_div(ftiles * nqg * qw, 16) * 16;
  // a launch is worth its fixed costs (quantisation, table staging of every workgroup) from about two query tiles on
  const int min_flagged = 2 * qw;
  GULON_REQUIRE(F <= 1024, "internal: %d flagged queries per replay round", F);
  const int tile_q = qw * nqg;
  ix->rp_fb.ensure((size_t)Fq + ftiles); ix->rp_fini.ensure((size_t)Fq);
  ix->rp_tau.ensure((size_t)Fq); ix->rp_finv.ensure((size_t)Fq);
  ix->rp_order.ensure((size_t)Fq);
  ix->qtab.ensure((size_t)Fq * ix->m_pad * 256);
  ix->sv_cnt.ensure((size_t)Fq * NSLOT);
  ix->sv_queue.ensure((size_t)Fq * NSLOT * cap);
  hipLaunchKernelGGL(rp_filter_order, dim3(1), dim3(1024), 0, st, count, F, min_flagged, K, prefix_v, prefix_c, done, rlast,
                     ix->row_base, Fq, tile_q, ftiles, ix->rp_order.p, ix->rp_tau.p, ix->rp_fb.p, ix->rp_finv.p, ix->rp_fini.p,
                     ix->rp_fb.p + Fq);
  HIP_CHECK(hipMemsetAsync(ix->sv_cnt.p, 0, sizeof(int) * (size_t)Fq * NSLOT, st));
  // tables of the flagged queries are [slot][m_pad][256]: "one query per entry" (W = 1) in qt_quantize's terms, read
  // through the order; queries beyond F (the padding of the last 16-query group) read no table
  launch_qt_quantize(ix, tables, 1, F, F, Fq, mins, ix->rp_finv.p, ix->rp_fini.p, ix->rp_tau.p, 1, fs.qmax, qw, ix->rp_fb.p,
                     1, ix->rp_order.p, st);
  const int NW = FILTER_THREADS / 64;
  int nc = std::max(1, std::min(std::max(ceil_div(fs.slots, ftiles), e_count / 768), std::max(1, e_count / NW)));
  const int per = ceil_div(e_count, nc);
  nc = ceil_div(e_count, per);
  const RbMap all{1, 0, 1};
  launch_filter(ix, qw, nqg, nadd, ftiles, nc, rb_lo, e_count, per, all, level_from, until, cap, 2, F, st, ix->rp_fb.p, 1);
  auto emit = ix->vec == 16 ? rp_filter_emit<16> : rp_filter_emit<4>;
  hipLaunchKernelGGL(emit, dim3(F), dim3(256), 0, st, ix->codes.p, ix->ng, ix->m_pad, tables, ix->row_base, ix->sv_cnt.p,
                     ix->sv_queue.p, cap, count, F, ix->rp_tau.p, ix->rp_fb.p, evv, evi, evcnt, pool, ix->rp_order.p, scanme);
  HIP_CHECK(hipGetLastError());
  *only = scanme;
  return true;
}

}  // namespace gulon

#ifdef GULON_TEST_HOOKS
using namespace gulon;

// ONE filter stage on its own, over every row block of [from, until), for tests/test_gpu_filter_stage.py: what the stage
// queues per query and the levels it quantized, against bounds the caller chooses.  The hook builds its own index (handle
// and hook share this library's statics) and runs run_filter_query's own steps on a FilterBatch -- plan, the filter half
// of the workspace, sample_bounds (tables, minima, counters; the bound of its sample is overwritten with `tau`, the running
// lists stay empty), quantize, filter -- with the whole range as one stage, a chunk rule of its own and no survivors
// kernel.  copy: 0 the plain codes, 1 the conflict-ordered copy, 2 the key-sorted copy (one-word codes with nadd = 4
// only; 2: the whole row range only).
// rows_out [b][16 cap]: the queued rows of a query, ascending (entries beyond a full sub-queue are lost, as in
// production); counts_out [b][16]: the sub-queues' fill counters, unclamped; flagged_out [b]: the flag of the query's
// tile; levels_out [b][m][k]: the 8-bit levels of the real quantizers and centroids; info: qmax, m_pad, queries per
// flag, queries per table entry, entry groups per workgroup, chunks launched.
// (Declared here and bound by its test: the header's list of hooks is pinned by test_abi.)
GULON_API int32_t gulon_selftest_filter_stage(const uint8_t *codes, int32_t n, int32_t d, int32_t m, int32_t k,
                                              const float *cents, const float *queries, int32_t b, int32_t from,
                                              int32_t until, const float *tau, int32_t copy, int32_t nadd, int32_t cap,
                                              int32_t main_stage, int32_t *rows_out, int32_t *counts_out,
                                              int32_t *flagged_out, uint8_t *levels_out, int32_t *info) {
  gulon_index *raw = nullptr;
  const int32_t rc = guarded([&] {
    GULON_REQUIRE(codes && cents && queries && tau && rows_out && counts_out && flagged_out && levels_out && info, "null argument");
    GULON_REQUIRE(k >= 1 && k <= 256 && b >= 1 && b <= 4096 && from >= 0 && from < until && until <= n && copy >= 0 && copy <= 2 &&
                  (nadd == 2 || nadd == 4) && cap >= 1 && cap <= (1 << 16), "bad arguments");
    GULON_REQUIRE(gulon_index_create(codes, n, d, m, k, cents, 0, &raw) == GULON_OK && raw, "no index");
    gulon_index *ix = raw;
    GULON_REQUIRE((size_t)ix->m_pad * 256 * 4 <= FILTER_LDS_BUDGET, "no filter for m = %d", m);
    ScanTuning &t = *ix->tune;   // the copy is chosen through the tuning, as a caller of the library would
    t.filter_nadd = nadd;
    t.filter_min_rb = 4;
    t.filter_order = copy == 1 ? std::max(1, t.filter_order) : 0;
    t.filter_sort = copy == 2;
    if (copy != 0) {
      GULON_REQUIRE(ix->vec == 16 && ix->ng == 1 && nadd == 4, "no ordered copy of this index");
      GULON_REQUIRE(copy == 1 || (from == 0 && until == n), "the key-sorted copy serves the whole range only");
      build_filter_copy(ix);
    }
    hipStream_t st = nullptr;
    FilterBatch fb(FlatCall{ix, nullptr, b, 10, from, until, QueryOut{}, st, nullptr});   // lists of keff = 11
    fb.plan(nullptr);
    GULON_REQUIRE(fb.fs.nadd == nadd, "internal: nadd");
    GULON_REQUIRE(fb.sorted == (copy == 2), "internal: copy");
    fb.cap = cap;
    fb.filter_workspace(false);
    DevBuf<float> dQ;
    dQ.upload(queries, (size_t)b * d, st);
    fb.dQ = dQ.p;
    fb.sample_bounds(nullptr);
    HIP_CHECK(hipMemcpyAsync(ix->tau0.p, tau, sizeof(float) * (size_t)b, hipMemcpyHostToDevice, st));
    fb.quantize();
    const int en = fb.frb_total, qw = fb.fs.qw;
    // the main-stage tag: chunks long enough for every wave to draw runs (all sixteen sub-queues fill, as in production);
    // the short-stage tag: many short chunks, whose first few waves take all the runs
    int nc = std::max(1, std::min(ceil_div(fb.fs.slots, fb.ftiles), en / (main_stage ? 4 * fb.NW : fb.NW)));
    const int per = ceil_div(en, nc);
    nc = ceil_div(en, per);
    fb.filter(RbMap{1, 0, 1}, en, nc, per, main_stage != 0);
    HIP_CHECK(hipStreamSynchronize(st));
    export_survivor_queues(ix->sv_cnt.p, ix->sv_queue.p, NSLOT, fb.Bq, b, cap, ix->row_base, rows_out, counts_out);
    std::vector<int> flags((size_t)fb.ntiles);
    std::vector<uint8_t> qt((size_t)fb.Bq * ix->m_pad * 256);
    HIP_CHECK(hipMemcpy(flags.data(), ix->fb_tile.p, sizeof(int) * flags.size(), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(qt.data(), ix->qtab.p, qt.size(), hipMemcpyDeviceToHost));
    for (int q = 0; q < b; q++) {
      flagged_out[q] = flags[q / fb.QT];
      for (int j = 0; j < m; j++)      // entry (j, c) of query q: byte q % QW of entry [q / QW][j][c] (qt_quantize)
        for (int c = 0; c < k; c++)
          levels_out[((size_t)q * m + j) * k + c] = qt[((((size_t)(q / qw)) * ix->m_pad + j) * 256 + c) * qw + q % qw];
    }
    info[0] = fb.fs.qmax; info[1] = ix->m_pad; info[2] = fb.QT; info[3] = qw; info[4] = fb.fs.nqg; info[5] = nc;
  });
  if (raw) (void)gulon_index_destroy(raw);
  return rc;
}
#endif
