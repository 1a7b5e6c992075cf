// The library's internal header: the index handle (gulon_index) with its workspaces and stream ordering, the call and
// output structs of the flat query path (QueryOut, FlatCall), the merge and peel launchers every top-k user shares
// (merge.hip), the tuning knobs, and the launchers the query drivers of scan.hip, wide*.hip, filter*.hip, replay.hip,
// literal.hip and decode.hip call across files.
#pragma once
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <memory>

#include "common.hpp"

struct gulon_index;
namespace gulon {
// Where a query writes: final [B][K] idx / dist (+ count, flags, both nullable), or one partial (K+1)-list per query.
// All members null: a call with no outputs (the phase-1 bounds call, whose bounds go to its SharedBounds).
struct QueryOut {
  int *idx; float *dist; int *count; int *flags; float *part_v; int *part_i;
  static QueryOut final_lists(int *idx, float *dist, int *count, int *flags) {
    return {idx, dist, count, flags, nullptr, nullptr};
  }
  static QueryOut partial_lists(float *v, int *i) { return {nullptr, nullptr, nullptr, nullptr, v, i}; }
  bool final_out() const { return idx != nullptr; }
  // the same outputs, starting at query q0 (null members stay null)
  QueryOut from_query(int q0, int K) const {
    auto at = [](auto *p, size_t o) { return p ? p + o : p; };
    return {at(idx, (size_t)q0 * K), at(dist, (size_t)q0 * K), at(count, (size_t)q0), at(flags, (size_t)q0),
            at(part_v, (size_t)q0 * (K + 1)), at(part_i, (size_t)q0 * (K + 1))};
  }
};
// Merge `lists` sorted partial lists per query (element (l,q,e) at l*stride_l + q*stride_q + e,
// each list K+1 long, padded with (+inf, INT_MAX)) into out: its final lists, else its partial ones.
void launch_merge(const float *in_v, const int *in_i, int lists, long long stride_l, long long stride_q, int B, int K,
                  const QueryOut &out, hipStream_t st);
// large-K peeling (merge.hip): append a 64-entry round to [B][cap] and set the next lower bound; then cut the
// concatenated list to [B][K] + count + tie flags
void launch_peel_update(const float *tv, const int *ti, int B, int round, int cap, float *pv, int *pi, float *lbv,
                        int *lbi, hipStream_t st);
void launch_peel_finalize(const float *pv, const int *pi, int B, int cap, int K, int *out_idx, float *out_dist,
                          int *out_count, int *out_flags, hipStream_t st);
void launch_fill_list(float *v, int *i, long long n, hipStream_t st);   // n entries of (+inf, INT_MAX)
// The rounds of a query for K > GULON_MAX_K neighbours on an index handle: 64 entries per scan round, every round
// restricted to the entries after the previous one's last.  The constructor sizes the handle's peel buffers -- the lists
// [B][cap], one round [tv_slots][64], the bounds [bound_slots] -- and writes the first bounds (nothing returned yet).
struct PeelRounds {
  gulon_index *ix;
  int B, K, rounds, cap;
  hipStream_t st;
  struct Bounds { const float *v; const int *i; };
  PeelRounds(gulon_index *ix, int B, int bound_slots, int tv_slots, int K, hipStream_t st);
  Bounds bounds(int q0) const;   // of queries q0, q0 + 1, ...: what the scan launch of a round reads
  // round r of queries [q0, q0 + nq): their `lists` 64-lists each in ix->part_v / part_i merged, appended, bounds moved
  void append(int r, int q0, int nq, int lists);
  void finish(const QueryOut &out);   // cut to final lists with count and tie flags, or (a shard) to K + 1 partial entries
};
struct ScanTuning;
// Workspace of the expression calls (compose.hip): the term lists, the composed vectors and the index's answer at
// k_nn + extra before the operands are dropped.  `mu` is held for a whole call, so the three steps of a query -- compose,
// the index's own *_dev query, drop -- see one set of buffers; it is taken before the handle's `mu`, never after.
struct ExprWork {
  DevBuf<int> off, rows;       // CSR term lists of the host-pointer forms
  DevBuf<float> w, q;          // their weights; the composed vectors [b][d]
  DevBuf<int> oi, oc;          // the answer at depth k_nn + extra
  DevBuf<float> od;
  DevBuf<int> fi, fc, ff;      // final lists of the host-pointer forms
  DevBuf<float> fd;
  std::mutex mu;
};
// Workspace of the cosmul calls of one handle.  The exact index uses it under its own mutex; the flat index holds `mu`
// for a whole call and takes the handle's mutex inside it, as ExprWork does.
struct CosmulWork {
  DevBuf<int> plan, bad;        // [3]: slots per question E' (1, 2, 4, 8), live term slots, first term; [b]: unusable
  DevBuf<int> uoff, urows;      // the terms as one-term expressions: offsets [tcap + 1], rows [tcap]
  DevBuf<float> ones;           // their weights [tcap]
  DevBuf<float> q, qt;          // the term vectors q_t [tcap][d]; exact: transposed per workgroup [tile][d][16]
  DevBuf<float> tables;         // flat: Index.prepareQuery of every q_t [tcap][m_pad][256]
  DevBuf<float> pv, od;         // per-chunk lists of keys; the merged answer at depth kin
  DevBuf<int> pi, oi, oc;
  DevBuf<int> off, rows, fi, fc;   // the host-pointer forms: term lists and final lists
  DevBuf<float> w, fd;
  std::mutex mu;
};
// Workspace of the offset queries of one handle (offset.hip), under the same two rules.
struct OffsetWork {
  DevBuf<float> qt;             // exact: the queries transposed per workgroup [tile][d][16]
  DevBuf<float> tables;         // flat: Index.prepareQuery of every query [b][m_pad][256]
  DevBuf<float> pv;             // per-chunk lists of keys
  DevBuf<int> pi;
  DevBuf<float> q, off, fd;     // the host-pointer forms: queries, row offsets, final keys
  DevBuf<int> ex, fi, fc;       // ... the excluded rows, final rows and counts
  std::mutex mu;
};
// Workspace of the rank queries of one handle (rank.hip), under the same two rules.
struct RankWork {
  DevBuf<float> qt;             // exact: the queries transposed per workgroup [tile][d][16]
  DevBuf<float> tables;         // flat: Index.prepareQuery of every query [b][m_pad][256]
  DevBuf<float> gk, bk;         // exact: the key of every (query, gold row) pair [G]; the best gold key per query [b]
  DevBuf<int> br, part;         // the best gold row per query [b]; (ahead, total) per (query, row chunk)
  DevBuf<float> q, off, fk;     // the host-pointer forms: queries, row offsets, final keys
  DevBuf<int> ex, goff, grows;  // ... the excluded rows, the gold lists (CSR)
  DevBuf<int> frank, frow, ftotal;   // ... final ranks, rows and totals
  std::mutex mu;
};
}
// PQIndex on the device (opaque to C callers)
using gulon::DevBuf;
struct gulon_index {
  // launch-shape / algorithm knobs of THIS handle: the environment at its creation, then gulon_index_tuning.  Contexts
  // inherit their parent's at creation.
  std::shared_ptr<gulon::ScanTuning> tune;
  int32_t n = 0, d = 0, m = 0, k = 0, row_base = 0;
  int vec = 16, ng = 1, m_pad = 16, nsub = 1, w = 4;   // w: queries interleaved per table entry
  DevBuf<uint8_t> codes;   // [n/64][ng][64][vec]
  // the filter's own copy of one-word codes (m <= 16), rows re-dealt inside every 64-row block for the LDS bank
  // conflicts of its table gathers (conflict_order.hip), and each lane's place in the block's row order
  DevBuf<uint8_t> fcodes, fperm;   // [n/64][64][16], [n/64][64]
  int fwindow = 1;                 // blocks per ordering window of fcodes (4: fperm = place in a 256-row window; 1: in the block)
  // a third copy for the filter stages that cover the whole index: rows in stable ascending order of
  // (code 15 << 8) | code 14, cut into 256-row windows that are dealt to lane groups like fcodes' (conflict_order.hip);
  // sids = the row behind every lane position (-1: padding of the last window)
  DevBuf<uint8_t> scodes;          // [ceil(n/256) * 4][64][16]
  DevBuf<int> sids;                // [ceil(n/256) * 4][64]
  bool wide = false;       // k > 256: 16-bit codes, tables in HBM (wide.hip)
  DevBuf<uint16_t> wcodes; // wide: [n/64][m][64]
  DevBuf<float> wpartial;  // wide, sliced tables: running sums [queries of the sub-batch][rows]
  DevBuf<uint32_t> wpark;  // wide filter, sliced 8-bit tables: byte sums [query group][row block][64 lanes] (wide_filter.hip)
  DevBuf<float> cents;     // k*d
  DevBuf<int> from, sdim;  // m
  // a view (subset.hip): this index holds rows vmap[0] < vmap[1] < ... of another one -- local rows of the root, whose
  // row_base is view_base.  The view-query entries answer view_base + vmap[p]; every other entry answers p.
  bool is_view = false;
  int view_base = 0;
  DevBuf<int> vmap;        // n
  // scratch, grown on demand under `mu`
  DevBuf<float> tables;
  DevBuf<float> part_v;
  DevBuf<int> part_i;
  DevBuf<unsigned> gtau;   // per-query cross-workgroup pruning thresholds (float bits)
  DevBuf<float> stage_q;
  DevBuf<int> stage_oi, stage_oc, stage_of;
  DevBuf<float> stage_od;
  DevBuf<int> flags_scratch;
  DevBuf<int> stage_rows;  // row ids of the host-pointer decode / query-by-row calls (decode.hip)
  DevBuf<int> row_err;     // set by the row decode when a *_dev call asked for a row outside [0, n)
  gulon::ExprWork expr;    // expression queries (compose.hip)
  gulon::CosmulWork cosmul;   // multiplicative analogy queries (cosmul.hip)
  gulon::OffsetWork offset;   // offset queries (offset.hip)
  gulon::RankWork rank;       // rank queries (rank.hip)
  DevBuf<unsigned long long> dbg;   // GULON_REPLAY_STATS stamps (replay.hip)
  // large-K peeling rounds
  DevBuf<float> peel_v, peel_tv, peel_lbv;
  DevBuf<int> peel_i, peel_ti, peel_lbi;
  // exact tie replay (replay.hip)
  DevBuf<int> rp_pack, rp_segcnt, rp_segi, rp_precnt, rp_l0i, rp_l0c;
  DevBuf<float> rp_q, rp_tables, rp_segtop, rp_prefix, rp_l0v;
  DevBuf<int> rp_fb, rp_fini;           // level 2 of the replay through the quantized filter (filter_query.hip)
  DevBuf<int> rp_done;                  // [3][F]: served by rp_shortcut / left to the segment scan / last row that can insert
  DevBuf<int> rp_order;                 // the long level's order of the flagged queries (rp_filter_order)
  DevBuf<float> rp_tau, rp_finv, rp_mins;
  // quantized lower-bound filter (filter.hip)
  DevBuf<float> fin_v, qmins, tau0; // running exact (K+1)-lists [Bq][keff]; table minima [Bq][m_pad]; sample bounds
  DevBuf<int> fin_i, sv_cnt, sv_queue, fb_tile;
  DevBuf<uint8_t> qtab;             // [Bq/16][m_pad][256][16] quantized table entries
  DevBuf<float> nf_tables;          // literal.hip: one fp32 table per workgroup of the non-finite pass
  float cents_absmax = 0.f;         // max |centroid coordinate| (+inf if any is NaN / inf): overflow bound of a query
  // optional hipEvent bracketing of the dominant scan kernel (bench.py roofline line)
  bool profile = false;
  long long prof_rows = 0;          // rows covered by the bracketed launches
  std::vector<std::pair<hipEvent_t, hipEvent_t>> events;   // recorded pairs (events belong to ev_pool)
  std::vector<hipEvent_t> ev_pool;  // created once: hipEventCreate inside the timed region is slow
  size_t ev_next = 0;
  std::mutex mu;
  // gulon_index_scan_bounds_dev -> gulon_index_scan_partial_bounded_dev: arguments of the pending first half
  int pend_b = -1, pend_k = -1, pend_from = -1, pend_until = -1;
  // host-mapped word the filter's fallback launch sets when it had anything to do: sizes the next one
  int *fb_hint_h = nullptr, *fb_hint_d = nullptr;
  int *rp_hint_h = nullptr, *rp_hint_d = nullptr;   // host-mapped: flagged queries of a recent batch (replay.hip)
  int fb_wide_left = 0;   // launches that stay wide after the word was last seen set
  int last_filter_tiles = 0;   // query tiles of the last filtered batch on this handle (0: it took the exact scan)
  // ---- query contexts (gulon_index_context_create): a context BORROWS the read-only members of its parent
  // (codes, wcodes, cents, from, sdim) and owns every scratch buffer above, so batches in flight on
  // different streams / threads never share device scratch.  The parent stays alive until its last context
  // is destroyed (refs).
  gulon_index *parent = nullptr;
  std::atomic<int> refs{1};
  // one handle = one workspace: the device work of consecutive calls on DIFFERENT streams is ordered through
  // this event (two batches in flight on one handle are serialised on the device, never corrupted)
  hipEvent_t order_ev = nullptr;
  hipStream_t order_st = nullptr;
  bool order_set = false;
  // host-pointer calls (gulon_index_batch_query) from several threads -- the reference's recall harness does
  // that (Tests.scala:109-122) -- run concurrently on lazily created internal contexts, each with its own stream
  std::mutex host_mu;
  std::condition_variable host_cv;
  std::vector<gulon_index *> host_all, host_free;   // internal contexts (owned); the handle itself is the first
  bool host_self_busy = false;
  hipStream_t host_stream = nullptr;
  hipEvent_t take_event() {
    if (ev_next == ev_pool.size()) {
      hipEvent_t e = nullptr;
      HIP_CHECK(hipEventCreate(&e));
      ev_pool.push_back(e);
    }
    return ev_pool[ev_next++];
  }
  ~gulon_index() {
    for (auto *c : host_all) delete c;
    for (auto &e : ev_pool) (void)hipEventDestroy(e);
    if (fb_hint_h) (void)hipHostFree(fb_hint_h);
    if (rp_hint_h) (void)hipHostFree(rp_hint_h);
    if (order_ev) (void)hipEventDestroy(order_ev);
    if (host_stream) (void)hipStreamDestroy(host_stream);
  }
};

namespace gulon {
// a new workspace over `parent`'s read-only data (no reference counting: the caller keeps `parent` alive)
gulon_index *make_context(gulon_index *parent);
// index_handle.hip, host-pointer calls: take a free workspace of this handle (the handle itself first), creating up to
// GULON_HOST_CONTEXTS (default 4) internal contexts; blocks while all are busy
gulon_index *acquire_host_context(gulon_index *idx);
void release_host_context(gulon_index *idx, gulon_index *c);
// scan.hip: the bodies of gulon_index_batch_query_dev / gulon_index_batch_query; map_view (a view only): the returned
// positions are translated to the root's row ids on the same stream, inside the handle's StreamOrder
void batch_query_dev_on(gulon_index *idx, const float *d_queries, int32_t b, int32_t k_nn, int32_t from, int32_t until,
                        int32_t *d_out_idx, float *d_out_dist, int32_t *d_out_count, int32_t *d_out_flags,
                        hipStream_t st, bool map_view);
void batch_query_host_on(gulon_index *idx, const float *queries, int32_t b, int32_t k_nn, int32_t from, int32_t until,
                         int32_t *out_idx, float *out_dist, int32_t *out_count, int32_t *out_flags, bool map_view);
// index_handle.hip: the filter's conflict-ordered copy of ix->codes, where this handle's tuning and shape call for one
void build_filter_copy(gulon_index *ix);
// subset.hip: d_idx[0..count) positions of `view` -> row ids of its root, in place; negative entries stay
void launch_map_rows(const gulon_index *view, int *d_idx, long long count, hipStream_t st);
// RAII: order this call's device work after the previous call's on the same handle when the stream differs
struct StreamOrder {
  gulon_index *ix;
  hipStream_t st;
  StreamOrder(gulon_index *ix_, hipStream_t st_) : ix(ix_), st(st_) {
    if (!ix->order_ev) HIP_CHECK(hipEventCreateWithFlags(&ix->order_ev, hipEventDisableTiming));
    if (ix->order_set && ix->order_st != st) HIP_CHECK(hipStreamWaitEvent(st, ix->order_ev, 0));
  }
  bool recorded = false;
  void done() {
    HIP_CHECK(hipEventRecord(ix->order_ev, st));
    mark();
  }
  void mark() {
    ix->order_st = st;
    ix->order_set = true;
    recorded = true;
  }
  // a call that throws after it enqueued part of its work on the handle's scratch never reaches done(): the next call
  // on another stream still has to wait for what was launched
  ~StreamOrder() {
    if (!recorded && hipEventRecord(ix->order_ev, st) == hipSuccess) mark();
  }
  StreamOrder(const StreamOrder &) = delete;
  StreamOrder &operator=(const StreamOrder &) = delete;
};

// Strided selection of row blocks: the e-th eligible block (relative to the first block of the
// scanned range) is (e / width) * period + lo + e % width.  {1, 0, 1} = every block.
struct RbMap { int period, lo, width; };
inline int rbmap_count(int rb_total, RbMap mp) {
  int extra = rb_total % mp.period - mp.lo;
  extra = extra < 0 ? 0 : extra > mp.width ? mp.width : extra;
  return (rb_total / mp.period) * mp.width + extra;
}

// launch shape knobs (the environment at index creation / gulon_index_tuning: for experiments and tests)
// filter.hip: of the 16 quantizers of a one-word code, the entries of the last GULON_FILTER_GLB are fetched through
// the vector L1 instead of LDS; conflict_order.hip orders rows for the bank conflicts of the others
#ifndef GULON_FILTER_GLB
#define GULON_FILTER_GLB 3
#endif
constexpr int FILTER_LDS_QUANTIZERS = 16 - GULON_FILTER_GLB;
// the same for the key-sorted copy, where the look-ups of the two sorted quantizers cost the vector L1 half of a random
// one (scripts/micro/l1_gather.hip): one more goes through it
#ifndef GULON_FILTER_SORT_GLB
#define GULON_FILTER_SORT_GLB 4
#endif
constexpr int FILTER_SORT_LDS_QUANTIZERS = 16 - GULON_FILTER_SORT_GLB;

// filter.hip: the main stage on the key-sorted copy tests a row on this many of its sixteen quantizers (the two sorted
// ones through the vector L1, the others from LDS) before it looks up the rest.  Measured at 10 M rows, five alternating
// runs each: 9 -> 1.814 ms per batch, 10 -> 1.797, 11 -> 1.810 (without: 2.268); profiles/r05/configs.md
constexpr int FILTER_PREFIX_P = 10;

struct ScanTuning {
  int threads = 1024;        // workgroup size (16 waves hide the pruning checkpoints' LDS drain)
  int target_blocks = 4096;  // workgroups per launch aimed for
  int prune = 1;             // exact early termination on/off
  int prune_from = -1;       // first quantizer index with a pruning checkpoint (-1: m_pad/2)
  int filter = 1;            // quantized lower-bound filter on/off
  int filter_min_rb = 512;   // smallest range (in 64-row blocks) the filter is used for
  int filter_period = 128;   // row blocks per sampling period
  int filter_sample = 65536; // most sample rows whose exact distances give the initial bounds
  int filter_stage0 = 0;     // blocks per period scanned by an extra first filter stage (0: none)
  int filter_stage1 = 10;    // blocks per period scanned by the second filter stage (6 until round 2: 2.44 -> 2.38 ms per
                             // batch at 10 M rows, 0.497 -> 0.469 at 1.25 M; flat from 10 to 20)
  int filter_cap = 32768;    // survivor queue entries per query and stage
  int filter_nadd = 0;       // table entries summed in 8 bits before widening (2: 7-bit, 4: 6-bit levels, 0: by m)
  int filter_blocks = 4096;         // workgroups aimed for by a filter launch
  int filter_shared_stage1 = -1;    // bounds shared across shards: run the short first stage? (-1: by sample size)
  int filter_order = 1;             // conflict-ordered code copy: built at index creation (the environment's value) / used (per handle)
  int filter_sort = 1;              // key-sorted code copy: built at index creation (the environment's value) / used (per handle)
  int filter_prefix = FILTER_PREFIX_P;   // main stage on the key-sorted copy: quantizers tested before a row's other look-ups (0: off)
  ScanTuning();
  bool set(const char *key, int v);
};
const ScanTuning &tuning_defaults();
inline const ScanTuning &tuning_of(const gulon_index *ix) { return ix && ix->tune ? *ix->tune : tuning_defaults(); }

// One batch query over rows [from, until) of a flat (byte-coded or wide) index: what run_query and every driver under
// it take.  sb: the shared-bounds half this call is (nullptr: an ordinary query).
struct SharedBounds;
struct FlatCall {
  gulon_index *ix; const float *dQ; int B, K, from, until; QueryOut out; hipStream_t st; const SharedBounds *sb;
};
// The chunks of a scan launch over row_blocks 64-row blocks: about `want` of them, but at least two row blocks for each
// of a workgroup's `waves` waves
inline void scan_chunks(int row_blocks, int want, int waves, int &nchunks, int &per_chunk) {
  nchunks = std::max(1, std::min(want, row_blocks / (2 * waves)));
  per_chunk = ceil_div(row_blocks, nchunks);
  nchunks = ceil_div(row_blocks, per_chunk);
}

// wide.hip: indexes with more than 256 centroids per quantizer (code widths 10/12/16)
constexpr int WIDE_THREADS = 512;              // scan_wide's workgroup: one partial list per wave
constexpr int WIDE_NW = WIDE_THREADS / 64;
void wide_store_codes(gulon_index *ix, const uint16_t *wide16 /* device, [m][n] */);
void launch_build_tables_wide(const float *cents, const int *from, const int *sdim, int d, int m, int k, const float *dQ,
                              int q0, int nq, float *tables /*[nq][m][k]*/, hipStream_t st);
// wide_filter.hip: the quantized lower-bound filter for 16-bit code words (k <= 1024 at m = 16)
bool wide_filter_eligible(const gulon_index *ix, int B, int K, int rb_total);
void run_wide_filter_query(const FlatCall &c);
void launch_scan_wide_range(gulon_index *ix, int B, int K, int from, int until, int rb_begin, int rb_total,
                            int rb_per_chunk, int nchunks, const int *enable, hipStream_t st);
void run_wide_query(const FlatCall &c);

// scan.hip: exact scan of the selected row blocks of [from, until) into ix->part_v/part_i
// ([query][nchunks][keff]); tile_enable (device, per query tile) skips disabled tiles.
void launch_scan(gulon_index *ix, int ntiles, int nchunks, int rb_begin, int e_count, int e_per_chunk, RbMap mp,
                 int from, int until, int keff, hipStream_t st, const float *lbv = nullptr, const int *lbi = nullptr,
                 const int *tile_enable = nullptr, bool one_sub = false, int grid_x = 0, int *hint = nullptr);
// merge_lists<false> restricted to the queries of enabled tiles (fallback of the filter)
void launch_merge_enabled(const float *in_v, const int *in_i, int lists, long long stride_l, long long stride_q, int B,
                          int K, float *out_pv, int *out_pi, const int *tile_enable, int qt, hipStream_t st);
// ---- the quantized lower-bound filter of byte codes: kernels and one launcher per kernel in filter.hip, the query
// driver, level 2 of the tie replay and the stage hook in filter_query.hip ----
constexpr size_t FILTER_LDS_BUDGET = 144 * 1024;
#ifndef GULON_FILTER_THREADS
#define GULON_FILTER_THREADS 1024
#endif
constexpr int FILTER_THREADS = GULON_FILTER_THREADS;   // filter_kernel's workgroup
constexpr int NSLOT = 16;   // survivor sub-queues per query (workgroups of different chunks use different ones)
// the launch shape run_filter_query and replay_level2_filtered share
struct FilterShape {
  int qw, nqg;      // queries per quantized table entry, entry groups per workgroup
  int nadd, qmax;   // table entries summed in 8 bits before widening, the top quantisation level
  int cap;          // entries per survivor sub-queue
  int slots;        // filter workgroups the chip holds at once
};
FilterShape filter_shape(const gulon_index *ix);
int device_cus();   // compute units of the current device (cached per ordinal, lock-free)
// the first block and the number of blocks a filter launch over rows [from, until) scans: whole ordering windows
void filter_block_range(const gulon_index *ix, int qw, int nqg, int nadd, int from, int until, int &rb_begin,
                        int &rb_total);
int filter_sample_rows(const ScanTuning &t, int rb_total);   // rows of the sample scan over rb_total row blocks
// per device: the event the main-stage launches take turns through; `fresh` = this call created it (nothing to wait for)
hipEvent_t filter_lane_event(int dev, bool &fresh);
// bound_tables, the batch's first kernel: counters, Index.prepareQuery into ix->tables / ix->qmins, and the sample
// bounds of [from, until) into ix->tau0 (and bounds_out, where given), which also resets ix->fin_v / ix->fin_i
void launch_bound_tables(gulon_index *ix, const float *dQ, int B, int Bp, int Bq, int ntiles, int keff, int from,
                         int until, int rb_begin, int rb_total, float *bounds_out, hipStream_t st);
void launch_shared_tau(gulon_index *ix, const float *all_bounds, int lists, int B, int keff, hipStream_t st);
// qt_quantize: ix->qtab for Bq queries from `tables` (W-interleaved) and `mins` against min(tau0, a full list's last)
void launch_qt_quantize(gulon_index *ix, const float *tables, int W, int Bp, int B, int Bq, const float *mins,
                        const float *fin_v, const int *fin_i, const float *tau0, int keff, int qmax, int qw, int *fb,
                        int qt, const int *slot, hipStream_t st);
void launch_filter(gulon_index *ix, int qw, int nqg, int nadd, int ftiles, int nchunks, int rb_begin, int e_count,
                   int e_per_chunk, RbMap mp, int from, int until, int cap, int stage, int B, hipStream_t st,
                   int *fb = nullptr /* tile flags other than the index's own, one per `qt` queries */, int qt = 1,
                   bool sorted = false /* read the key-sorted copy (the launch covers every row of the index) */,
                   int prefix = 0 /* sorted main stage: quantizers of the prefix test (filter.hip), 0: none */);
// survivors_kernel: the queued rows re-evaluated exactly and merged into ix->fin_v / ix->fin_i
void launch_survivors(gulon_index *ix, int B, int Bq, int keff, int cap, int give_up, hipStream_t st);
// filter_query.hip: level 2 of the tie replay (replay.hip) through the quantized filter.  For the flagged queries f < *count
// (tables [f][m_pad][256] with their minima `mins`, bounds = the K-th of prefix_v[f][K] when prefix_c[f] >= K) every
// row of blocks [rb_lo, rb_hi) with an exact distance BELOW the bound is appended to the query's candidate pool
// (evv / evi / evcnt, `pool` entries per query).  only[f] is left 0 for the queries served here and 1 for those the
// caller's segment scan still has to do (fewer than `min_flagged` flagged queries, unusable bound, queue overflow).
// Returns false (nothing enqueued) when this index does not take the filter.
bool replay_level2_filtered(gulon_index *ix, int F, int K, int rb_lo, int rb_hi, int from, int until,
                            const float *tables, const float *mins, const float *prefix_v, const int *prefix_c,
                            const int *count, float *evv, int *evi, int *evcnt, int pool, int **only, hipStream_t st,
                            const int *done, const int *rlast, int *scanme);
// filter.hip: does this index and range take the filter?
bool filter_eligible(const gulon_index *ix, int K, int rb_total);
// Bounds shared across row shards (sharded.py): phase 1 stops after the sample scan and writes the K+1
// smallest sample distances per query ([B][K+1], ascending, +inf padded) to bounds_out; phase 2 resumes
// with the `lists` gathered arrays ([lists][B][K+1]) -- the (K+1)-th smallest of their union bounds the
// (K+1)-th distance of the WHOLE index, so every shard filters against the global bound.
struct SharedBounds { int phase; float *bounds_out; const float *all_bounds; int lists; };
// filter_query.hip: sample scan -> quantized filter stages -> exact re-evaluation of the survivors.
void run_filter_query(const FlatCall &c);

#ifdef __HIPCC__
template <int VEC> struct CodeWord;
template <> struct CodeWord<4> { using type = uint32_t; };
template <> struct CodeWord<16> { using type = uint4; };
template <int VEC>
__device__ inline uint32_t code_byte(const typename CodeWord<VEC>::type &w, int b);
template <>
__device__ inline uint32_t code_byte<4>(const uint32_t &w, int b) { return (w >> (8 * b)) & 0xFFu; }
template <>
__device__ inline uint32_t code_byte<16>(const uint4 &w, int b) {
  uint32_t x = (b < 4) ? w.x : (b < 8) ? w.y : (b < 12) ? w.z : w.w;
  return (x >> (8 * (b & 3))) & 0xFFu;
}
// 32-bit word `seg` of a code word (seg need not be a constant: no register array is indexed)
template <int VEC>
__device__ __forceinline__ uint32_t code_word32(const typename CodeWord<VEC>::type &w, int seg);
template <>
__device__ __forceinline__ uint32_t code_word32<4>(const uint32_t &w, int) { return w; }
template <>
__device__ __forceinline__ uint32_t code_word32<16>(const uint4 &w, int seg) {
  return seg == 0 ? w.x : seg == 1 ? w.y : seg == 2 ? w.z : w.w;
}
#endif

// Index.prepareQuery tables, W queries interleaved (scan.hip)
void launch_build_tables(int W, gulon_index *ix, const float *dQ, int B, int Bpad, float *tables, hipStream_t st,
                         const int *live_queries = nullptr, float *mins = nullptr);
// literal.hip: queries whose distances can be NaN / +inf are redone through the literal TopKHeap over all rows
float centroid_absmax(const float *d_cents, long long count);
// (over the call's final outputs; `flags`: the flags array the pass reads and updates, nullable)
void run_nonfinite_literal(const FlatCall &c, int *flags);
// For every query flagged with an exact distance tie, recompute the result with the
// reference's TopKHeap semantics (insertion history in row order) -- replay.hip
void run_tie_replay(const FlatCall &c, int *flags);
// scan.hip: the tail of every query path that is not peeled -- `lists` sorted lists per query merged into the call's
// outputs, then, over final ones, the tie replay and (literal_pass) the non-finite literal pass.  The byte-coded paths
// pass literal_pass = true; the wide paths pass false: they have never run that pass, and unifying the tail did not
// change that.  A driver that merges in sub-batches (run_wide_query) calls the two halves itself: its merges write to
// merge_outputs(c).from_query(q0, K), and finish_replay gets merge_outputs(c).flags.
void finish_query(const FlatCall &c, const float *in_v, const int *in_i, int lists, long long stride_l,
                  long long stride_q, bool literal_pass);
// c.out as the merge writes it: final outputs with the replay on need the tie flags even if the caller does not, and
// take the handle's scratch for them
QueryOut merge_outputs(const FlatCall &c);
void finish_replay(const FlatCall &c, int *flags, bool literal_pass);
void launch_conflict_order(const uint8_t *src, uint8_t *dst, uint8_t *perm, long long nblk, int nq, int rounds,
                           hipStream_t st);
bool conflict_order_windowed();   // the ordering spans windows of four blocks (default) or single blocks
// conflict_order.hip: the key-sorted copy of n one-word rows -- dst [ceil(n/256) * 256] code words, ids [the same] rows
void launch_sorted_copy(const uint8_t *codes, int n, uint8_t *dst, int *ids, int rounds, hipStream_t st);
// decode.hip: rows of the index back into vectors (ProductQuantizer.decode, GroupedIndex.lookup).  gcent != nullptr:
// out = gcent[partition] + decode(row), the partition by Arrays.binarySearch over offsets[0..n_offsets); normalize:
// MathUtils.normalize of the result.  d_rows / d_out are device pointers; rows outside [0, n) give NaN rows and set
// *d_err (nullable).  launch_decode_range: rows [from, until) into d_out [until - from][d].
void launch_decode_rows(const gulon_index *ix, const int *d_rows, int b, const float *gcent, const int *offsets,
                        int n_offsets, bool normalize, float *d_out, int *d_err, hipStream_t st);
void launch_decode_range(const gulon_index *ix, int from, int until, float *d_out, hipStream_t st);
// host rows (checked: GULON_ERR_INVALID_ARGUMENT before any launch) -> host out, through the given scratch; synchronises
void decode_rows_host(const gulon_index *ix, DevBuf<int> &rows_buf, DevBuf<float> &out_buf, const int32_t *rows, int b,
                      const float *gcent, const int *offsets, int n_offsets, bool normalize, float *out, hipStream_t st);
void ensure_row_err(gulon_index *ix);   // the handle's row_err word, allocated and zeroed: when the handle is made
int take_row_err(gulon_index *ix);      // synchronises; returns and clears it
// grouped.hip: what compose.hip needs of a GroupedIndex handle (the struct is private to grouped.hip) -- the residual
// index, the group centroids, the raw offsets GroupedIndex.lookup searches, and the handle's mutex; for inspect.hip the
// groups' row ranges: group c holds rows [bounds[c], bounds[c + 1]), c < g
struct GroupedParts {
  gulon_index *pq; const float *gcent; const int *offsets; int n_offsets; std::mutex *mu;
  const int *bounds; int g;
};
GroupedParts grouped_parts(gulon_grouped_index *idx);
}  // namespace gulon
