// KMeans / ProductQuantizer on gfx950 (KMeans.scala, ProductQuantizer.scala): the training driver and the C ABI.
//
//   train    KMeans.computeClusters loop for a batch of independent problems
//            (ProductQuantizer.apply = m problems, seed = quantizer index).
// The assign is kmeans_assign.hip (exact) behind kmeans_mfma.hip (filter); the update kmeans_stream.hip (k <= 1024) or
// kmeans_update.hip (bucketed).
#include "kmeans.hpp"

#include <chrono>

namespace gulon {

__global__ void gather_centroids(const float *__restrict__ X, int ld, int from, int s, const int *__restrict__ rows,
                                 int k, float *__restrict__ C) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= k * s) return;
  int c = t / s, j = t - c * s;
  C[t] = X[(size_t)rows[c] * ld + from + j];
}

__global__ void count_mismatch(const int *__restrict__ a, const int *__restrict__ b, int n,
                               unsigned *__restrict__ out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  bool diff = i < n && a[i] != b[i];
  // plain store of a constant: no atomic needed, and no contention when every wave differs
  if (__ballot(diff) && (threadIdx.x & 63) == 0) *out = 1u;
}

__global__ void copy_slice(const float *__restrict__ X, int ld, int from, int s, long long total,
                           float *__restrict__ out) {
  long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  long long r = t / s;
  int j = (int)(t - r * s);
  out[t] = X[(size_t)r * ld + from + j];
}

__global__ void narrow_assign_u8(const int *__restrict__ a, long long n, uint8_t *__restrict__ out) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (uint8_t)a[i];
}

static void validate_assignments(const int32_t *a, int n, int k) {
  for (int i = 0; i < n; i++)
    GULON_REQUIRE(a[i] >= 0 && a[i] < k, "assignment %d at row %d is outside [0,%d)", a[i], i, k);
}

// SummaryStats builder over MathUtils.distance(prev_c, next_c) (KMeans.scala:160-168,
// MathUtils.scala:43-57,85-98): k values, host side.
static void step_stats(const float *prev, const float *next, int k, int s, gulon_kmeans_report *r) {
  int n = 0;
  float m = 0.f, ss = 0.f;
  for (int c = 0; c < k; c++) {
    float sum = 0.f;
    for (int j = 0; j < s; j++) {
      float dx = next[(size_t)c * s + j] - prev[(size_t)c * s + j];
      sum += dx * dx;
    }
    float x = (float)std::sqrt((double)sum);
    n += 1;
    float m0 = m;
    m = m0 + (x - m0) / (float)n;
    ss = ss + (x - m0) * (x - m);
  }
  r->step_count = n;
  r->step_mean = m;
  r->step_s = ss;
}

TrainTrace &train_trace() { static TrainTrace t; return t; }

// Stage timing of kmeans_train_batch (GULON_TRACE=1 prints it, gulon_kmeans_trace collects it): a device synchronisation
// closes every stage, so the stages of the m concurrent problems are timed as a whole, one after the other.
struct StageClock {
  const bool print = getenv("GULON_TRACE") != nullptr;
  TrainTrace &tt = train_trace();
  const bool on = print || tt.on;
  double t_mark = now();
  static double now() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
  }
  void lap(const char *what, double *acc = nullptr) {
    if (!on) return;
    (void)hipDeviceSynchronize();
    double t = now();
    if (print) fprintf(stderr, "[gulon trace] %-28s %8.2f ms\n", what, t - t_mark);
    if (acc && tt.on) *acc += t - t_mark;
    t_mark = t;
  }
};

// KMeans.computeClusters (KMeans.scala:134-157) for `np` independent problems
// (from[p], s[p], seed[p]) over the same n x ld data, run iteration-synchronously: every
// problem owns a stream and a workspace, so the small latency-bound kernels (sequential
// update chains, sorts, tie replays) of different sub-quantizers overlap on the GPU.
// One method per timed stage; kmeans_train_batch below is the sequence.
class TrainBatch {
 public:
  TrainBatch(const float *dX, int n, int ld, int np, const int *from, const int *sdim, int k,
             gulon_kmeans_report *reports, int max_reports)
      : dX(dX), n(n), ld(ld), np(np), from(from), sdim(sdim), k(k), reports(reports), max_reports(max_reports), P(np) {}
  TrainBatch(const TrainBatch &) = delete;
  TrainBatch &operator=(const TrainBatch &) = delete;
  ~TrainBatch() {
    if (upd_done) (void)hipEventDestroy(upd_done);
    if (bst) (void)hipStreamDestroy(bst);
  }
  void setup(const int *seeds);        // alloc + init + pack + stage 1 of the first assign
  void first_assign();
  bool select_active();                // false: every problem has converged
  void update();                       // one batched update of the active problems
  void launch_assigns();               // stage 1 of every active problem's assign, behind the update
  void finish_assigns() { finish_assigns(act); clock.lap("  assign stages 2-3", &clock.tt.recheck_ms); }
  void count_rechecks();               // (tracing only)
  void order_ahead();                  // the next update's chunk order, under the convergence test
  bool converge(int i);                // mismatch + reports; true: every active problem converged
  void results(float *const *c_out, int32_t *n_reports);

 private:
  struct Prob {
    KmeansWorkspace ws;
    hipStream_t st = nullptr;
    hipEvent_t assigned = nullptr;   // this problem's assignment of the iteration is final
    DevBuf<float> c_prev, c_next;
    DevBuf<int> a_prev, a_next, d_rows;
    DevBuf<unsigned> mism;
    // host copies of the centroids and of the mismatch counter: PINNED, so that the per-iteration downloads of all
    // problems are truly asynchronous (into pageable memory every hipMemcpyAsync stages and blocks: 64 of them were
    // most of the "convergence test" stage)
    float *h_prev = nullptr, *h_next = nullptr;
    unsigned *h_mism = nullptr;
    PackedSlice packed;                 // MFMA-ready copy of this problem's column slice
    const PackedSlice *ps = nullptr;    // &packed where the MFMA filter takes the shape
    DevBuf<float> xs;                   // row-major n x s copy of the slice: compact target of the update's gathers
    StreamSlice stream;                 // the streamed update's copy and scratch (kmeans_stream.hip)
    AssignJob job;
    bool done = false;
    bool shared_stream = false;
    int nrep = 0;
    ~Prob() {
      if (assigned) (void)hipEventDestroy(assigned);
      if (st && !shared_stream) (void)hipStreamDestroy(st);
    }
  };
  // ONE pinned allocation for all problems' host copies (a hipHostMalloc costs milliseconds: three per problem were
  // 1.5 s of a 32-quantizer training)
  struct PinnedBlock {
    void *p = nullptr;
    ~PinnedBlock() { if (p) (void)hipHostFree(p); }
  };

  void alloc_host_copies();
  bool stream_update_fits() const;
  void setup_problem(int p, int seed);
  void finish_assigns(const std::vector<int> &which);
  std::vector<StreamDesc> stream_descs(bool next) const;
  void push_report(int p, const gulon_kmeans_report &r) {
    if (reports && P[p].nrep < max_reports) reports[(size_t)p * max_reports + P[p].nrep] = r;
    P[p].nrep++;
  }
  void make_job(int p, const float *dC, int *d_assign) {
    Prob &pr = P[p];
    pr.job = AssignJob(pr.ws, dX, n, ld, from[p], sdim[p], dC, k, 25000, d_assign, pr.st, pr.ps);
  }

  StageClock clock;
  const float *dX;
  const int n, ld, np;
  const int *from, *sdim;
  const int k;
  gulon_kmeans_report *reports;
  const int max_reports;
  std::vector<Prob> P;
  PinnedBlock pinned;
  DevBuf<UpdDesc> d_descs;
  DevBuf<StreamDesc> d_sdescs, d_odescs;
  bool order_ready = false;      // stream_order has already run on the current a_prev of every active problem
  bool stream_update = true;     // every problem through kmeans_stream.hip (all or none: one batched launch pair)
  hipStream_t bst = nullptr;     // the batch stream: the updates
  hipEvent_t upd_done = nullptr;
  std::vector<int> act;          // the problems still iterating
};

void TrainBatch::alloc_host_copies() {
  size_t words = 0;
  for (int p = 0; p < np; p++) words += 2 * (size_t)k * sdim[p] + 1;
  HIP_CHECK(hipHostMalloc(&pinned.p, sizeof(float) * std::max<size_t>(words, 1)));
  float *w = static_cast<float *>(pinned.p);
  for (int p = 0; p < np; p++) {
    P[p].h_prev = w; w += (size_t)k * sdim[p];
    P[p].h_next = w; w += (size_t)k * sdim[p];
    P[p].h_mism = reinterpret_cast<unsigned *>(w); w += 1;
  }
}

// The streamed update keeps a second, pair-major copy of every slice (+ 4 bytes of order per row): it is taken only
// where that fits beside the slices and the assign's packed operands with a quarter of the device's memory to spare.
// Per problem and row, the first term is StreamSlice: 8 bytes per pair of dimensions (xp) and 4 for ord and coff (which
// take 2 and, at k = 1024, 0.25: the rest is slack).  The second is what setup_problem allocates either way: xs (4 s),
// the filter's packed operands at their widest (PackedSlice::xq, five words of 16 bytes for each of the two lanes a row
// has a share in: 160), and a_prev, a_next, ws.ties, ws.local (16).  The spare quarter once also had to hold the
// bucketed update's scratch, which every training allocated (xb, 4 bytes per row and dimension rounded up to even;
// hist, gtot, corder): a streamed training no longer has it (KmeansWorkspace::ensure_update), so that much of the
// quarter is slack now.  The formula stays as it was: it decides which update a training takes.
bool TrainBatch::stream_update_fits() const {
  size_t need = 0, free_b = 0, total_b = 0;
  for (int p = 0; p < np; p++) need += (size_t)stream_padded_rows(n) * (8 * (size_t)((sdim[p] + 1) / 2) + 4);
  for (int p = 0; p < np; p++) need += (size_t)n * (4 * (size_t)sdim[p] + 160 + 16);
  HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
  return !(need + total_b / 4 > free_b);
}

void TrainBatch::setup_problem(int p, int seed) {
  const int s = sdim[p];
  Prob &pr = P[p];
  // GULON_KMEANS_SERIAL=1 (profiling): every problem on the batch stream, so that kernels run one at a time and
  // rocprofv3's per-kernel durations are not inflated by the other sub-quantizers' concurrent launches
  static const bool serial = getenv("GULON_KMEANS_SERIAL") != nullptr;
  if (serial) { pr.st = bst; pr.shared_stream = true; }
  else HIP_CHECK(hipStreamCreateWithFlags(&pr.st, hipStreamNonBlocking));
  HIP_CHECK(hipEventCreateWithFlags(&pr.assigned, hipEventDisableTiming));
  pr.c_prev.alloc((size_t)k * s); pr.c_next.alloc((size_t)k * s);
  pr.a_prev.alloc(n); pr.a_next.alloc(n);
  pr.mism.alloc(1);
  // KMeans.init (KMeans.scala:188-196)
  std::vector<int> rows(k);
  JRandom rng((int64_t)seed);
  for (int c = 0; c < k; c++) rows[c] = rng.next_int(n);
  pr.d_rows.alloc(k);
  HIP_CHECK(hipMemcpy(pr.d_rows.p, rows.data(), sizeof(int) * k, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(gather_centroids, dim3(ceil_div((long long)k * s, 256)), dim3(256), 0, pr.st, dX, ld, from[p], s,
                     pr.d_rows.p, k, pr.c_prev.p);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemsetAsync(pr.a_prev.p, 0, sizeof(int) * (size_t)n, pr.st));
  pr.xs.alloc((size_t)n * s);
  GULON_UNSUPPORTED((long long)n * s >= (1ll << 32), "slice of %lld elements: a dispatch carries fewer than 2^32 work-items",
                    (long long)n * s);
  hipLaunchKernelGGL(copy_slice, dim3(ceil_div((long long)n * s, 256)), dim3(256), 0, pr.st, dX, ld, from[p], s,
                     (long long)n * s, pr.xs.p);
  // the matrix-core operands from the COMPACT copy: the strided slices of the row-major data cost a partial line per
  // row and pass (pack_slice_split 1.0 ms per sub-quantizer at BASELINE config 3 from the rows, 0.3 from the copy)
  pr.ps = pack_slice_if_filtered(pr.xs.p, n, s, 0, s, k, pr.packed, pr.st);
  if (stream_update) pr.stream.prepare(pr.xs.p, n, s, k, pr.st);
  make_job(p, pr.c_prev.p, pr.a_prev.p);
  assign_stage1(pr.job);
  push_report(p, gulon_kmeans_report{0, 0, 0, 0.f, 0.f});
}

void TrainBatch::setup(const int *seeds) {
  alloc_host_copies();
  d_descs.alloc(np); d_sdescs.alloc(np); d_odescs.alloc(np);
  for (int p = 0; p < np; p++) stream_update = stream_update && stream_update_supported(n, k, sdim[p]);
  if (stream_update) stream_update = stream_update_fits();
  HIP_CHECK(hipStreamCreateWithFlags(&bst, hipStreamNonBlocking));
  HIP_CHECK(hipEventCreateWithFlags(&upd_done, hipEventDisableTiming));
  for (int p = 0; p < np; p++) setup_problem(p, seeds[p]);
  clock.lap("alloc+pack+stage1");
}

// run stages 2 and 3 of every listed problem, one synchronisation round per stage.  (Measured and dropped: a few
// host threads issuing the ~300 short launches of these stages side by side -- 4.3 ms against 4.1 ms with one: the
// stage is not bound by the host's launch rate.)
void TrainBatch::finish_assigns(const std::vector<int> &which) {
  for (int stage = 2; stage <= 3; stage++) {
    bool pending = false;
    for (int p : which) pending |= !P[p].job.done;
    if (!pending) break;
    for (int p : which) if (!P[p].job.done) HIP_CHECK(hipStreamSynchronize(P[p].st));
    for (int p : which) { if (stage == 2) assign_stage2(P[p].job); else assign_stage3(P[p].job); }
  }
}

void TrainBatch::first_assign() {
  std::vector<int> all(np);
  for (int p = 0; p < np; p++) all[p] = p;
  finish_assigns(all);
  for (int p = 0; p < np; p++) {
    P[p].c_prev.download(P[p].h_prev, (size_t)k * sdim[p], P[p].st);
    HIP_CHECK(hipStreamSynchronize(P[p].st));
  }
  clock.lap("first assign done");
  if (clock.print) {
    unsigned long long dr = 0;
    for (int p = 0; p < np; p++) dr += P[p].ws.last_draws;
    fprintf(stderr, "[gulon trace]   first assign: tie draws %llu\n", dr);
  }
}

bool TrainBatch::select_active() {
  act.clear();
  for (int p = 0; p < np; p++) if (!P[p].done) act.push_back(p);
  return !act.empty();
}

// the active problems' descriptors for the update that reads a_prev, or (next) for the order of a_next
std::vector<StreamDesc> TrainBatch::stream_descs(bool next) const {
  std::vector<StreamDesc> sd;
  for (int p : act) sd.push_back(P[p].stream.desc(next ? P[p].a_next.p : P[p].a_prev.p, P[p].c_next.p));
  return sd;
}

// one batched update for all active problems, then every problem's assign on its own stream.  (Measured and
// dropped: the update in staggered groups of problems -- a group's chains under the next group's regrouping, its
// assign under the next chains, so that the first assign starts after a quarter of the update: 12 iterations at
// BASELINE config 3 take 0.66 s with one group, 0.71 / 0.79 / 0.93 s with 2 / 4 / 8 -- the memory-bound regrouping
// and the assign slow each other down by more than the overlap saves.)
void TrainBatch::update() {
  if (stream_update) {
    const std::vector<StreamDesc> sd = stream_descs(false);
    // (sd is read by hipMemcpyAsync from pageable memory: staged before the calls return)
    if (!order_ready) kmeans_stream_order(sd, d_odescs.p, n, k, bst);
    kmeans_stream_chains(sd, d_sdescs.p, n, k, bst);
    order_ready = false;
  } else {
    std::vector<UpdDesc> descs;
    for (int p : act)
      descs.push_back(make_upd_desc(P[p].ws, P[p].xs.p, sdim[p], n, k, 0, sdim[p], P[p].a_prev.p, P[p].c_next.p));
    kmeans_update_batch(descs, d_descs.p, n, k, bst);
  }
  HIP_CHECK(hipEventRecord(upd_done, bst));
  clock.lap("  update batch", &clock.tt.update_ms);
}

void TrainBatch::launch_assigns() {
  for (int p : act) {
    Prob &pr = P[p];
    HIP_CHECK(hipStreamWaitEvent(pr.st, upd_done, 0));
    HIP_CHECK(hipMemsetAsync(pr.a_next.p, 0, sizeof(int) * (size_t)n, pr.st));   // fresh Array[Int] per parAssign
    make_job(p, pr.c_next.p, pr.a_next.p);
    assign_stage1(pr.job);
  }
  clock.lap("  assign stage1", &clock.tt.assign_ms);
}

void TrainBatch::count_rechecks() {
  if (!clock.on) return;
  TrainTrace &tt = clock.tt;
  unsigned long long fl = 0, dr = 0;
  double fm = 0, ub = 0;
  for (int p : act) {
    fl += P[p].ws.last_flagged; dr += P[p].ws.last_draws;
    if (P[p].ps) fm += 2.0 * n * k * sdim[p];
    ub += 4.0 * n * sdim[p];
  }
  if (clock.print)
    fprintf(stderr, "[gulon trace]   rows re-checked exactly %llu of %llu (%.3g), tie draws %llu\n", fl,
            (unsigned long long)n * act.size(), (double)fl / ((double)n * act.size()), dr);
  if (tt.on) {
    tt.iterations++; tt.rows_rechecked += fl; tt.rows_total += (unsigned long long)n * act.size();
    tt.mfma_flops += fm; tt.update_bytes += ub;
  }
}

// The next update's chunk order depends on nothing but this assignment: it runs now, on the batch stream, under
// the convergence test's downloads and host round trip (~1 ms in which the GPU was idle).  Wasted only in the
// iteration that finds every problem converged.
void TrainBatch::order_ahead() {
  if (!stream_update) return;
  for (int p : act) {
    HIP_CHECK(hipEventRecord(P[p].assigned, P[p].st));
    HIP_CHECK(hipStreamWaitEvent(bst, P[p].assigned, 0));
  }
  kmeans_stream_order(stream_descs(true), d_odescs.p, n, k, bst);
  order_ready = true;
}

bool TrainBatch::converge(int i) {
  for (int p : act) {
    Prob &pr = P[p];
    HIP_CHECK(hipMemsetAsync(pr.mism.p, 0, sizeof(unsigned), pr.st));
    hipLaunchKernelGGL(count_mismatch, dim3(ceil_div(n, 256)), dim3(256), 0, pr.st, pr.a_prev.p, pr.a_next.p, n,
                       pr.mism.p);
    pr.c_next.download(pr.h_next, (size_t)k * sdim[p], pr.st);
    pr.mism.download(pr.h_mism, 1, pr.st);
  }
  for (int p : act) HIP_CHECK(hipStreamSynchronize(P[p].st));
  bool all_conv = true;
  for (int p : act) {
    Prob &pr = P[p];
    bool converged = *pr.h_mism == 0;                      // Arrays.equals(prev, next)
    gulon_kmeans_report r{i, converged ? 1 : 0, 0, 0.f, 0.f};
    step_stats(pr.h_prev, pr.h_next, k, sdim[p], &r);
    push_report(p, r);
    std::swap(pr.c_prev, pr.c_next);
    std::swap(pr.a_prev, pr.a_next);
    std::swap(pr.h_prev, pr.h_next);
    if (converged) pr.done = true; else all_conv = false;
  }
  clock.lap("  mismatch+reports", &clock.tt.converge_ms);
  return all_conv;
}

void TrainBatch::results(float *const *c_out, int32_t *n_reports) {
  for (int p = 0; p < np; p++) {
    memcpy(c_out[p], P[p].h_prev, sizeof(float) * (size_t)k * sdim[p]);
    if (n_reports) n_reports[p] = P[p].nrep;
  }
}

// c_out[p] receives k x s[p] floats.
void kmeans_train_batch(const float *dX, int n, int ld, int np, const int *from, const int *sdim, const int *seeds,
                        int k, int max_iterations, float *const *c_out, gulon_kmeans_report *reports,
                        int max_reports, int32_t *n_reports) {
  GULON_REQUIRE(n >= 1, "KMeans.init needs at least one row (n = %d)", n);   // rng.nextInt(0) throws on the JVM
  TrainBatch tb(dX, n, ld, np, from, sdim, k, reports, max_reports);
  tb.setup(seeds);
  tb.first_assign();
  for (int i = 0; i <= max_iterations && tb.select_active(); i++) {
    tb.update();
    tb.launch_assigns();
    tb.finish_assigns();
    tb.count_rechecks();
    if (i < max_iterations) tb.order_ahead();
    if (tb.converge(i)) break;
  }
  tb.results(c_out, n_reports);
}

}  // namespace gulon

using namespace gulon;

GULON_API int32_t gulon_kmeans_trace(int32_t enable) {
  return guarded([&] {
    TrainTrace &t = train_trace();
    t = TrainTrace();
    t.on = enable != 0;
  });
}

GULON_API int32_t gulon_kmeans_trace_read(gulon_kmeans_trace_totals *out) {
  return guarded([&] {
    GULON_REQUIRE(out != nullptr, "out is null");
    const TrainTrace &t = train_trace();
    out->iterations = t.iterations;
    out->update_ms = t.update_ms; out->assign_ms = t.assign_ms; out->recheck_ms = t.recheck_ms;
    out->converge_ms = t.converge_ms;
    out->mfma_flops = t.mfma_flops; out->update_bytes = t.update_bytes;
    out->rows_rechecked = (double)t.rows_rechecked; out->rows_total = (double)t.rows_total;
  });
}

static void check_slice(const gulon_dataset *ds, int from, int s, int k) {
  GULON_REQUIRE(ds != nullptr, "dataset is null");
  GULON_REQUIRE(from >= 0 && s >= 0 && from + s <= ds->d, "column slice [%d,%d) outside [0,%d)", from, from + s,
                ds ? ds->d : 0);
  GULON_REQUIRE(k >= 1, "numClusters must be >= 1 (got %d)", k);
}

GULON_API int32_t gulon_kmeans_init(const gulon_dataset *ds, int32_t from, int32_t s, int32_t k, int32_t seed,
                                    float *c_out, int32_t *rows_out) {
  return guarded([&] {
    check_slice(ds, from, s, k);
    GULON_REQUIRE(ds->n >= 1, "KMeans.init needs at least one row");
    std::vector<int> rows(k);
    JRandom rng((int64_t)seed);
    for (int c = 0; c < k; c++) rows[c] = rng.next_int(ds->n);
    if (rows_out) memcpy(rows_out, rows.data(), sizeof(int) * k);
    if (c_out && s > 0) {
      DevBuf<int> dr; dr.upload(rows.data(), k);
      DevBuf<float> dc((size_t)k * s);
      hipLaunchKernelGGL(gather_centroids, dim3(ceil_div((long long)k * s, 256)), dim3(256), 0, 0, ds->x.p, ds->d,
                         from, s, dr.p, k, dc.p);
      HIP_CHECK(hipGetLastError());
      dc.download(c_out, (size_t)k * s);
      HIP_CHECK(hipDeviceSynchronize());
    }
  });
}

GULON_API int32_t gulon_kmeans_assign(const gulon_dataset *ds, int32_t from, int32_t s, const float *centroids,
                                      int32_t k, int32_t rng_batch, int32_t *assignments) {
  return guarded([&] {
    check_slice(ds, from, s, k);
    if (ds->n == 0) return;
    KmeansWorkspace ws;
    DevBuf<float> dc; dc.upload(centroids, std::max<size_t>((size_t)k * s, 1));
    DevBuf<int> da; da.upload(assignments, ds->n);
    PackedSlice packed;
    const PackedSlice *ps = pack_slice_if_filtered(ds->x.p, ds->n, ds->d, from, s, k, packed, nullptr);
    kmeans_assign_dev(ws, ds->x.p, ds->n, ds->d, from, s, dc.p, k, rng_batch, da.p, nullptr, ps);
    da.download(assignments, ds->n);
    HIP_CHECK(hipDeviceSynchronize());
  });
}

GULON_API int32_t gulon_kmeans_update(const gulon_dataset *ds, int32_t from, int32_t s, int32_t k,
                                      const int32_t *assignments, float *c_out) {
  return guarded([&] {
    check_slice(ds, from, s, k);
    if (s == 0) return;
    validate_assignments(assignments, ds->n, k);
    KmeansWorkspace ws;
    DevBuf<int> da; da.upload(assignments, std::max(ds->n, 1));
    DevBuf<float> dc((size_t)k * s);
    kmeans_update_dev(ws, ds->x.p, ds->n, ds->d, from, s, k, da.p, dc.p, nullptr);
    dc.download(c_out, (size_t)k * s);
    HIP_CHECK(hipDeviceSynchronize());
  });
}

GULON_API int32_t gulon_kmeans_iterate(const gulon_dataset *ds, int32_t from, int32_t s, const float *c_in, int32_t k,
                                       int32_t iters, float *c_out) {
  return guarded([&] {
    check_slice(ds, from, s, k);
    GULON_REQUIRE(iters >= 0, "iters must be >= 0");
    if (s == 0) return;
    KmeansWorkspace ws;
    DevBuf<float> dc; dc.upload(c_in, (size_t)k * s);
    DevBuf<int> da(std::max(ds->n, 1));
    HIP_CHECK(hipMemset(da.p, 0, sizeof(int) * (size_t)std::max(ds->n, 1)));   // one array reused (KMeans.scala:101)
    PackedSlice packed;
    const PackedSlice *ps = iters > 0 ? pack_slice_if_filtered(ds->x.p, ds->n, ds->d, from, s, k, packed, nullptr) : nullptr;
    for (int it = 0; it < iters; it++) {
      kmeans_assign_dev(ws, ds->x.p, ds->n, ds->d, from, s, dc.p, k, 0, da.p, nullptr, ps);
      kmeans_update_dev(ws, ds->x.p, ds->n, ds->d, from, s, k, da.p, dc.p, nullptr);
    }
    dc.download(c_out, (size_t)k * s);
    HIP_CHECK(hipDeviceSynchronize());
  });
}

GULON_API int32_t gulon_kmeans_train(const gulon_dataset *ds, int32_t from, int32_t s, int32_t k,
                                     int32_t max_iterations, int32_t seed, float *c_out,
                                     gulon_kmeans_report *reports, int32_t max_reports, int32_t *n_reports) {
  return guarded([&] {
    check_slice(ds, from, s, k);
    GULON_REQUIRE(s >= 1, "dimension must be >= 1");
    float *outs[1] = {c_out};
    kmeans_train_batch(ds->x.p, ds->n, ds->d, 1, &from, &s, &seed, k, max_iterations, outs, reports, max_reports,
                       n_reports);
  });
}

static void check_quantizer_range(const gulon_dataset *ds, int m, int k, int j_begin, int j_end) {
  GULON_REQUIRE(ds != nullptr, "dataset is null");
  GULON_REQUIRE(m >= 1 && m <= ds->d && k >= 1, "bad quantizer shape m=%d k=%d d=%d", m, k, ds->d);
  GULON_REQUIRE(0 <= j_begin && j_begin <= j_end && j_end <= m, "bad quantizer range [%d,%d) of %d", j_begin, j_end, m);
}

// quantizers [j_begin, j_end) of an m-quantizer ProductQuantizer (all of them: 0, m)
static void pq_train_range(const gulon_dataset *ds, int m, int k, int max_iterations, int j_begin, int j_end,
                           float *cents_out, gulon_kmeans_report *reports, int max_reports, int32_t *n_reports) {
  check_quantizer_range(ds, m, k, j_begin, j_end);
  const int np = j_end - j_begin;
  if (np == 0) return;
  std::vector<int> from, until, f(np), sdim(np), seeds(np);
  subvectors(ds->d, m, from, until);
  std::vector<float *> outs(np);
  for (int p = 0; p < np; p++) {
    const int j = j_begin + p;
    f[p] = from[j];
    sdim[p] = until[j] - from[j];
    seeds[p] = j;                                     // ProductQuantizer.scala:139
    outs[p] = cents_out + (size_t)k * from[j];
  }
  kmeans_train_batch(ds->x.p, ds->n, ds->d, np, f.data(), sdim.data(), seeds.data(), k, max_iterations, outs.data(),
                     reports, max_reports, n_reports);
}

GULON_API int32_t gulon_pq_train(const gulon_dataset *ds, int32_t m, int32_t k, int32_t max_iterations,
                                 float *cents_out, gulon_kmeans_report *reports, int32_t max_reports,
                                 int32_t *n_reports) {
  return guarded([&] { pq_train_range(ds, m, k, max_iterations, 0, m, cents_out, reports, max_reports, n_reports); });
}

GULON_API int32_t gulon_pq_train_range(const gulon_dataset *ds, int32_t m, int32_t k, int32_t max_iterations,
                                       int32_t j_begin, int32_t j_end, float *cents_out,
                                       gulon_kmeans_report *reports, int32_t max_reports, int32_t *n_reports) {
  return guarded(
      [&] { pq_train_range(ds, m, k, max_iterations, j_begin, j_end, cents_out, reports, max_reports, n_reports); });
}

// quantizers [j_begin, j_end) of ProductQuantizer.encode (ProductQuantizer.scala:25-35)
static void pq_encode_range(const gulon_dataset *ds, int m, int k, const float *cents, int j_begin, int j_end,
                            uint8_t *codes_out) {
  check_quantizer_range(ds, m, k, j_begin, j_end);
  int width = -1;
  GULON_REQUIRE(gulon_coder_width(k, &width) == GULON_OK, "too many clusters: %d", k);
  const int n = ds->n;
  int bytes = 0;
  gulon_coder_bytes(width, n, &bytes);
  if (n == 0 || width == 0) return;   // Coder0: empty codes
  std::vector<int> from, until;
  subvectors(ds->d, m, from, until);
  KmeansWorkspace ws;
  DevBuf<float> dc;
  DevBuf<int> da(n);
  DevBuf<uint8_t> d8(n);
  std::vector<int> h_idx;
  PackedSlice packed;
  for (int j = j_begin; j < j_end; j++) {
    const int s = until[j] - from[j];
    dc.upload(cents + (size_t)k * from[j], (size_t)k * s);
    pq_assign_quantizer(ws, packed, ds->x.p, n, ds->d, from[j], s, dc.p, k, da.p);
    uint8_t *out = codes_out + (size_t)(j - j_begin) * bytes;
    if (width == 8) {                                                                   // Coder8: idx.toByte
      hipLaunchKernelGGL(narrow_assign_u8, dim3(ceil_div(n, 256)), dim3(256), 0, 0, da.p, (long long)n, d8.p);
      HIP_CHECK(hipGetLastError());
      d8.download(out, n);
      HIP_CHECK(hipDeviceSynchronize());
    } else {
      h_idx.resize(n);
      da.download(h_idx.data(), n);
      HIP_CHECK(hipDeviceSynchronize());
      GULON_REQUIRE(gulon_coder_build(width, h_idx.data(), n, out) == GULON_OK, "coder failed");
    }
  }
}

GULON_API int32_t gulon_pq_encode(const gulon_dataset *ds, int32_t m, int32_t k, const float *cents,
                                  uint8_t *codes_out) {
  return guarded([&] { pq_encode_range(ds, m, k, cents, 0, m, codes_out); });
}

// codes_out: (j_end - j_begin) packed code arrays back to back (quantizer j_begin first)
GULON_API int32_t gulon_pq_encode_range(const gulon_dataset *ds, int32_t m, int32_t k, const float *cents,
                                        int32_t j_begin, int32_t j_end, uint8_t *codes_out) {
  return guarded([&] { pq_encode_range(ds, m, k, cents, j_begin, j_end, codes_out); });
}
