/*
 * gulon_hip.h -- C ABI of libgulon_hip.so: the MI355X (gfx950) implementation of
 * tixxit/gulon's ANN hot path (KMeans train/assign, ProductQuantizer encode +
 * distance tables, Index.query ADC scan + top-k, partial top-k merge).
 *
 * The reference has NO native boundary (it is 100 % Scala); every entry point
 * below replaces the body of one public Scala method and cites it.  Paths are
 * relative to /root/reference/core/src/main/scala/net/tixxit/gulon/.  The JNI /
 * Scala stubs that bind these are shown in INTEGRATION.md.
 *
 * Conventions
 *  - plain pointers and sizes only; the caller owns every host buffer for the
 *    duration of a call; handles own device memory until *_destroy.
 *  - matrices are flat row-major float32 (Matrix.data flattened, ld = cols).
 *  - codebooks are ONE flat array of k*d floats: quantizer j's k x s_j block
 *    starts at cents + k*from_j (from_j, s_j from gulon_subvectors).
 *  - every function returns a status: 0 ok, <0 error class (below);
 *    gulon_last_error() gives the thread-local message.  The JNI glue maps
 *    INVALID_ARGUMENT -> IllegalArgumentException (the reference's `require`),
 *    ILLEGAL_STATE -> IllegalStateException, the rest -> RuntimeException.
 *  - all arithmetic is IEEE binary32, unfused, in the reference's evaluation
 *    order; results are bit-identical to the reference algorithm (see DESIGN.md
 *    for the two documented tie rules).
 *  - "_dev" variants take DEVICE pointers and a hipStream_t (as void*), do not
 *    synchronise, and are what bench.py times (inputs resident in HBM).
 */
#ifndef GULON_HIP_H
#define GULON_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GULON_ABI_VERSION 3

#define GULON_OK 0
#define GULON_ERR_INVALID_ARGUMENT (-1) /* reference: require(...) / IllegalArgumentException */
#define GULON_ERR_ILLEGAL_STATE (-2)    /* reference: IllegalStateException("heap is empty") */
#define GULON_ERR_UNSUPPORTED (-3)      /* valid in the reference, not yet on this path */
#define GULON_ERR_DEVICE (-4)           /* HIP runtime failure */
#define GULON_ERR_OOM (-5)

/* flags written per query by the top-k kernels (see DESIGN.md "tie rule") */
#define GULON_FLAG_BOUNDARY_TIE 1 /* K-th and (K+1)-th smallest distances are equal */
#define GULON_FLAG_INTERIOR_TIE 2 /* two equal distances inside the top K */
#define GULON_FLAG_EXACT_REPLAY 4 /* tie resolved by replaying the reference heap's insertion history:
                                     ids and order are exactly TopKHeap's (single, unsharded index only).
                                     A tie-flagged query is left unreplayed -- tie flags without this one, ids in
                                     (distance, row id) order -- when the replay collects more than 8 192 candidate
                                     rows for it (2 048 in one shard of a sharded index), when the reference heap
                                     makes more than 2 048 successful insertions over the range, or at
                                     k_nn > GULON_MAX_K.  Which queries reach a candidate limit depends on the launch
                                     geometry, which follows the handle's recent batches: the same query may be
                                     replayed in one batch and not in another; both answers hold this contract. */

#define GULON_FLAG_NONFINITE 8    /* the query's distances can be NaN / +inf (NaN or huge query components, NaN
                                     centroids): result = the literal TopKHeap over all rows, TopKHeap.scala:69-79 */

#define GULON_MAX_K 63 /* neighbours per query held by one wavefront list: fast path, exact tie replay,
                          sharded merge */
#define GULON_MAX_K_PEELED 8191 /* larger k_nn (flat index of any code width, sharded or not; exact kNN): the result
                                   is peeled 64 entries per scan (a shard returns k_nn + 1 <= 8191 entries); ties keep
                                   the (distance, row id) order + flags */

typedef struct gulon_dataset gulon_dataset; /* device-resident Matrix            */
typedef struct gulon_index gulon_index;     /* device-resident PQIndex (codes+PQ) */
typedef struct gulon_sharded_index gulon_sharded_index; /* PQIndex row-sharded over the GPUs of one node */

/* One KMeans.ProgressReport (KMeans.scala:119-127) as plain numbers. */
typedef struct {
  int32_t num_iterations;
  int32_t converged;
  int32_t step_count; /* SummaryStats.count */
  float step_mean;    /* SummaryStats.mean  */
  float step_s;       /* SummaryStats.s     */
} gulon_kmeans_report;

/* ---- runtime ---------------------------------------------------------- */
const char *gulon_last_error(void);
int32_t gulon_abi_version(void);
int32_t gulon_device_count(int32_t *out);
int32_t gulon_set_device(int32_t device);
int32_t gulon_device_synchronize(void);
int32_t gulon_dev_malloc(void **out, size_t bytes);
int32_t gulon_dev_free(void *p);
int32_t gulon_memcpy_h2d(void *dst_dev, const void *src_host, size_t bytes);
int32_t gulon_memcpy_d2h(void *dst_host, const void *src_dev, size_t bytes);

/* ---- Vectors.subvectors (Vectors.scala:84-104) -------------------------- */
int32_t gulon_subvectors(int32_t d, int32_t m, int32_t *from, int32_t *until);

/* ---- Coder (Coder.scala) ------------------------------------------------ */
/* ProductQuantizer.coderFactory (ProductQuantizer.scala:11-16): width for k
 * clusters after Coder.factoryFor rounding (Coder.scala:35-45); -1 if > 16 bit. */
int32_t gulon_coder_width(int32_t num_clusters, int32_t *width_out);
/* BytePackedCoder.bytesPerCode / BytePlus (Coder.scala:82-83,153) */
int32_t gulon_coder_bytes(int32_t width, int32_t length, int32_t *bytes_out);
/* Coder.buildCode (Coder.scala:85-89,100-108,115-123,130-136,147-161) */
int32_t gulon_coder_build(int32_t width, const int32_t *indices, int32_t length, uint8_t *code_out);
/* Coder.getIndex for all i (Coder.scala:91-92,110-111,125-126,138-139,163-167) */
int32_t gulon_coder_unpack(int32_t width, const uint8_t *code, int32_t length, int32_t *indices_out);

/* ---- Matrix on the device ------------------------------------------------ */
/* Copies an n x d row-major host matrix to HBM (Matrix.scala:3). */
int32_t gulon_dataset_create(const float *x_host, int32_t n, int32_t d, gulon_dataset **out);
/* Synthetic data generated on the device, bit-identical to the CPU test
 * generator: kind 0 iid N(0,1)~Irwin-Hall, 1 clustered, 2 U[0,1), 3 overlapping clusters. */
int32_t gulon_dataset_create_synth(int32_t n, int32_t d, int32_t kind, uint64_t seed,
                                   int32_t ncentres, gulon_dataset **out);
int32_t gulon_dataset_destroy(gulon_dataset *ds);
int32_t gulon_dataset_shape(const gulon_dataset *ds, int32_t *n, int32_t *d);
/* device pointer to the n x d row-major float32 data (for *_dev entry points) */
int32_t gulon_dataset_device_ptr(const gulon_dataset *ds, const float **out);
/* copy rows[0..nrows) (row-major) back to the host */
int32_t gulon_dataset_get_rows(const gulon_dataset *ds, const int32_t *rows, int32_t nrows, float *out_host);
/* WordVectors.sorted (WordVectors.scala:60-71) and every other reordering of rows: a new dataset of n rows with
 * out[i] = ds[rows[i]], gathered on the device (rows: host ints in [0, ds rows); destroy with gulon_dataset_destroy). */
int32_t gulon_dataset_gather(const gulon_dataset *ds, const int32_t *rows, int32_t n, gulon_dataset **out);

/* ---- word2vec text ingest (WordVectors.readWord2Vec, WordVectors.scala:141-252) -----------------
 * text[0, len): the bytes of the file (host memory; copied to the device in chunks of about chunk_bytes cut at line
 * ends, 0 = 64 MiB), data_offset: where the first data line starts (the header line, if any, is the host's:
 * readDimension, WordVectors.scala:143-160), d: the dimension.  Lines end at \n only; an empty line adds no row; a last line without
 * \n counts; fields are separated by single blanks; the word is the bytes before the first blank, the vector fields
 * 1 .. d; further fields are ignored (readFast, WordVectors.scala:162-197).  Each token becomes the correctly rounded binary32
 * (java.lang.Float.parseFloat, :190) on the device, or is FLAGGED: outside the plain decimal grammar, or not decidable
 * in the 64-bit significand the kernel carries (gulon_amd/csrc/ingest_parse.h).  The caller converts the flagged
 * tokens and passes them to gulon_ingest_finish; their coordinates are 0 until then.
 *   gulon_ingest_counts   rows read, flagged tokens, and the first row with fewer than d components (-1: none --
 *                         the reference fails on such a line, :183-189; its coordinates are not defined)
 *   gulon_ingest_words    per row the byte offset in text and the length of its word (:183)
 *   gulon_ingest_flagged  per flagged token (in no particular order): row, component 0 .. d-1, byte offset, length
 *   gulon_ingest_finish   writes patch_value[i] to (patch_row[i], patch_field[i]), then, normalize != 0,
 *                         MathUtils.normalize of every row (MathUtils.scala:100-120, as
 *                         readWord2Vec(..., normalize = true) does per line, :222-227), and hands the matrix over as
 *                         a gulon_dataset; once per ingest
 * Rows keep the order of the file. */
typedef struct gulon_ingest gulon_ingest;
int32_t gulon_ingest_word2vec(const uint8_t *text, uint64_t len, uint64_t data_offset, int32_t d,
                              uint64_t chunk_bytes, gulon_ingest **out);
int32_t gulon_ingest_counts(const gulon_ingest *in, int64_t *rows, int64_t *flagged, int64_t *first_short_row);
int32_t gulon_ingest_words(const gulon_ingest *in, int64_t *begin, int32_t *length);
int32_t gulon_ingest_flagged(const gulon_ingest *in, int64_t *row, int32_t *field, int64_t *begin, int32_t *length);
int32_t gulon_ingest_finish(gulon_ingest *in, const int64_t *patch_row, const int32_t *patch_field,
                            const float *patch_value, int64_t n_patch, int32_t normalize, gulon_dataset **out);
int32_t gulon_ingest_destroy(gulon_ingest *in);

/* ---- KMeans (KMeans.scala) ------------------------------------------------ */
/* KMeans.init (KMeans.scala:188-196): k rows drawn with java.util.Random(seed),
 * with replacement.  c_out: k x s host floats; rows_out (nullable): k ints. */
int32_t gulon_kmeans_init(const gulon_dataset *ds, int32_t from, int32_t s, int32_t k, int32_t seed,
                          float *c_out, int32_t *rows_out);
/* KMeans.assign (serial, KMeans.scala:18-22,70-98; rng_batch = 0: one Random(0)
 * stream over all rows) and KMeans.parAssign (KMeans.scala:57-68; rng_batch =
 * 25000: a fresh Random(0) per 25 000-row batch).  assignments: n host ints,
 * written for every row (the reference leaves NaN-distance rows untouched; see
 * DESIGN.md). */
int32_t gulon_kmeans_assign(const gulon_dataset *ds, int32_t from, int32_t s, const float *centroids,
                            int32_t k, int32_t rng_batch, int32_t *assignments);
/* KMeans.fromAssignment (KMeans.scala:198-226): order-dependent fp32 running mean. */
int32_t gulon_kmeans_update(const gulon_dataset *ds, int32_t from, int32_t s, int32_t k,
                            const int32_t *assignments, float *c_out);
/* KMeans.iterate (KMeans.scala:100-106). */
int32_t gulon_kmeans_iterate(const gulon_dataset *ds, int32_t from, int32_t s, const float *c_in,
                             int32_t k, int32_t iters, float *c_out);
/* KMeans.computeClusters (KMeans.scala:134-157) with Config(numClusters = k,
 * maxIterations, seed) (KMeans.scala:129-132).  reports (nullable) receives the
 * ProgressReports in order (first = the init report); *n_reports the count. */
int32_t gulon_kmeans_train(const gulon_dataset *ds, int32_t from, int32_t s, int32_t k,
                           int32_t max_iterations, int32_t seed, float *c_out,
                           gulon_kmeans_report *reports, int32_t max_reports, int32_t *n_reports);

#ifdef GULON_TEST_HOOKS   /* libgulon_hip_testhooks.so only: the product library does not export these */
/* Self-test of the running mean's division (kmeans.hip, update_chains): the three-operation quotient
 * q0 = RN(a y), r = fma(-n, q0, a), q = fma(r, y, q0) with y = RN(1/n) against the correctly rounded division
 * for every divisor n in [1, n_max] (n_max < 2^24) and `numerators_per_divisor` numerators each (random, and
 * next to rounding boundaries).  *mismatches must come back 0. */
int32_t gulon_selftest_mean_division(int32_t n_max, int32_t numerators_per_divisor, uint64_t seed, int64_t *mismatches);
/* KMeans.fromAssignment (KMeans.scala:198-226) of one slice -- columns [from, from + s) of the host matrix x (n rows,
 * leading dimension ld), host assignments in [0, k) -- through the STREAMED update of PQ training (kmeans_stream.hip),
 * which the library proper reaches inside gulon_pq_train only.  centroids_out: k x s. */
int32_t gulon_selftest_stream_update(const float *x, int32_t n, int32_t ld, int32_t from, int32_t s, int32_t k,
                                     const int32_t *assign, float *centroids_out);
/* Self-test of the filter's conflict-ordered code copy (conflict_order.hip; no reference counterpart: where a row
 * sits inside the device copy is an implementation detail behind PQIndex.batchQuery, Index.scala:209-263).
 * codes: n_blocks x 64 rows x 16 code bytes; rows are re-dealt inside WINDOWS of four consecutive blocks (a last
 * window of fewer blocks: inside the blocks it has).  codes_out receives the re-dealt blocks, place_out[b * 64 + lane]
 * the place (0..255) in its window of the row that now sits in `lane` of block b: over a window the places are a
 * permutation and codes_out[b][lane] == codes[window rows][place].  rounds = passes of the ordering (0: identity). */
int32_t gulon_selftest_conflict_order(const uint8_t *codes, int64_t n_blocks, int32_t rounds, uint8_t *codes_out,
                                      uint8_t *place_out);
/* Self-test of the bf16-split MFMA filter of KMeans.assign (kmeans_mfma.hip, assign_bf16): largest
 * |d' - d| / band over 64 random rows x 32 random centroids of sub-dimension s (coordinates ~ scale * U(-1,1) with
 * outliers), d' = the matrix cores' value, d = the reference's unfused fp32 chain (KMeans.scala:42-47).  The filter
 * is sound while the result stays below 0.5 (the band is twice the error bound). */
int32_t gulon_selftest_assign_band(int32_t s, uint64_t seed, float scale, double *max_error_over_band);
/* The MFMA filter stage of KMeans.assign (KMeans.scala:24-98) alone, as the library runs it in front of the exact
 * kernels: the slice [from, from + s) of the host matrix x (n rows, leading dimension ld) is packed and filtered against
 * centroids (k x s).  assign_inout (n, pre-filled by the caller) comes back as the filter left it: the answer of every
 * row it decided, untouched where it did not.  flagged_rows_out (n) receives the rows it handed to the exact kernel, in
 * no particular order, *n_flagged their number.  form_out = {kind, width} of the kernel the dispatch chose:
 * kind 0 no filter for this (s, k) (nothing runs), 1 assign_mfma<T>, 2 assign_mfma_stream<T>, 3 assign_bf16 with compact
 * operand words, 4 assign_bf16 with three pieces; width = T, or the operand words per lane. */
int32_t gulon_selftest_assign_filter(const float *x, int32_t n, int32_t ld, int32_t from, int32_t s,
                                     const float *centroids, int32_t k, int32_t *assign_inout,
                                     int32_t *flagged_rows_out, int32_t *n_flagged, int32_t form_out[2]);
#endif
/* Stage times of the training loop for bench.py's k-means record (BASELINE config 3): while enabled, every
 * stage of KMeans.computeClusters / ProductQuantizer.apply is closed by a device synchronisation and its wall
 * time accumulated over the iterations (process-wide; not for concurrent trainings):
 *   update   = KMeans.fromAssignment of all sub-quantizers (stable counting sort + sequential mean chains)
 *   assign   = first stage of parAssign of all sub-quantizers: centroid prep + the MFMA filter kernel
 *   recheck  = exact re-evaluation of the rows the filter flagged + java.util.Random tie replay
 *   converge = Arrays.equals(prev, next) + ProgressReport
 * mfma_flops = 2 n k s summed over the filtered sub-quantizers and iterations (2 n k d per PQ
 * iteration); update_bytes = 4 n s summed likewise (n d 4 B per PQ iteration). */
typedef struct {
  int32_t iterations;
  double update_ms, assign_ms, recheck_ms, converge_ms;
  double mfma_flops, update_bytes;
  double rows_rechecked, rows_total;
} gulon_kmeans_trace_totals;
int32_t gulon_kmeans_trace(int32_t enable);   /* resets the totals */
int32_t gulon_kmeans_trace_read(gulon_kmeans_trace_totals *out);

/* ---- ProductQuantizer (ProductQuantizer.scala) ----------------------------- */
/* ProductQuantizer.apply / fromSubvectors (ProductQuantizer.scala:121-153), Config
 * (:107-111): m independent computeClusters, seed = quantizer index.
 * cents_out: k*d floats.  reports (nullable): m x max_reports, n_reports: m. */
int32_t gulon_pq_train(const gulon_dataset *ds, int32_t m, int32_t k, int32_t max_iterations,
                       float *cents_out, gulon_kmeans_report *reports, int32_t max_reports,
                       int32_t *n_reports);
/* The same for quantizers [j_begin, j_end) only -- the unit of work when the m independent
 * sub-quantizers are trained on different GPUs (ProductQuantizer.scala:130-145 runs them with
 * parTraverse).  Only those quantizers' blocks of cents_out are written; reports/n_reports are
 * indexed from j_begin. */
int32_t gulon_pq_train_range(const gulon_dataset *ds, int32_t m, int32_t k, int32_t max_iterations,
                             int32_t j_begin, int32_t j_end, float *cents_out, gulon_kmeans_report *reports,
                             int32_t max_reports, int32_t *n_reports);
/* ProductQuantizer.encode (ProductQuantizer.scala:25-35): per quantizer the serial
 * assign, packed by the Coder for k (coderFactory :11-16).  codes_out: m arrays of
 * gulon_coder_bytes(width, n) bytes, back to back ([m][bytesPerCode], the
 * EncodedMatrix.encodings layout, EncodedMatrix.scala:11-23). */
int32_t gulon_pq_encode(const gulon_dataset *ds, int32_t m, int32_t k, const float *cents,
                        uint8_t *codes_out);
/* quantizers [j_begin, j_end) only: codes_out holds (j_end - j_begin) packed arrays back to back */
int32_t gulon_pq_encode_range(const gulon_dataset *ds, int32_t m, int32_t k, const float *cents,
                              int32_t j_begin, int32_t j_end, uint8_t *codes_out);

/* ---- Index (Index.scala) ---------------------------------------------------- */
/* Index.prepareQuery (Index.scala:352-383): t_out[B][m][k]. */
int32_t gulon_prepare_query(const float *cents, int32_t d, int32_t m, int32_t k, const float *queries,
                            int32_t b, float *t_out);
/* PQIndex(productQuantizer, data) (Index.scala:385-391): copies the m packed code
 * arrays (each gulon_coder_bytes(width,n) bytes, back to back) and the codebooks
 * to HBM.  row_base is added to every returned row id (row sharding).
 * Every code width of ProductQuantizer.coderFactory: k <= 256 (widths 0/2/4/8) runs the
 * byte-coded kernels; 256 < k <= 65536 (Coder.BytePlus, widths 10/12/16) the wide-code path
 * (wide.hip: exact scan behind a quantized filter, exact tie replay up to k_nn = GULON_MAX_K; larger k_nn up to
 * GULON_MAX_K_PEELED peeled 64 entries per scan round like a byte-coded index: (distance, row id) order, tie flags
 * without GULON_FLAG_EXACT_REPLAY; queries with NaN / +inf distances keep the (distance, row id) rule at every k_nn). */
int32_t gulon_index_create(const uint8_t *codes, int32_t n, int32_t d, int32_t m, int32_t k,
                           const float *cents, int32_t row_base, gulon_index **out);
int32_t gulon_index_destroy(gulon_index *idx);
/* Concurrency rules of a gulon_index handle (the reference's PQIndex is immutable and queried from many
 * threads at once, Tests.scala:109-122):
 *  - one handle = one workspace.  All per-query scratch (tables, partial lists, survivor queues, replay pools)
 *    belongs to the handle.  Calls on one handle may come from any thread and any stream: the host side is
 *    serialised by a mutex, and the DEVICE work of a call on another stream than the previous call's is
 *    ordered behind it with an event -- two batches "in flight" on one handle run one after the other,
 *    never on top of each other's scratch.  Results do not depend on the handle's earlier calls, and
 *    gulon_index_tuning on a live handle changes the work a call does, never its results.
 *  - gulon_index_context_create gives another workspace over the SAME read-only codes and codebooks (no
 *    copy): one context per batch in flight (bench.py: one per stream) overlaps their device work.  A
 *    context is destroyed with gulon_index_destroy; the codes live until the index and all of its contexts
 *    are destroyed.  Create and use a context with the index's device current.
 *  - the host-pointer gulon_index_batch_query takes such a context internally (up to GULON_HOST_CONTEXTS,
 *    default 4, created on first use, each with a stream of its own), so concurrent callers overlap.
 *  - the two-call sequence scan_bounds -> scan_partial_bounded must not be interleaved with other calls on the
 *    same handle (any other query call drops the pending first half: GULON_ERR_INVALID_ARGUMENT).
 *  - a gulon_grouped_index handle follows the first rule as well: it is one workspace (coarse distances, group lists,
 *    per-group heaps, the pre-selection's tables), its calls are serialised by a mutex, and the device work of a call
 *    on another stream than the previous call's -- queries, lookups, expressions, pair distances, diagnostics -- is
 *    ordered behind it with the same event.  It has no contexts: batches that should overlap need a handle each. */
int32_t gulon_index_context_create(gulon_index *parent, gulon_index **out);
/* PQIndex.batchQuery(k, vectors, from, until) (Index.scala:417-440) followed by
 * Index.Result.fromHeap (Index.scala:83-94): per query the K nearest rows of
 * [from, until) by ADC distance, ascending.  out_idx/out_dist: [B][K];
 * out_count[B] = live entries (< K when until - from < K); out_flags (nullable)
 * [B] GULON_FLAG_*.  from/until are LOCAL row numbers (0..n). */
int32_t gulon_index_batch_query(gulon_index *idx, const float *queries, int32_t b, int32_t k_nn,
                                int32_t from, int32_t until, int32_t *out_idx, float *out_dist,
                                int32_t *out_count, int32_t *out_flags);
/* Device-resident form: queries/out_* are device pointers, work is enqueued on
 * `stream` (hipStream_t) and not synchronised. */
int32_t gulon_index_batch_query_dev(gulon_index *idx, const float *d_queries, int32_t b, int32_t k_nn,
                                    int32_t from, int32_t until, int32_t *d_out_idx, float *d_out_dist,
                                    int32_t *d_out_count, int32_t *d_out_flags, void *stream);
/* Per-shard partial top-(K+1) for the multi-GPU merge: d_part_dist/d_part_idx are
 * [B][K+1] device arrays, ascending by (distance, row id), padded with
 * (+inf, INT32_MAX). */
int32_t gulon_index_scan_partial_dev(gulon_index *idx, const float *d_queries, int32_t b, int32_t k_nn,
                                     int32_t from, int32_t until, float *d_part_dist,
                                     int32_t *d_part_idx, void *stream);
/* The same partial scan in two halves, so that ROW SHARDS can share their pruning bounds (one tiny
 * all-gather between the halves; sharded.py).  The reference scans every row of every partition
 * (Index.scala:424-437); the quantized filter in front of the exact arithmetic prunes against an
 * upper bound of the (K+1)-th distance, and a bound drawn from the samples of ALL shards is
 * `shards` times tighter than a shard's own -- results do not change, only the work.
 *   1. gulon_index_scan_bounds_dev: table build + sample scan of this shard; d_bounds [B][K+1] =
 *      the K+1 smallest sample distances per query, ascending, +inf padded (all +inf for ranges
 *      the filter does not take);
 *   2. the caller gathers the arrays of all shards: d_all_bounds [lists][B][K+1] (this shard's
 *      own among them, any order);
 *   3. gulon_index_scan_partial_bounded_dev: the rest of the scan against the (K+1)-th smallest
 *      value of the union; same arguments as step 1 on the same index (GULON_ERR_INVALID_ARGUMENT
 *      otherwise), outputs as gulon_index_scan_partial_dev.  k_nn <= GULON_MAX_K. */
int32_t gulon_index_scan_bounds_dev(gulon_index *idx, const float *d_queries, int32_t b, int32_t k_nn,
                                    int32_t from, int32_t until, float *d_bounds, void *stream);
int32_t gulon_index_scan_partial_bounded_dev(gulon_index *idx, const float *d_queries, int32_t b, int32_t k_nn,
                                             int32_t from, int32_t until, const float *d_all_bounds,
                                             int32_t lists, float *d_part_dist, int32_t *d_part_idx,
                                             void *stream);
/* Exact TopKHeap replay of tie-flagged queries across ROW SHARDS (the unsharded
 * gulon_index_batch_query* does this internally).  After gulon_topk_merge_dev every shard holds
 * the same flags; each shard then collects, for up to `max_flagged` flagged queries after the first
 * `skip` ones (ascending query number), the rows of its range that may insert into the reference's
 * heap (a superset, with global row ids, at most `pool` per query) into a buffer of
 * gulon_replay_pack_words(max_flagged, pool) int32 words; word [3] of the buffer receives the number
 * of flagged queries of the whole batch.  The buffers of all shards (in row order: shard 0 first),
 * laid out back to back, go to gulon_replay_apply_dev, which runs the literal TopKHeap
 * (TopKHeap.scala:57-79) over their union and overwrites idx/dist/count of those queries, setting
 * GULON_FLAG_EXACT_REPLAY.  A batch with more flagged queries than one round holds is finished by
 * further rounds with skip advanced (gulon_sharded_index_batch_query and gulon_amd/sharded.py loop
 * until skip >= word [3]).  A query with more than `pool` candidates in a shard (or more than 16 384
 * over all shards) keeps the (distance, row id) result and its tie flags.
 * max_flagged in [1, 1024], pool in [64, 8192]; the defaults below size the first, unconditional round. */
#define GULON_REPLAY_MAX_FLAGGED 16
#define GULON_REPLAY_POOL 2048
int64_t gulon_replay_pack_words(int32_t max_flagged, int32_t pool); /* -1: out of range */
int32_t gulon_index_replay_collect_dev(gulon_index *idx, const float *d_queries, int32_t b, int32_t k_nn,
                                       int32_t from, int32_t until, const int32_t *d_flags, int32_t skip,
                                       int32_t max_flagged, int32_t pool, int32_t *d_pack, void *stream);
int32_t gulon_replay_apply_dev(const int32_t *d_packs, int32_t lists, int32_t max_flagged, int32_t pool, int32_t b,
                               int32_t k_nn, int32_t *d_out_idx, float *d_out_dist, int32_t *d_out_count,
                               int32_t *d_out_flags, void *stream);
/* ---- PQIndex row-sharded over the GPUs of one node, ONE host process (sharded.hip) ---------------
 * The multi-GPU form of PQIndex.batchQuery for a caller that is one process (the JVM): shard s holds rows
 * [n*s/S, n*(s+1)/S) -- the from/until contract of Index.scala:417-419 -- on device devices[s] (a device
 * may hold several shards); every query batch runs bounds -> scan -> merge -> tie replay on all shards
 * with three RCCL all-gathers over xGMI in between (ncclCommInitAll over the distinct devices; librccl is
 * loaded on first use).  The merge is TopKHeap.merge (TopKHeap.scala:44-53) under the (distance, row id)
 * order and tie-flagged queries are replayed with the literal heap over the candidates of all shards, in
 * as many rounds as the batch needs: ids, order, distances and flags equal the unsharded
 * gulon_index_batch_query bit for bit, whatever the number of shards.  codes/cents as gulon_index_create
 * (all n rows).  GULON_MAX_K < k_nn < GULON_MAX_K_PEELED: peeled partial lists, pairwise merge, no tie replay
 * (as the unsharded index at such k_nn). */
int32_t gulon_sharded_index_create(const uint8_t *codes, int32_t n, int32_t d, int32_t m, int32_t k,
                                   const float *cents, const int32_t *devices, int32_t n_shards,
                                   gulon_sharded_index **out);
int32_t gulon_sharded_index_destroy(gulon_sharded_index *idx);
int32_t gulon_sharded_index_batch_query(gulon_sharded_index *idx, const float *queries, int32_t b, int32_t k_nn,
                                        int32_t *out_idx, float *out_dist, int32_t *out_count, int32_t *out_flags);
/* shards, distinct devices (= RCCL ranks), ncclGetVersion, and of the last batch: replay rounds, flagged queries
 * (every out pointer nullable) */
int32_t gulon_sharded_index_info(const gulon_sharded_index *idx, int32_t *n_shards, int32_t *n_devices,
                                 int32_t *rccl_version, int32_t *last_replay_rounds, int32_t *last_flagged_queries);
/* ---- GroupedIndex (Index.scala:231-308): coarse groups + product-quantized residuals ---------
 * Rows are in GROUPED order (WordVectors.grouped, WordVectors.scala:24-58): stably ordered by the
 * coarse cluster they were assigned to; group c covers rows [offsets[c-1], offsets[c]) (first group
 * from 0, last to n); group_centroids holds the centroids of the g groups as the reference's builder
 * loop emits them (the non-empty clusters in cluster order, preceded by a copy of original row 0's
 * centroid for an EMPTY group [0, 0) when row 0 is not in the first of them, :38-39); the codes are the ProductQuantizer codes of the RESIDUALS (row - its group's centroid,
 * WordVectors.Grouped.residuals :118-138).  Returned ids are grouped row positions.
 *
 * gulon_dataset_group_residuals builds that residual matrix on the device:
 *   out[i] = ds[perm[i]] - group_centroids[group_of[i]]                       (MathUtils.subtract)
 * gulon_grouped_index_batch_query = GroupedIndex.batchQuery (:254-282): per query searchSpace
 * (:285-299; strategy 0 = LimitGroups(limit), 1 = LimitVectors(limit)), then for every searched
 * group, nearest first, PQIndex.query on (query - centroid) over the group's rows and
 * TopKHeap.merge into the result heap, then Result.fromHeap.  The heaps are the reference's,
 * literally (array order included), so ids and order equal the JVM's also under distance ties --
 * equally distant coarse centroids included (they are common: WordVectors.grouped's leading empty
 * group repeats a centroid, WordVectors.scala:38-39): queries whose searched groups hang on such a tie
 * (or on a NaN distance) select their groups through the literal exactNearestNeighbours heap.
 * Groups may be empty (offsets may repeat).  k_nn <= GULON_MAX_K on the fast paths; up to 2048 (every code width)
 * through the literal heaps alone, kept in LDS (Tests.scala asks for up to 1000 neighbours).
 * The _dev form enqueues on `stream` and does not synchronise, with one exception: LimitVectors over more than 64
 * groups waits for `stream` once, to size the per-group heaps by a counter it reads back. */
typedef struct gulon_grouped_index gulon_grouped_index;
int32_t gulon_dataset_group_residuals(const gulon_dataset *ds, const int32_t *perm, const int32_t *group_of,
                                      const float *group_centroids, int32_t g, gulon_dataset **out);
int32_t gulon_grouped_index_create(const uint8_t *codes, int32_t n, int32_t d, int32_t m, int32_t k,
                                   const float *pq_cents, const float *group_centroids, const int32_t *offsets,
                                   int32_t g, gulon_grouped_index **out);
int32_t gulon_grouped_index_destroy(gulon_grouped_index *idx);
int32_t gulon_grouped_index_batch_query(gulon_grouped_index *idx, const float *queries, int32_t b, int32_t k_nn,
                                        int32_t strategy, int32_t limit, int32_t *out_idx, float *out_dist,
                                        int32_t *out_count);
int32_t gulon_grouped_index_batch_query_dev(gulon_grouped_index *idx, const float *d_queries, int32_t b,
                                            int32_t k_nn, int32_t strategy, int32_t limit, int32_t *d_out_idx,
                                            float *d_out_dist, int32_t *d_out_count, void *stream);

/* ---- Decoding stored rows; query by stored row (decode.hip) ------------------------------------------
 * Row ids are LOCAL rows of the index (0..n; for a GroupedIndex: grouped row positions).  The host-pointer forms
 * check every id before launching anything (GULON_ERR_INVALID_ARGUMENT for one outside [0, n)).  The _dev forms take
 * device pointers and a stream, do not synchronise, and cannot check ids on the host: a row outside [0, n) comes back
 * as an all-NaN vector (its query as the query of an all-NaN vector) and sets the handle's row-error word, which
 * gulon_index_row_error / gulon_grouped_index_row_error return and clear (synchronising the device).
 * normalize != 0 applies MathUtils.normalize (MathUtils.scala:100-120: sequential fp32 sum of x * x, sqrt in double,
 * one division per coordinate; a zero vector gives NaN) -- the handles carry no metric, so a cosine index passes 1.
 *
 * ProductQuantizer.decode(EncodedVector) (ProductQuantizer.scala:37-50), i.e. PQIndex.decode (Index.scala:390-391)
 * and SortedIndex.lookup (Index.scala:318-319) for b rows: out [b][d]. */
int32_t gulon_index_decode_rows(gulon_index *idx, const int32_t *rows, int32_t b, int32_t normalize, float *out);
int32_t gulon_index_decode_rows_dev(gulon_index *idx, const int32_t *d_rows, int32_t b, int32_t normalize,
                                    float *d_out, void *stream);
/* ProductQuantizer.decode(EncodedMatrix) (ProductQuantizer.scala:58-78) of rows [from, until) into a new device
 * dataset of until - from rows (destroy with gulon_dataset_destroy). */
int32_t gulon_index_decode_dataset(gulon_index *idx, int32_t from, int32_t until, gulon_dataset **out);
/* GroupedIndex.lookup (Index.scala:247-253) for b rows: centroids(partition) + decode(row), one fp32 add per
 * coordinate (MathUtils.add, MathUtils.scala:63-71), partition = the reference's Arrays.binarySearch(offsets, row)
 * rule -- which, where offsets repeat (empty groups), can name another group than the row's own. */
int32_t gulon_grouped_index_lookup_rows(gulon_grouped_index *idx, const int32_t *rows, int32_t b, int32_t normalize,
                                        float *out);
int32_t gulon_grouped_index_lookup_rows_dev(gulon_grouped_index *idx, const int32_t *d_rows, int32_t b,
                                            int32_t normalize, float *d_out, void *stream);
/* Index.queryByWord (Index.scala:38-45) on row ids: PQIndex.batchQuery (Index.scala:417-440) of the decoded rows over
 * [from, until), outputs as gulon_index_batch_query. */
int32_t gulon_index_query_rows(gulon_index *idx, const int32_t *rows, int32_t b, int32_t k_nn, int32_t normalize,
                               int32_t from, int32_t until, int32_t *out_idx, float *out_dist, int32_t *out_count,
                               int32_t *out_flags);
int32_t gulon_index_query_rows_dev(gulon_index *idx, const int32_t *d_rows, int32_t b, int32_t k_nn, int32_t normalize,
                                   int32_t from, int32_t until, int32_t *d_out_idx, float *d_out_dist,
                                   int32_t *d_out_count, int32_t *d_out_flags, void *stream);
/* The same for a GroupedIndex: GroupedIndex.lookup, then GroupedIndex.batchQuery (Index.scala:254-299), outputs
 * as gulon_grouped_index_batch_query. */
int32_t gulon_grouped_index_query_rows(gulon_grouped_index *idx, const int32_t *rows, int32_t b, int32_t k_nn,
                                       int32_t normalize, int32_t strategy, int32_t limit, int32_t *out_idx,
                                       float *out_dist, int32_t *out_count);
int32_t gulon_grouped_index_query_rows_dev(gulon_grouped_index *idx, const int32_t *d_rows, int32_t b, int32_t k_nn,
                                           int32_t normalize, int32_t strategy, int32_t limit, int32_t *d_out_idx,
                                           float *d_out_dist, int32_t *d_out_count, void *stream);
int32_t gulon_index_row_error(gulon_index *idx, int32_t *out);
int32_t gulon_grouped_index_row_error(gulon_grouped_index *idx, int32_t *out);
/* ---- Index views: a chosen subset of an index's rows as an index of its own ------------------------
 * A view of `idx` over rows r_0 < r_1 < ... < r_{s-1} (local rows, 0 <= r_i < n) is the PQIndex over the EncodedMatrix
 * whose columns are those rows in that order, gathered on the device from the codes already in HBM.  Through every
 * other entry point a view is an ordinary gulon_index of s rows that answers in positions p (from / until are
 * positions; its row_base is 0); the gulon_index_view_* queries answer in the row ids of `idx`: every returned p >= 0
 * becomes idx.row_base + r_p, padding, distances, counts and flags pass through.  The map ascends strictly, so the
 * (distance, row id) order and the tie flags mean the same before and after it.  A view of a view takes positions of
 * the view and names rows of the root.  s = 0 is a valid view.  A view owns all it reads (codes gathered, codebooks
 * copied device to device): `idx` may be destroyed first, and a context of a view hangs off the view.  Destroy a view
 * with gulon_index_destroy.
 * gulon_index_select_rows: `rows` (host) is checked before anything is launched -- strictly ascending, every row in
 * [0, n), else GULON_ERR_INVALID_ARGUMENT naming the first offending position. */
int32_t gulon_index_select_rows(gulon_index *idx, const int32_t *rows, int32_t s, gulon_index **out);
/* The rows as a bit mask of ceil(n / 64) 64-bit words in device memory: bit (r & 63) of word (r >> 6) selects row r,
 * bits at or above n are ignored.  Synchronises once to learn s.  gulon_index_select_mask_dev takes no stream: it works
 * on the null stream, so the mask must be complete before the call (a caller that wrote it on a stream of its own
 * synchronises that stream first). */
int32_t gulon_index_select_mask_dev(gulon_index *idx, const uint64_t *d_mask, gulon_index **out);
/* The same with the mask in host memory. */
int32_t gulon_index_select_mask(gulon_index *idx, const uint64_t *mask, gulon_index **out);
/* s, the rows (s entries, local rows of the root index) to the host, and the device array they live in (valid until
 * the view is destroyed).  On a handle that is not a view: GULON_ERR_INVALID_ARGUMENT.  gulon_index_view_rows_dev takes
 * no stream: it launches nothing, and the array it returns was completed on the null stream when the view was created. */
int32_t gulon_index_view_size(gulon_index *view, int32_t *s);
int32_t gulon_index_view_rows(gulon_index *view, int32_t *rows_out);
int32_t gulon_index_view_rows_dev(gulon_index *view, const int32_t **d_rows);
/* gulon_index_batch_query_dev / gulon_index_batch_query on the view (from / until are positions), the returned
 * positions translated to the root's row ids on the same stream. */
int32_t gulon_index_view_batch_query_dev(gulon_index *view, const float *d_queries, int32_t b, int32_t k_nn,
                                         int32_t from, int32_t until, int32_t *d_out_idx, float *d_out_dist,
                                         int32_t *d_out_count, int32_t *d_out_flags, void *stream);
int32_t gulon_index_view_batch_query(gulon_index *view, const float *queries, int32_t b, int32_t k_nn, int32_t from,
                                     int32_t until, int32_t *out_idx, float *out_dist, int32_t *out_count,
                                     int32_t *out_flags);
/* The translation alone, in place, for the answers of the other entry points (query by row, partial scans): every
 * d_idx[i] in [0, s) becomes the root's row id, anything else (-1 padding, INT32_MAX) stays. */
int32_t gulon_index_view_map_rows_dev(gulon_index *view, int32_t *d_idx, int64_t count, void *stream);

/* ---- Index updates (update.hip): new root indexes from an index's quantizer and from existing codes --------
 * The reference has no mutation: an updated index is the PQIndex it would hold over the merged EncodedMatrix.  Both
 * entries below give an ordinary root index (row_base 0, not a view) that owns all it reads -- codebooks copied device to
 * device -- so the sources may be destroyed first.  Sources may be views or contexts: they are read as the indexes they are.
 *
 * gulon_index_encode_dataset: PQIndex(pq, pq.encode(ds)) where pq is the quantizer `idx` holds in HBM
 * (ProductQuantizer.scala:25-35: per quantizer the serial KMeans.assign, one java.util.Random(0) stream over the rows of
 * `ds` in their order -- the path of gulon_pq_encode), the codes written straight into the device layout.  ds->d must
 * equal the index's d; ds->n = 0 is valid.  Nothing but the status reaches the host. */
int32_t gulon_index_encode_dataset(gulon_index *idx, const gulon_dataset *ds, gulon_index **out);
/* A root index of s rows: row p carries the code of a's row take[p] when take[p] >= 0, of b's row -1 - take[p]
 * otherwise -- any order, repeats allowed.  b may be NULL (then every entry is >= 0).  `take` (host) is checked before
 * anything is launched: every entry in range for its source, a and b equal in d, m, k and bitwise equal codebooks, else
 * GULON_ERR_INVALID_ARGUMENT (for an entry: naming the first offending position). */
int32_t gulon_index_merge(gulon_index *a, gulon_index *b, const int32_t *take, int32_t s, gulon_index **out);
/* EncodedMatrix.indices of local rows [from, until): out[j * (until - from) + (r - from)] = the code of row r at
 * quantizer j, for every code layout; a view answers in its own positions.  Un-blocked on the device from the plain code
 * buffer (never the filter's reordered copy), copied down once. */
int32_t gulon_index_get_codes(gulon_index *idx, int32_t from, int32_t until, uint16_t *out);

/* ---- Expression queries: stored rows composed on the device, operands dropped (compose.hip) ------------------------
 * An EXPRESSION is a non-empty list of terms (row, weight): LOCAL rows of the index (for a GroupedIndex: grouped row
 * positions) and binary32 weights.  b expressions are given in CSR form: term_offsets[b + 1] (term_offsets[0] = 0,
 * strictly ascending), term_rows[T] and term_weights[T] with T = term_offsets[b].  The composed vector of an expression:
 *   v_t = Index.lookup(row_t) -- gulon_index_decode_rows / gulon_grouped_index_lookup_rows (the partition by the
 *         reference's binarySearch rule) -- and, normalize_terms != 0, MathUtils.normalize(v_t);
 *   per coordinate e: acc = w_0 * v_0[e]; acc = acc + (w_t * v_t[e]) for t = 1, 2, ... in list order, every product and
 *         every sum rounded to binary32 on its own (no fma, no reassociation);
 *   normalize_query != 0: MathUtils.normalize of the sum (SortedIndex.prepare, Index.scala:324-331).
 * The handles carry no metric: a cosine index passes 1 for both flags, an l2 index 0 for both.  Nothing treats a zero
 * vector specially: it is a legitimate l2 query, normalises to NaN on a cosine index, and a NaN query is answered as
 * every NaN query is (GULON_FLAG_NONFINITE).  d * 4 <= 64 KiB, as for the row decode.
 * The host-pointer forms check b, the offsets and every row before launching anything (GULON_ERR_INVALID_ARGUMENT).
 * The _dev forms take device pointers and a stream, do not synchronise and cannot check: an expression without terms, or
 * with a term row outside [0, n), comes back as an all-NaN vector (its query as the query of an all-NaN vector) and
 * sets the handle's row-error word (gulon_index_row_error / gulon_grouped_index_row_error).
 *
 * gulon_*_compose_rows: the composed vectors, out [b][d]. */
int32_t gulon_index_compose_rows(gulon_index *idx, const int32_t *term_offsets, const int32_t *term_rows,
                                 const float *term_weights, int32_t b, int32_t normalize_terms,
                                 int32_t normalize_query, float *out);
int32_t gulon_index_compose_rows_dev(gulon_index *idx, const int32_t *d_term_offsets, const int32_t *d_term_rows,
                                     const float *d_term_weights, int32_t b, int32_t normalize_terms,
                                     int32_t normalize_query, float *d_out, void *stream);
int32_t gulon_grouped_index_compose_rows(gulon_grouped_index *idx, const int32_t *term_offsets,
                                         const int32_t *term_rows, const float *term_weights, int32_t b,
                                         int32_t normalize_terms, int32_t normalize_query, float *out);
int32_t gulon_grouped_index_compose_rows_dev(gulon_grouped_index *idx, const int32_t *d_term_offsets,
                                             const int32_t *d_term_rows, const float *d_term_weights, int32_t b,
                                             int32_t normalize_terms, int32_t normalize_query, float *d_out,
                                             void *stream);
/* gulon_*_query_terms: per expression (extra >= 0)
 *   1. the index's own answer to the composed vector at depth k_nn + extra: what gulon_index_batch_query_dev /
 *      gulon_grouped_index_batch_query_dev returns for it -- tie flags, the peeled (distance, row id) order above
 *      GULON_MAX_K and the limits and errors of the index form (k_nn + extra counts against them) included;
 *   2. every entry whose row is one of the expression's term rows is removed, the others keep their order;
 *   3. the first k_nn are kept.
 * Outputs as gulon_index_batch_query ([b][k_nn] idx/dist, -1 / +inf after the last entry; count[b]; flags[b], those of
 * step 1, nullable) and gulon_grouped_index_batch_query.  With extra = the number of distinct term rows of every
 * expression of the batch a full list can only fall short where step 1's does.  Everything runs on one stream (the
 * _dev forms: the caller's); nothing returns to the host in between. */
int32_t gulon_index_query_terms(gulon_index *idx, const int32_t *term_offsets, const int32_t *term_rows,
                                const float *term_weights, int32_t b, int32_t k_nn, int32_t extra,
                                int32_t normalize_terms, int32_t normalize_query, int32_t from, int32_t until,
                                int32_t *out_idx, float *out_dist, int32_t *out_count, int32_t *out_flags);
int32_t gulon_index_query_terms_dev(gulon_index *idx, const int32_t *d_term_offsets, const int32_t *d_term_rows,
                                    const float *d_term_weights, int32_t b, int32_t k_nn, int32_t extra,
                                    int32_t normalize_terms, int32_t normalize_query, int32_t from, int32_t until,
                                    int32_t *d_out_idx, float *d_out_dist, int32_t *d_out_count, int32_t *d_out_flags,
                                    void *stream);
int32_t gulon_grouped_index_query_terms(gulon_grouped_index *idx, const int32_t *term_offsets, const int32_t *term_rows,
                                        const float *term_weights, int32_t b, int32_t k_nn, int32_t extra,
                                        int32_t normalize_terms, int32_t normalize_query, int32_t strategy,
                                        int32_t limit, int32_t *out_idx, float *out_dist, int32_t *out_count);
int32_t gulon_grouped_index_query_terms_dev(gulon_grouped_index *idx, const int32_t *d_term_offsets,
                                            const int32_t *d_term_rows, const float *d_term_weights, int32_t b,
                                            int32_t k_nn, int32_t extra, int32_t normalize_terms,
                                            int32_t normalize_query, int32_t strategy, int32_t limit,
                                            int32_t *d_out_idx, float *d_out_dist, int32_t *d_out_count, void *stream);

/* Kernel timing for the roofline line of bench.py: when enabled, every scan-kernel
 * launch of this index is bracketed by hipEvents on the launch stream;
 * gulon_index_profile_read synchronises them and returns the summed duration. */
int32_t gulon_index_profile(gulon_index *idx, int32_t enable);
int32_t gulon_index_profile_read(gulon_index *idx, double *scan_ms_total, int32_t *launches);
/* Same, plus the number of rows the bracketed launches covered (the dominant kernel is the
 * quantized filter when it is active, the exact scan otherwise). */
int32_t gulon_index_profile_read_ex(gulon_index *idx, double *ms_total, int32_t *launches, int64_t *rows_total);
/* Of the last batch this handle ran through the quantized filter (synchronises the device): its query tiles
 * and how many of them the device-side safety net redid with the exact scan (unusable bound or survivor-queue
 * overflow).  query_tiles = 0: the batch took the exact scan. */
int32_t gulon_index_filter_stats(gulon_index *idx, int32_t *query_tiles, int32_t *tiles_redone);
/* Launch-shape / algorithm knobs of the scan, per handle (tests and tuning experiments).  A handle takes its settings
 * from the ENVIRONMENT when it is created -- the variable names are the keys: "GULON_SCAN_FILTER" (0/1),
 * "GULON_FILTER_MIN_RB", "GULON_FILTER_PERIOD", "GULON_FILTER_STAGE0", "GULON_FILTER_STAGE1", "GULON_FILTER_SAMPLE",
 * "GULON_FILTER_CAP", "GULON_FILTER_NADD", "GULON_FILTER_BLOCKS", "GULON_FILTER_SHARED_STAGE1", "GULON_SCAN_BLOCKS",
 * "GULON_SCAN_PRUNE", "GULON_SCAN_PRUNE_FROM" -- and this call changes them for ONE handle (and the contexts created
 * from it afterwards); there is no process-wide setter.  Results never depend on them.
 * "GULON_FILTER_ORDER" (default 1): an index of one-word codes (m <= 16) created while the environment's value is
 * non-zero keeps a second, conflict-ordered copy of its codes for the filter kernel (+ 17 bytes per row; the value =
 * rounds of the ordering); per handle 0 makes the filter read the plain copy again.
 * "GULON_FILTER_SORT" (default 1): such an index also keeps a copy of its codes sorted by the last two quantizers'
 * codes with a 32-bit row id per row (+ 20 bytes per row), which the filter reads for queries over the index's whole
 * row range; per handle 0 makes those queries read the other copies again.
 * "GULON_FILTER_PREFIX" (default 10): the filter's main stage on that copy tests a row on 10 of its 16 quantizers first
 * and looks up the other six only for rows some query of the tile may still keep; 0: all sixteen at once. */
int32_t gulon_index_tuning(gulon_index *idx, const char *key, int32_t value);
/* TopKHeap.merge semantics (TopKHeap.scala:44-53, used at Index.scala:279) under
 * the deterministic (distance, row id) order: merges `lists` partial lists per
 * query, laid out [lists][B][K+1], into the final K.  list_stride = elements
 * between consecutive lists (0 = B*(K+1), i.e. dense).  k_nn > GULON_MAX_K (lists from
 * gulon_index_scan_partial_dev at that k_nn): pairwise merges through scratch; synchronises the stream. */
int32_t gulon_topk_merge_dev(const float *d_part_dist, const int32_t *d_part_idx, int32_t lists,
                             int64_t list_stride, int32_t b, int32_t k_nn, int32_t *d_out_idx,
                             float *d_out_dist, int32_t *d_out_count, int32_t *d_out_flags, void *stream);
/* All-NaN queries on a ROW-SHARDED index: a query with a NaN component has every distance NaN
 * (Index.scala:352-383), the reference's heap then keeps the first min(K, n_total) rows it is offered
 * (TopKHeap.scala:69-79) and Result.fromHeap returns them as [1, ..., c-1, 0] with NaN distances.  Run on the
 * merged result of the shards (gulon_amd/sharded.py, gulon_sharded_index_batch_query); the unsharded
 * gulon_index_batch_query* handles every non-finite case itself (GULON_FLAG_NONFINITE). */
int32_t gulon_nan_queries_fix_dev(const float *d_queries, int32_t b, int32_t d, int32_t k_nn, int32_t n_total,
                                  int32_t *d_out_idx, float *d_out_dist, int32_t *d_out_count, int32_t *d_out_flags,
                                  void *stream);
/* host-pointer convenience form of the same merge */
int32_t gulon_topk_merge(const float *part_dist, const int32_t *part_idx, int32_t lists, int32_t b,
                         int32_t k_nn, int32_t *out_idx, float *out_dist, int32_t *out_count,
                         int32_t *out_flags);
/* Index.exactNearestNeighbours (Index.scala:209-229) + Result.fromHeap for B
 * queries over rows [from, until) of the dataset. */
int32_t gulon_exact_knn(const gulon_dataset *ds, int32_t from, int32_t until, const float *queries,
                        int32_t b, int32_t k_nn, int32_t *out_idx, float *out_dist, int32_t *out_count,
                        int32_t *out_flags);
/* MathUtils.distanceSq(query_q, X[rows[q][i]]) (MathUtils.scala:85-95) for the
 * recall harness (Tests.scala:18-41): out[B][K]; rows < 0 are skipped (0). */
int32_t gulon_distance_sq_rows(const gulon_dataset *ds, const float *queries, int32_t b,
                               const int32_t *rows, int32_t k_nn, float *out);
/* Tests.recallOf (Tests.scala:18-41) for a batch, evaluated on the device (recall.hip): rows[b][max_k] are the
 * dataset rows an index returned for each query, in result order, negative = none (padding after a short result).
 * For every query and every j < nks: out_tp[q][j] = #{p < ks[j] : rows[q][p] >= 0 and
 * MathUtils.distanceSq(query_q, X[rows[q][p]]) <= cutoffs[q][j]} (a NaN distance or cutoff counts nothing).
 * ks ascending, 1 <= ks[j] <= max_k <= GULON_MAX_K_PEELED, nks <= 16.  out_dist: NULL, or [b][max_k] for the
 * distances themselves (0 where there is no row), the same bits as gulon_distance_sq_rows.  A row >= n is
 * GULON_ERR_INVALID_ARGUMENT (found on the device; the outputs are then undefined). */
int32_t gulon_recall_counts(const gulon_dataset *ds, const float *queries, int32_t b, const int32_t *rows,
                            int32_t max_k, const int32_t *ks, int32_t nks, const float *cutoffs, int32_t *out_tp,
                            float *out_dist);
/* Exact re-ranking of candidate lists (refine.hip; DESIGN.md "Refined queries"): per query
 *   heap = TopKHeap(k_nn); for p = 0 .. c-1, in that order, with id = cand_rows[q][p] >= 0:
 *     heap.update(id, MathUtils.distanceSq(query_q, X[row_map ? row_map[id] : id]));   Result.fromHeap(heap)
 * (TopKHeap.scala:69-79, MathUtils.scala:85-95, Index.scala:83-94): ties and NaN as the heap decides them.
 * cand_rows[b][c]: an index's result rows in result order, negative = none; row_map[map_len] takes such a row to the row
 * of the dataset that holds the same vector (NULL: the identity; map_len is then ignored).  1 <= k_nn <= c <=
 * GULON_MAX_K_PEELED.  out_idx/out_dist: [b][k_nn], the candidates' OWN ids (not the mapped ones) and their exact
 * distances, ascending, -1 / 0 after the last entry; out_count[b] = entries.  A candidate >= map_len, or one whose
 * (mapped) row is outside [0, n), is GULON_ERR_INVALID_ARGUMENT (found on the device; the outputs are then undefined).
 * Device form: every pointer but ds is a device pointer, the work is enqueued on `stream` (hipStream_t) and not
 * synchronised, nothing is allocated.  It cannot return what the device finds: a query with such a candidate gets
 * d_out_count[q] = -1 (its other outputs are undefined) -- the caller's status word, to be tested after the stream. */
int32_t gulon_refine_topk(const gulon_dataset *ds, const float *queries, int32_t b, const int32_t *cand_rows,
                          int32_t c, const int32_t *row_map, int32_t map_len, int32_t k_nn, int32_t *out_idx,
                          float *out_dist, int32_t *out_count);
int32_t gulon_refine_topk_dev(const gulon_dataset *ds, const float *d_queries, int32_t b,
                              const int32_t *d_cand_rows, int32_t c, const int32_t *d_row_map, int32_t map_len,
                              int32_t k_nn, int32_t *d_out_idx, float *d_out_dist, int32_t *d_out_count,
                              void *stream);

/* ---- Index diagnostics (inspect.hip; DESIGN.md "Index diagnostics") -------------------------------------------------
 * Two computations over a device-resident index: how its code books are used, and how far its rows lie from the
 * vectors they were built from.  Rows are LOCAL rows of the index (for a GroupedIndex: grouped row positions; for a
 * view: its own positions), 0 <= from <= until <= n, else GULON_ERR_INVALID_ARGUMENT.  Both use scratch of their own
 * and leave no trace on the handle.
 *
 * gulon_*_code_histogram: out[j * k + c] (host, m * k entries) = the number of rows in [from, until) whose code at
 * quantizer j is c.  Integer arithmetic: exact; every quantizer's k counts sum to until - from. */
int32_t gulon_index_code_histogram(gulon_index *idx, int32_t from, int32_t until, int64_t *out);
int32_t gulon_grouped_index_code_histogram(gulon_grouped_index *idx, int32_t from, int32_t until, int64_t *out);
/* gulon_*_row_errors: for every row r in [from, until), with x = vectors[row_map ? row_map[r] : r] and y = the vector
 * the index's distances are about --
 *   flat index:    ProductQuantizer.decode of row r (ProductQuantizer.scala:37-50);
 *   grouped index: centroid(c) + decode(r), one fp32 add per coordinate (MathUtils.add, MathUtils.scala:63-71), c = the
 *                  group whose row range holds r, i.e. the group a query scans the row in.  This is NOT the partition
 *                  of gulon_grouped_index_lookup_rows: where offsets repeat (empty groups) the reference's binarySearch
 *                  rule can name another group --
 *   row_error[r - from]   = MathUtils.distanceSq(x, y) (MathUtils.scala:85-95): binary32, t = x_e - y_e; sum += t * t,
 *                           unfused, e ascending, one running sum -- the summand of ProductQuantizerSpec.quality
 *                           (ProductQuantizerSpec.scala:70-73);
 *   row_norm_sq[r - from] = the same sum with y = 0 (nullable);
 *   quantizer_error[j]    = the sum over those rows, in binary64, of the same binary32 sum restarted at 0 over the
 *                           coordinates of quantizer j only (gulon_subvectors); [m], host memory in both forms.
 * vectors->d must equal the index's; row_map (NULL: the identity, which needs vectors->n >= n) has map_len = n entries;
 * an entry of [from, until) outside [0, vectors->n) is GULON_ERR_INVALID_ARGUMENT, found on the device (nothing is read
 * for that row; the outputs are then undefined).  One 64-row block's codes must fit in LDS, as for
 * gulon_index_decode_dataset.  Device form: row_map and the per-row outputs are device pointers, the work is enqueued on
 * `stream` (hipStream_t), which is synchronised before the call returns (quantizer_error and the status come back). */
int32_t gulon_index_row_errors(gulon_index *idx, const gulon_dataset *vectors, const int32_t *row_map, int32_t map_len,
                               int32_t from, int32_t until, float *row_error, float *row_norm_sq,
                               double *quantizer_error);
int32_t gulon_index_row_errors_dev(gulon_index *idx, const gulon_dataset *vectors, const int32_t *d_row_map,
                                   int32_t map_len, int32_t from, int32_t until, float *d_row_error,
                                   float *d_row_norm_sq, double *quantizer_error, void *stream);
int32_t gulon_grouped_index_row_errors(gulon_grouped_index *idx, const gulon_dataset *vectors, const int32_t *row_map,
                                       int32_t map_len, int32_t from, int32_t until, float *row_error,
                                       float *row_norm_sq, double *quantizer_error);
int32_t gulon_grouped_index_row_errors_dev(gulon_grouped_index *idx, const gulon_dataset *vectors,
                                           const int32_t *d_row_map, int32_t map_len, int32_t from, int32_t until,
                                           float *d_row_error, float *d_row_norm_sq, double *quantizer_error,
                                           void *stream);

/* ---- Fine codes (fine.hip; DESIGN.md "Fine codes") -------------------------------------------------------------------
 * A second quantizer over the residuals an index leaves, and the index's candidates re-ranked against the two-level
 * reconstruction.  y_r is the vector the index's distances are about for row r, exactly as for gulon_*_row_errors: the
 * decode of row r for a flat index, centroid(g) + decode(r) for a grouped one (MathUtils.add, MathUtils.scala:63-71; g
 * the group whose row range holds r).  Rows are LOCAL rows (a view: its own positions).  Both calls use scratch of their
 * own and leave no trace on the handles.
 *
 * gulon_*_row_residuals: *out = a new device dataset of s x d with
 *   out[t][e] = vectors[vector_rows[t]][e] - y_{rows[t]}[e]     (MathUtils.subtract, MathUtils.scala:74-83: one binary32
 *                                                                subtraction per coordinate), t < s.
 * rows / vector_rows: host arrays of s entries, any order, repeats allowed.  Every entry is checked before anything is
 * launched: an entry outside [0, n) resp. [0, vectors->n) is GULON_ERR_INVALID_ARGUMENT, the message naming the first
 * offending position.  vectors->d must equal the index's.  s = 0 gives an empty dataset. */
int32_t gulon_index_row_residuals(gulon_index *idx, const gulon_dataset *vectors, const int32_t *rows,
                                  const int32_t *vector_rows, int32_t s, gulon_dataset **out);
int32_t gulon_grouped_index_row_residuals(gulon_grouped_index *idx, const gulon_dataset *vectors, const int32_t *rows,
                                          const int32_t *vector_rows, int32_t s, gulon_dataset **out);
/* gulon_*_refine_codes_topk: gulon_refine_topk with the two-level reconstruction in the place of the original vectors --
 * per query
 *   heap = TopKHeap(k_nn); for p = 0 .. c-1, in that order, with id = cand_rows[q][p] >= 0:
 *     z[e] = y_id[e] + decode_fine(fine_map ? fine_map[id] : id)[e]     (y_id[e] formed first, the fine coordinate added
 *                                                                        last: one binary32 add each)
 *     heap.update(id, MathUtils.distanceSq(query_q, z));   Result.fromHeap(heap)
 * (TopKHeap.scala:69-79, MathUtils.scala:85-95 -- the sum of (z_e - q_e)^2, e ascending, unfused -- Index.scala:83-94).
 * `fine` is an ordinary flat index over the residuals; the two handles must agree in d and in nothing else (m, k and code
 * layout are independent).  Arguments, outputs and conventions are those of gulon_refine_topk: negative candidates are
 * padding, 1 <= k_nn <= c <= GULON_MAX_K_PEELED (a larger c: GULON_ERR_UNSUPPORTED), out_idx the candidates' own ids,
 * -1 / 0 after a query's last entry.  A candidate outside the coarse index or the map, or whose fine row is outside
 * `fine`, is GULON_ERR_INVALID_ARGUMENT (found on the device; the outputs are then undefined).  Device form: every
 * pointer but the handles is a device pointer, the work is enqueued on `stream` and not synchronised, nothing is
 * allocated; a query with such a candidate gets d_out_count[q] = -1. */
int32_t gulon_index_refine_codes_topk(gulon_index *coarse, gulon_index *fine, const float *queries, int32_t b,
                                      const int32_t *cand_rows, int32_t c, const int32_t *fine_map, int32_t map_len,
                                      int32_t k_nn, int32_t *out_idx, float *out_dist, int32_t *out_count);
int32_t gulon_index_refine_codes_topk_dev(gulon_index *coarse, gulon_index *fine, const float *d_queries, int32_t b,
                                          const int32_t *d_cand_rows, int32_t c, const int32_t *d_fine_map,
                                          int32_t map_len, int32_t k_nn, int32_t *d_out_idx, float *d_out_dist,
                                          int32_t *d_out_count, void *stream);
int32_t gulon_grouped_index_refine_codes_topk(gulon_grouped_index *coarse, gulon_index *fine, const float *queries,
                                              int32_t b, const int32_t *cand_rows, int32_t c, const int32_t *fine_map,
                                              int32_t map_len, int32_t k_nn, int32_t *out_idx, float *out_dist,
                                              int32_t *out_count);
int32_t gulon_grouped_index_refine_codes_topk_dev(gulon_grouped_index *coarse, gulon_index *fine,
                                                  const float *d_queries, int32_t b, const int32_t *d_cand_rows,
                                                  int32_t c, const int32_t *d_fine_map, int32_t map_len, int32_t k_nn,
                                                  int32_t *d_out_idx, float *d_out_dist, int32_t *d_out_count,
                                                  void *stream);

/* ---- Rotated indexes (rotate.hip; DESIGN.md "Rotated indexes") -------------------------------------------------------
 * None of these is a Scala method: the reference has no rotation, so nothing here cites it.  An orthogonal d x d matrix R
 * is applied once to the data and once to each query; the index over the rotated rows is an ordinary index.
 *
 * rotate: out[i][c] = sum_j x[i][j] * R[j][c] (transpose != 0: R[c][j] in its place), in the project's arithmetic --
 * binary32, s = 0; for j ascending: s = s + (x[i][j] * R[j][c]); product and sum each rounded, nothing fused.  Non-finite
 * inputs propagate as IEEE 754 says.  Any d >= 1 and n >= 0 (n = 0 succeeds and launches nothing); `rotation` is d * d
 * row-major.  Otherwise GULON_ERR_INVALID_ARGUMENT.
 *   gulon_dataset_rotate    rotation in host memory; *out = a new device dataset of ds's shape (gulon_dataset_destroy)
 *   gulon_rotate_rows       x, rotation and out in host memory
 *   gulon_rotate_rows_dev   every pointer a device pointer, d_out != d_x; enqueued on `stream` (hipStream_t) and not
 *                           synchronised, nothing is allocated */
int32_t gulon_dataset_rotate(const gulon_dataset *ds, const float *rotation, int32_t transpose, gulon_dataset **out);
int32_t gulon_rotate_rows(const float *x, int32_t n, int32_t d, const float *rotation, int32_t transpose, float *out);
int32_t gulon_rotate_rows_dev(const float *d_x, int64_t n, int32_t d, const float *d_rotation, int32_t transpose,
                              float *d_out, void *stream);
/* moment: out[p * b->d + q] = sum_r a[r][p] * b[r][q], accumulated in binary64 (host memory, a->d * b->d doubles); the
 * two datasets must have the same number of rows.  The products are exact in binary64, only the additions round:
 * |out - exact| <= gamma_(n-1) * sum_r |a[r][p] * b[r][q]|.  The order of the additions is fixed by the source (chunks of
 * a constant number of rows, each summed r ascending, the chunks added in ascending order) and uses no atomics: the same
 * bits on every call and every device.  Zero rows give zeros. */
int32_t gulon_dataset_moment(const gulon_dataset *a, const gulon_dataset *b, double *out);

/* ---- The exact index (exact.hip; DESIGN.md "Exact index") ------------------------------------------------------------
 * Brute-force neighbours of rows [from, until) of a dataset behind a handle: what gulon_exact_knn answers -- squared L2
 * summed e ascending in unfused binary32, entries ascending in (distance, row id), count = min(k_nn, until - from) with
 * -1 / +inf after the last entry, GULON_FLAG_BOUNDARY_TIE / GULON_FLAG_INTERIOR_TIE -- the same rows, distance bits,
 * counts and flags for every query whose distances are all finite, 0 <= k_nn <= GULON_MAX_K_PEELED.  A query that meets
 * a NaN / +inf distance gets what gulon_exact_knn returns for it when asked alone.  k_nn <= GULON_MAX_K takes
 * gulon_exact_knn's single pass; a larger k_nn reads the rows ONCE (a sample pass bounds the (k_nn + 1)-th distance,
 * the main pass queues the rows at or below the bound, a selection sorts each queue) where gulon_exact_knn reads them
 * ceil((k_nn + 1) / 64) times; a query whose queue overflows is answered by that peeled path.
 *   create      the handle holds scratch, knobs and counters; it does NOT own the dataset, which must outlive it.
 *   batch_query host pointers; outputs as gulon_exact_knn (out_count / out_flags may be NULL).
 *   *_dev       device pointers, enqueued on `stream` (hipStream_t).  The outputs are complete only after the stream;
 *               the call itself waits for the stream once per batch, to read the per-query counters that decide
 *               whether fallback launches are needed, and may grow the handle's scratch.
 *   query_rows  the queries are rows of the DATASET (0 <= row < its rows, whatever [from, until) is), gathered on the
 *               device.  The host form checks every row before anything is launched (GULON_ERR_INVALID_ARGUMENT names
 *               the first bad one); in the device form such a row is a NaN query.
 *   tuning      keys "GULON_EXACT_SAMPLE" (sample rows S; 0 = chosen from k_nn, the range and the capacity) and
 *               "GULON_EXACT_QUEUE_CAP" (queue entries per query, default 32768); a handle reads the environment
 *               variables of the same names when it is created.  Results never depend on them.
 *   stats       of the last batch on the handle: out[0] queries answered in one pass, out[1] by the peeled fallback,
 *               out[2] one at a time as non-finite, out[3] S (0: no sample pass ran), out[4] the capacity, out[5] the
 *               largest number of rows at or below a query's bound (above out[4]: that queue overflowed).
 * One batch at a time per handle (calls are serialised); batches on different streams are ordered on the device. */
typedef struct gulon_exact_index gulon_exact_index;
int32_t gulon_exact_index_create(const gulon_dataset *ds, int32_t from, int32_t until, gulon_exact_index **out);
int32_t gulon_exact_index_destroy(gulon_exact_index *idx);
int32_t gulon_exact_index_batch_query(gulon_exact_index *idx, const float *queries, int32_t b, int32_t k_nn,
                                      int32_t *out_idx, float *out_dist, int32_t *out_count, int32_t *out_flags);
int32_t gulon_exact_index_batch_query_dev(gulon_exact_index *idx, const float *d_queries, int32_t b, int32_t k_nn,
                                          int32_t *d_out_idx, float *d_out_dist, int32_t *d_out_count,
                                          int32_t *d_out_flags, void *stream);
int32_t gulon_exact_index_query_rows(gulon_exact_index *idx, const int32_t *rows, int32_t b, int32_t k_nn,
                                     int32_t *out_idx, float *out_dist, int32_t *out_count, int32_t *out_flags);
int32_t gulon_exact_index_query_rows_dev(gulon_exact_index *idx, const int32_t *d_rows, int32_t b, int32_t k_nn,
                                         int32_t *d_out_idx, float *d_out_dist, int32_t *d_out_count,
                                         int32_t *d_out_flags, void *stream);
int32_t gulon_exact_index_tuning(gulon_exact_index *idx, const char *key, int32_t value);
int32_t gulon_exact_index_stats(gulon_exact_index *idx, int64_t *out);

/* ---- Expressions over the true vectors (dataset_compose.hip, exact.hip) ---------------------------------
 * gulon_dataset_compose_rows: the composed vectors of b expressions, out [b][d] -- the CSR input and the arithmetic of
 * gulon_index_compose_rows (above) with v_t = row row_t of the DATASET in the place of Index.lookup: optionally
 * MathUtils.normalize per term; per coordinate acc = w_0 * v_0[e], acc = acc + (w_t * v_t[e]) in list order, every product
 * and every sum its own binary32 operation; optionally MathUtils.normalize of the sum.  d * 4 <= 64 KiB.  The host form
 * checks b, the offsets and every row before anything is launched (GULON_ERR_INVALID_ARGUMENT names the first bad row).
 * The _dev form takes device pointers and a stream, does not synchronise and cannot check: an expression without terms,
 * or with a row outside [0, n), comes back as an all-NaN vector and sets *d_err = 1 (d_err may be NULL; the caller zeroes
 * it). */
int32_t gulon_dataset_compose_rows(const gulon_dataset *ds, const int32_t *term_offsets, const int32_t *term_rows,
                                   const float *term_weights, int32_t b, int32_t normalize_terms,
                                   int32_t normalize_query, float *out);
int32_t gulon_dataset_compose_rows_dev(const gulon_dataset *ds, const int32_t *d_term_offsets,
                                       const int32_t *d_term_rows, const float *d_term_weights, int32_t b,
                                       int32_t normalize_terms, int32_t normalize_query, float *d_out, int32_t *d_err,
                                       void *stream);
/* gulon_exact_index_query_terms: gulon_index_query_terms on the exact index.  Term rows are rows of the DATASET, as in
 * gulon_exact_index_query_rows and as the ids the index returns (from + slot).  Per expression (extra >= 0):
 *   1. the handle's own answer to the composed vector (gulon_dataset_compose_rows) at depth k_nn + extra: what
 *      gulon_exact_index_batch_query_dev returns for it -- flags, the one-pass path above GULON_MAX_K, its fallbacks and
 *      the non-finite rule included; k_nn + extra > GULON_MAX_K_PEELED is GULON_ERR_UNSUPPORTED;
 *   2. every entry whose row is one of the expression's term rows is removed (a term row outside [from, until) removes
 *      nothing), the others keep their order;
 *   3. the first k_nn are kept, -1 / +inf after the last; out_count per query; out_flags those of step 1 (both nullable).
 * Everything runs on one stream; the call waits for it once per batch, as gulon_exact_index_batch_query_dev does.  The
 * host form checks the term lists first; in the _dev form a bad expression is a NaN query.  gulon_exact_index_stats then
 * tells of step 1. */
int32_t gulon_exact_index_query_terms(gulon_exact_index *idx, const int32_t *term_offsets, const int32_t *term_rows,
                                      const float *term_weights, int32_t b, int32_t k_nn, int32_t extra,
                                      int32_t normalize_terms, int32_t normalize_query, int32_t *out_idx,
                                      float *out_dist, int32_t *out_count, int32_t *out_flags);
int32_t gulon_exact_index_query_terms_dev(gulon_exact_index *idx, const int32_t *d_term_offsets,
                                          const int32_t *d_term_rows, const float *d_term_weights, int32_t b,
                                          int32_t k_nn, int32_t extra, int32_t normalize_terms, int32_t normalize_query,
                                          int32_t *d_out_idx, float *d_out_dist, int32_t *d_out_count,
                                          int32_t *d_out_flags, void *stream);

/* ---- Analogy accuracy (analogy.hip) --------------------------------------------------------------------
 * Scores b answer lists against one expected row each.  idx_lists [b][kin] with counts[q] live entries (what a
 * *_query_terms call returns); expected[q] >= 0; section[q] in [0, nsections).
 *   rank(q) = the position of expected[q] among the first counts[q] entries of idx_lists[q], or -1;
 *   hits[section[q]][j] += 1 for every j < nks with 0 <= rank(q) < ks[j];   asked[section[q]] += 1.
 * hits [nsections][nks] and asked [nsections] are int32 and ACCUMULATE over calls: the caller zeroes them.  ks ascends
 * within [1, kin], nks <= 16, as for gulon_recall_counts.  out_rank [b]: NULL, or the ranks.  Integer atomics only: the
 * counters are the same whatever the order of the questions.  The host form checks ks, section and expected
 * (GULON_ERR_INVALID_ARGUMENT) and copies the counters up and down; the _dev form takes device pointers (ks too) and a
 * stream, does not synchronise, and counts a question with a section outside [0, nsections) nowhere. */
int32_t gulon_analogy_counts(const int32_t *idx_lists, const int32_t *counts, int32_t b, int32_t kin,
                             const int32_t *expected, const int32_t *section, const int32_t *ks, int32_t nks,
                             int32_t nsections, int32_t *hits, int32_t *asked, int32_t *out_rank);
int32_t gulon_analogy_counts_dev(const int32_t *d_idx_lists, const int32_t *d_counts, int32_t b, int32_t kin,
                                 const int32_t *d_expected, const int32_t *d_section, const int32_t *d_ks, int32_t nks,
                                 int32_t nsections, int32_t *d_hits, int32_t *d_asked, int32_t *d_out_rank,
                                 void *stream);

/* ---- Multiplicative analogy queries, 3CosMul (cosmul.hip) ------------------------------------------------
 * Levy & Goldberg's objective on the exact index and on a flat byte-code index.  Expressions are CSR term lists as in
 * gulon_index_query_terms; a term with weight > 0 is positive, any other negative.  Per expression with E terms and per
 * row r of the handle's range (the index: of [from, until)):
 *   q_t   = what the handle's *_compose_rows returns for [(row_t, 1.0)] with normalize_terms = normalize_query = normalize
 *           (the dataset row; the decoded row);
 *   d_t   = the bits the handle's ordinary query returns as the distance between q_t and r;
 *   s_t   = fmaxf(1 - 0.25 * d_t, 0): (1 + cos) / 2 on unit vectors, 0 for a NaN distance;
 *   P, N  = the products of the positive and of the negative terms' s_t in list order, the first factor starting each,
 *           N = 1 without a negative term;   score = P / (N + 0.001);   every operation rounded to binary32 on its own.
 * The answer: the rows that are no term rows by (score descending, row id ascending), the first k_nn.  out_idx [b][k_nn]
 * padded with -1, out_score [b][k_nn] padded with -inf, out_count [b] (nullable).  The order is total: no tie flags.  A
 * term row outside the range removes nothing but still scores.
 * Limits: 1 <= E <= 8, else GULON_ERR_UNSUPPORTED; k_nn + (largest E of the batch) <= GULON_MAX_K, else
 * GULON_ERR_UNSUPPORTED; the index: byte codes only (wide codes and views are GULON_ERR_UNSUPPORTED), and the tables of
 * one question, E * m_pad KiB, must fit in 144 KiB of LDS, else GULON_ERR_UNSUPPORTED naming m and E.
 * The host forms check b, the offsets, every row, |w_t| == 1, a positive term per expression
 * (GULON_ERR_INVALID_ARGUMENT) and the limits before anything is launched.  The _dev forms take device pointers and a
 * stream and do not synchronise: there an expression with no term, no positive term, a row outside the handle or
 * beyond a limit comes back with count 0 and nothing but padding, and sets *d_err (nullable) / the index's row-error
 * word (gulon_index_row_error). */
int32_t gulon_exact_index_query_cosmul(gulon_exact_index *idx, const int32_t *term_offsets, const int32_t *term_rows,
                                       const float *term_weights, int32_t b, int32_t k_nn, int32_t normalize,
                                       int32_t *out_idx, float *out_score, int32_t *out_count);
int32_t gulon_exact_index_query_cosmul_dev(gulon_exact_index *idx, const int32_t *d_term_offsets,
                                           const int32_t *d_term_rows, const float *d_term_weights, int32_t b,
                                           int32_t k_nn, int32_t normalize, int32_t *d_out_idx, float *d_out_score,
                                           int32_t *d_out_count, int32_t *d_err, void *stream);
int32_t gulon_index_query_cosmul(gulon_index *idx, const int32_t *term_offsets, const int32_t *term_rows,
                                 const float *term_weights, int32_t b, int32_t k_nn, int32_t normalize, int32_t from,
                                 int32_t until, int32_t *out_idx, float *out_score, int32_t *out_count);
int32_t gulon_index_query_cosmul_dev(gulon_index *idx, const int32_t *d_term_offsets, const int32_t *d_term_rows,
                                     const float *d_term_weights, int32_t b, int32_t k_nn, int32_t normalize,
                                     int32_t from, int32_t until, int32_t *d_out_idx, float *d_out_score,
                                     int32_t *d_out_count, void *stream);

/* ---- Word-pair similarity (pairs.hip) -------------------------------------------------------------------
 * gulon_*_pair_distances: for n pairs of row ids, out_dist[i] = MathUtils.distanceSq(y_a[i], y_b[i])
 * (MathUtils.scala:85-95): binary32, t = y_a[e] - y_b[e]; sum += t * t, unfused, e ascending, one running sum from 0 --
 * the arithmetic of gulon_index_row_errors.  y_r is the vector `lookup` returns for row r:
 *   gulon_index           ProductQuantizer.decode of the row (gulon_index_decode_rows); a view's rows are its positions;
 *   gulon_grouped_index   centroid + decode with the partition of GroupedIndex.lookup (gulon_grouped_index_lookup_rows),
 *                         NOT the row's own group that gulon_grouped_index_row_errors uses;
 *   gulon_dataset         the stored row as it is.
 * A row id outside [0, rows of the handle) is GULON_ERR_INVALID_ARGUMENT: the host form checks before anything is launched
 * and names the pair; the _dev form (device pointers, the work enqueued on `stream`, a hipStream_t, NULL allowed) finds
 * it on the device -- nothing is read for that pair, its distance is NaN -- and reports it when the call returns: the
 * _dev forms synchronise `stream` once.  n == 0 returns without touching the device.  The calls leave no scratch on a
 * handle. */
int32_t gulon_index_pair_distances(gulon_index *idx, const int32_t *rows_a, const int32_t *rows_b, int32_t n,
                                   float *out_dist);
int32_t gulon_index_pair_distances_dev(gulon_index *idx, const int32_t *d_rows_a, const int32_t *d_rows_b, int32_t n,
                                       float *d_out_dist, void *stream);
int32_t gulon_grouped_index_pair_distances(gulon_grouped_index *idx, const int32_t *rows_a, const int32_t *rows_b,
                                           int32_t n, float *out_dist);
int32_t gulon_grouped_index_pair_distances_dev(gulon_grouped_index *idx, const int32_t *d_rows_a,
                                               const int32_t *d_rows_b, int32_t n, float *d_out_dist, void *stream);
int32_t gulon_dataset_pair_distances(const gulon_dataset *ds, const int32_t *rows_a, const int32_t *rows_b, int32_t n,
                                     float *out_dist);
int32_t gulon_dataset_pair_distances_dev(const gulon_dataset *ds, const int32_t *d_rows_a, const int32_t *d_rows_b,
                                         int32_t n, float *d_out_dist, void *stream);
/* gulon_rank_sums: the integer sums of Spearman's rank correlation between x [n] and y [n], per section.  section [n]
 * holds ids, in any order; NULL: one section, and nsections must be 1.  A pair is LIVE if neither x[i] nor y[i] is NaN
 * and its section lies in [0, nsections).  For a live pair i, over the live pairs j of its section:
 *   less_x = #{j : x[j] < x[i]},  eq_x = #{j : x[j] == x[i]}  (IEEE comparisons: -0 == +0, an infinity ties with itself, i
 *   counts in eq),  cx = 2 * less_x + eq_x - n_s -- twice the centred average rank -- and cy likewise from y.
 * out [nsections][5] = {n_s, sum cx * cy, sum cx * cx, sum cy * cy, dropped}: n_s the section's live pairs, dropped its
 * pairs with a NaN.  out is overwritten.  Integer work only: exact, whatever the order.  0 <= n <= 2^20 (then every sum
 * stays below 2^60) and nsections >= 1, checked before any device call.  An all-pairs count, O(n^2).  The _dev form takes
 * device pointers (out too) and a stream and does not synchronise. */
int32_t gulon_rank_sums(const float *x, const float *y, const int32_t *section, int32_t n, int32_t nsections,
                        int64_t *out);
int32_t gulon_rank_sums_dev(const float *d_x, const float *d_y, const int32_t *d_section, int32_t n, int32_t nsections,
                            int64_t *d_out, void *stream);

/* ---- Offset queries and CSLS (offset.hip) ----------------------------------------------------------------
 * Neighbours by distance plus one number per row, on the exact index and on a flat byte-code index.  Per query q and per
 * row r of the handle's range (the index: of [from, until)):
 *   d = the bits the handle's ordinary query returns as the distance between q and r (the exact index: the sum of
 *       MathUtils.distanceSq; the index: the running sum over the quantizers' Index.prepareQuery tables, quantizer 0
 *       first, from 0);
 *   t = d + row_offsets[r], one binary32 addition.
 * row_offsets is indexed by the row: the exact index returns dataset rows and the array has the dataset's rows; the
 * index returns row_base + r for its row r and the array has the index's length, entry r for that row.  exclude
 * (nullable) holds per query one row id as the handle returns it, or -1.
 * A row is a candidate if and only if t is finite and its id is not exclude[q].  The answer: the candidates by
 * (t ascending, row id ascending; -0 equals +0), the first k_nn.  out_idx [b][k_nn] padded with -1, out_key [b][k_nn] = t
 * padded with +inf, out_count [b] (nullable).  The order is total: no tie flags.  An offset of +inf masks its row; the
 * same array serves a per-row prior, and CSLS retrieval (Conneau et al. 2018): on unit vectors CSLS(x, y) = 2 - d(x, y)
 * - r_T(x) - r_S(y), so ranking by d + r_S ascending is ranking by CSLS descending, r_S from gulon_mean_similarity.
 * Queries are taken as given (no normalisation).
 * Limits: 1 <= k_nn <= GULON_MAX_K, else GULON_ERR_UNSUPPORTED.  The index: byte codes only (wide codes and views are
 * GULON_ERR_UNSUPPORTED), and the tables of one query, m_pad KiB, must fit in 144 KiB of LDS, else GULON_ERR_UNSUPPORTED
 * naming m.
 * The host forms check b, k_nn, from / until, NaN or -inf in row_offsets and exclude outside -1 or the handle's row ids
 * (GULON_ERR_INVALID_ARGUMENT) before anything is launched.  The _dev forms take device pointers and a stream and neither
 * check the arrays nor synchronise: there a NaN or -inf offset makes t non-finite and so masks its row. */
int32_t gulon_exact_index_query_offset(gulon_exact_index *idx, const float *queries, int32_t b, int32_t k_nn,
                                       const float *row_offsets, const int32_t *exclude, int32_t *out_idx,
                                       float *out_key, int32_t *out_count);
int32_t gulon_exact_index_query_offset_dev(gulon_exact_index *idx, const float *d_queries, int32_t b, int32_t k_nn,
                                           const float *d_row_offsets, const int32_t *d_exclude, int32_t *d_out_idx,
                                           float *d_out_key, int32_t *d_out_count, void *stream);
int32_t gulon_index_query_offset(gulon_index *idx, const float *queries, int32_t b, int32_t k_nn, int32_t from,
                                 int32_t until, const float *row_offsets, const int32_t *exclude, int32_t *out_idx,
                                 float *out_key, int32_t *out_count);
int32_t gulon_index_query_offset_dev(gulon_index *idx, const float *d_queries, int32_t b, int32_t k_nn, int32_t from,
                                     int32_t until, const float *d_row_offsets, const int32_t *d_exclude,
                                     int32_t *d_out_idx, float *d_out_key, int32_t *d_out_count, void *stream);
/* The same on a GroupedIndex (grouped_offset.hip), over the handle's own distances.  The rows a query sees
 * are the rows of the groups gulon_grouped_index_batch_query searches for it at the same (strategy, limit) -- as a set;
 * rows of other groups are never candidates.  For such a row r, d = the bits that query returns for it: the residual
 * q - centroid(group) by MathUtils.subtract, Index.prepareQuery on the residual, the row's table entries summed quantizer
 * 0 first, from 0, unfused.  t = d + row_offsets[r], one binary32 addition; row_offsets has one entry per grouped row
 * position, exclude (nullable) one row position or -1 per query.  Candidates, order, padding and out_count as above;
 * queries are taken as given.  Everything is checked before anything is launched: b, NaN or -inf in row_offsets,
 * exclude outside -1 or [0, n), strategy and limit as the ordinary query checks them (GULON_ERR_INVALID_ARGUMENT);
 * 1 <= k_nn <= GULON_MAX_K, byte codes only, and the LDS bound of the ordinary query's group scan (160 KiB), else
 * GULON_ERR_UNSUPPORTED.  b = 0 and an index without rows succeed (no candidates: counts 0).  Host pointers only; the
 * work runs on the null stream and the call returns when the answers have arrived.  (A device-pointer form with a
 * stream is left to a later change.) */
int32_t gulon_grouped_index_query_offset(gulon_grouped_index *idx, const float *queries, int32_t b, int32_t k_nn,
                                         int32_t strategy, int32_t limit, const float *row_offsets,
                                         const int32_t *exclude, int32_t *out_idx, float *out_key, int32_t *out_count);
/* gulon_mean_similarity: the mean cosine similarity of each of b lists of squared distances between unit vectors,
 * dist_lists [b][kin] as a query returns them.  c = min(counts[q], K), or min(kin, K) when counts is NULL; out[q] = 0
 * when c == 0; else s_j = 1 - 0.5 * d_j, sum = s_0, sum = sum + s_j for j = 1 .. c - 1, out[q] = sum / (float)c, every
 * operation rounded to binary32 on its own.  b >= 0, kin >= 1, K >= 1 (GULON_ERR_INVALID_ARGUMENT).  The _dev form takes
 * device pointers and a stream and does not synchronise. */
int32_t gulon_mean_similarity(const float *dist_lists, const int32_t *counts, int32_t b, int32_t kin, int32_t K,
                              float *out);
int32_t gulon_mean_similarity_dev(const float *d_dist_lists, const int32_t *d_counts, int32_t b, int32_t kin, int32_t K,
                                  float *d_out, void *stream);

/* ---- Rank queries (rank.hip) ------------------------------------------------------------------------------
 * The counting twin of the offset query: not the first k_nn candidates, but how many candidates come before a given
 * one -- at any depth, without a list.  Candidates, keys and order are exactly those of "Offset queries and CSLS" above:
 * d the handle's own distance bits, t = d + row_offsets[r] in one binary32 addition, a row a candidate if and only if t is
 * finite and its id is not exclude[q] (nullable), the order (t ascending, row id ascending; -0 equals +0).  row_offsets
 * is indexed as there; NULL stands for +0.0 at every row.
 * Every query q has a gold list of zero or more row ids, as the handle returns them, in CSR form: gold_offsets[b + 1]
 * (gold_offsets[0] = 0, non-decreasing) and gold_rows[gold_offsets[b]].  Per query:
 *   out_row, out_key [b]   the best gold row -- the gold row that is a candidate and comes first in the order -- and its
 *                          t; -1 and +inf when no gold row is a candidate: the list is empty, or every row of it is
 *                          masked by +inf, is the excluded row or lies outside the range, or the query's distances are
 *                          not finite (a NaN query)
 *   out_rank [b]           the number of candidates strictly before the best gold row, -1 without one: the (0-based)
 *                          position of that row in the offset query's answer at any k_nn larger than it
 *   out_total [b]          (nullable) the number of candidates
 * All integers are exact; out_key carries the bits the offset query returns for that row.
 * Everything is checked before anything is launched: b, NaN or -inf in row_offsets, exclude outside -1 or the handle's
 * row ids, gold_offsets, and every gold row, which must be an id the handle returns -- the exact index: a row of its
 * dataset; the index: in [row_base, row_base + length) -- else GULON_ERR_INVALID_ARGUMENT naming the first bad entry.
 * The index: from / until and the limits of the offset query (byte codes only, no views, the tables of one query within
 * 144 KiB of LDS), else GULON_ERR_UNSUPPORTED.  b = 0 succeeds at once.
 * gulon_exact_index_query_rank and gulon_index_query_rank take host pointers only: the work runs on the null stream
 * and the call returns when the answers have arrived.  (Device-pointer forms with a stream, and their stream-contract
 * cases, are left to a later change.) */
int32_t gulon_exact_index_query_rank(gulon_exact_index *idx, const float *queries, int32_t b, const float *row_offsets,
                                     const int32_t *exclude, const int32_t *gold_offsets, const int32_t *gold_rows,
                                     int32_t *out_rank, int32_t *out_row, float *out_key, int32_t *out_total);
int32_t gulon_index_query_rank(gulon_index *idx, const float *queries, int32_t b, int32_t from, int32_t until,
                               const float *row_offsets, const int32_t *exclude, const int32_t *gold_offsets,
                               const int32_t *gold_rows, int32_t *out_rank, int32_t *out_row, float *out_key,
                               int32_t *out_total);

/* ---- Log-sum-exp queries and the inverted softmax (logsumexp.hip) ----------------------------------------
 * Not a Scala method.  Per query q and per row r of the handle's range [from, until):
 *   d        the handle's own distance bits (MathUtils.distanceSq order, binary32), as the ordinary query returns them
 *   term     r is a term if and only if d is finite and r != exclude[q] (exclude nullable; -1 excludes nothing)
 *   z, e     z = (double)d * (-0.5 * (double)beta), one binary64 product; e = exp(z) in binary64
 *   S_q      the sum of e over the terms, in binary64, in a fixed order: per lane the 256-row steps of its row chunk
 *            ascending, the lanes of a wave by an xor butterfly (32 down to 1), the waves in wave order, the chunks
 *            ascending.  No atomics
 *   out_lse [b]     L_q = log(S_q) in binary64; -inf for a query without a term, and for one whose terms all underflow
 *                   to 0 (beta too large for these distances)
 *   out_terms [b]   (nullable) the number of terms, exact
 * The bits of out_lse are a function of (range, queries, b, beta) alone: a used handle answers like a fresh one.  They
 * are NOT pinned across batch shapes: the number of row chunks follows the number of 16-query tiles of a pass (4096
 * queries at most), so the same query asked in a batch of another size may differ in its last bits.  Against the exactly
 * rounded sum of the same terms, |L - L_ref| <= 2^-40 + 4 ulp(L_ref) for ranges of up to 2^20 rows.
 * The offsets of the inverted softmax (Smith et al. 2017) follow from it.  On unit vectors cos = 1 - d / 2, and the rule
 * ranks target row y for source word x by beta * cos(x, y) - log sum_x' exp(beta * cos(x', y)), which is the ascending
 * order of t = d(x, y) + (2 / beta) * L(y) with L(y) = log sum_x' exp(-(beta / 2) * d(x', y)): an offset query
 * ("Offset queries and CSLS" above) with row_offsets[y] = (float)((2 / beta) * L(y)), L(y) this entry point's answer on
 * a handle over the SOURCE vectors with the target row y as the query.
 * Queries are taken as given (nothing is normalised).  Everything is checked before anything is launched: idx, b >= 0,
 * beta finite and > 0, every exclude[q] either -1 or a row of the dataset, queries and out_lse non-null when b > 0, else
 * GULON_ERR_INVALID_ARGUMENT naming the first bad entry.  b = 0 launches nothing.
 * gulon_exact_index_query_logsumexp takes host pointers only: the work runs on the null stream and the call returns when
 * the answers have arrived.  (A device-pointer form with a stream, and its stream-contract case, is left to a later
 * change.) */
int32_t gulon_exact_index_query_logsumexp(gulon_exact_index *idx, const float *queries, int32_t b, float beta,
                                          const int32_t *exclude, double *out_lse, int32_t *out_terms);

/* ---- Alignment (alignment.hip) ---------------------------------------------------------------------------
 * Not Scala methods: the reference aligns nothing.  The two device steps of learning an orthogonal map between two
 * embedding spaces (MUSE's Procrustes refinement) that the entry points above do not cover.
 *
 * pair moment: out[p * b->d + q] = sum_i a[rows_a[i]][p] * b[rows_b[i]][q] over i in [0, n), accumulated in binary64
 * (host memory, a->d * b->d doubles) -- gulon_dataset_moment over a list of row pairs of two datasets that may differ in
 * rows and in dimension.  A pair with a negative row on either side adds nothing and is not counted; *out_used (host)
 * is the number of pairs that were.  Duplicates and any order are allowed.  The products are exact in binary64, only the
 * additions round, and their order is fixed by the source as for gulon_dataset_moment: the list is cut BY POSITION into
 * chunks of 4096 pairs (a skipped pair keeps its position and adds +0), each chunk summed i ascending from 0.0, the chunk
 * sums added in ascending chunk order, no atomics on floating-point values: the same bits on every call and every
 * device, and with rows_a = rows_b = 0 .. n - 1 over two datasets of n rows the bits of gulon_dataset_moment.
 * n = 0 gives zeros and *out_used = 0.  Null pointers (the lists may be null when n = 0), n < 0: GULON_ERR_INVALID_ARGUMENT.
 *   gulon_dataset_pair_moment       the lists in host memory; a row >= its dataset's row count is
 *                                   GULON_ERR_INVALID_ARGUMENT, before anything is launched
 *   gulon_dataset_pair_moment_dev   the lists in device memory, trusted: a row beyond its dataset is read out of bounds.
 *                                   Runs on the null stream and returns when out and *out_used have arrived
 *
 * mutual rows: out[s] = fwd[s] if 0 <= fwd[s] < nt and bwd[fwd[s]] == s, else -1, for s in [0, ns): fwd [ns] each
 * source row's best target row, bwd [nt] each target row's best source row, out [ns] the pairs that chose each other.
 * Elementwise, nothing is compacted: the pair moment skips the -1.  ns, nt >= 0; entries of fwd outside [0, nt) (-1: a
 * query without an answer) give -1.  The _dev form takes device pointers, is enqueued on `stream` (hipStream_t),
 * allocates nothing and does not synchronise. */
int32_t gulon_dataset_pair_moment(const gulon_dataset *a, const gulon_dataset *b, const int32_t *rows_a,
                                  const int32_t *rows_b, int64_t n, double *out, int64_t *out_used);
int32_t gulon_dataset_pair_moment_dev(const gulon_dataset *a, const gulon_dataset *b, const int32_t *d_rows_a,
                                      const int32_t *d_rows_b, int64_t n, double *out, int64_t *out_used);
int32_t gulon_mutual_rows(const int32_t *fwd, int32_t ns, const int32_t *bwd, int32_t nt, int32_t *out);
int32_t gulon_mutual_rows_dev(const int32_t *d_fwd, int32_t ns, const int32_t *d_bwd, int32_t nt, int32_t *d_out,
                              void *stream);
#ifdef GULON_TEST_HOOKS   /* libgulon_hip_testhooks.so only */
/* The launch geometry of the 3CosMul scans (cosmul.hip), by the arithmetic their launchers run; host code, nothing is
 * launched.  b >= 1 questions.  Flat index, rows [from, until): out = {questions per pass, row chunks of the first
 * pass, 64-row code blocks per chunk}.  Exact index, the handle's range: out = {questions per pass, row chunks of the
 * first pass, 256-row groups per chunk}. */
int32_t gulon_selftest_cosmul_flat_shape(const gulon_index *idx, int32_t b, int32_t from, int32_t until, int32_t out[3]);
int32_t gulon_selftest_cosmul_exact_shape(const gulon_exact_index *idx, int32_t b, int32_t out[3]);
#endif

#ifdef __cplusplus
}
#endif
#endif /* GULON_HIP_H */
