// Multiplicative analogy queries, 3CosMul (Levy & Goldberg 2014).  Per expression with terms
// (row_t, w_t), t = 0 .. E-1, and per candidate row r:
//   d_t(r)  the distance the handle's ordinary query returns between q_t (the term's vector as *_compose_rows gives it
//           for the one-term expression [(row_t, 1)]) and r;
//   s_t(r)  = fmaxf(1 - 0.25 * d_t, 0)                    (on unit vectors (1 + cos) / 2; a NaN distance gives 0)
//   P, N    the products of the s_t of the positive (w_t > 0) and of the other terms in list order, the first factor
//           starting each; N = 1 without a negative term
//   score   = P / (N + 0.001)
// every operation a binary32 rounding of its own (expressions.cosmul_reference restates it).  The answer: the rows that
// are no term rows by (score descending, row id ascending).
//
//   cosmul_plan        one workgroup: which expressions are unusable, the slots per question E' = the largest E rounded
//                      up to 1, 2, 4 or 8, and the terms as one-term expressions for the compose launchers
//   (compose)          q_t for every term slot: launch_dataset_compose / gulon_index_compose_rows_dev
//   exact index        cosmul_transpose: q_t of the 16 / E' questions of a workgroup -> Qt; cosmul_exact_scan: the d_t by
//                      exact_tile (exact.hpp), its 16 accumulators = the term slots of 16 / E' questions
//   flat index         launch_build_tables: Index.prepareQuery of every q_t; cosmul_flat_scan: a workgroup is (question,
//                      row chunk), the flat table scan (table_scan.hpp) over the question's E tables, one sum per term
//   both               after the sums the score, and the key -score into the question's WaveList (wave_offer), which
//                      orders by (key ascending, row ascending); the workgroup's lists merged (merge_wave_lists) into
//                      the chunk's; launch_merge: the row chunks' lists -> one list of depth
//                      kin = min(k_nn + 8, 63); launch_drop (compose.hip's kernel): the term rows removed, the first
//                      k_nn kept; cosmul_negate: key -> score (the +inf padding becomes -inf)
// E' is known on the device only (the *_dev forms do not synchronise), so the exact scan is launched once per E' and the
// launches that do not match leave at once.
#include "cosmul.hpp"
#include "exact.hpp"

namespace gulon {
namespace {

constexpr int PLAN_THREADS = 256;

// plan[0] = E', plan[1] = T, the term slots in use, plan[2] = off[0]: slot s is term off[0] + s of the caller's lists.
// Every slot is a usable one-term expression for the compose launchers: a slot that is not in use, or whose row is
// outside [0, n), asks for row 0.
__global__ __launch_bounds__(PLAN_THREADS) void cosmul_plan(const int *__restrict__ off, const int *__restrict__ rows,
                                                            const float *__restrict__ w, int b, int n, int tcap,
                                                            int k_nn, int max_terms, int *__restrict__ plan,
                                                            int *__restrict__ bad, int *__restrict__ uoff,
                                                            int *__restrict__ urows, float *__restrict__ ones,
                                                            int *__restrict__ err) {
  __shared__ int emax, anybad;
  const int tid = threadIdx.x;
  if (tid == 0) { emax = 1; anybad = 0; }
  __syncthreads();
  const int base = off[0];
  const int T = min(max(off[b] - base, 0), tcap);
  for (int q = tid; q < b; q += PLAN_THREADS) {
    const int t0 = off[q], t1 = off[q + 1], E = t1 - t0;
    bool u = E < 1 || E > max_terms || k_nn + E > GULON_MAX_K || t0 < base || t1 - base > tcap;
    bool pos = false;
    if (!u)
      for (int t = t0; t < t1; t++) {
        const int row = rows[t];
        u = u || row < 0 || row >= n;
        pos = pos || w[t] > 0.f;
      }
    u = u || !pos;
    bad[q] = u ? 1 : 0;
    if (u) atomicOr(&anybad, 1); else atomicMax(&emax, E);
  }
  for (int s = tid; s <= tcap; s += PLAN_THREADS) {
    uoff[s] = s;
    if (s < tcap) {
      const int row = s < T ? rows[base + s] : 0;
      urows[s] = (row >= 0 && row < n) ? row : 0;
      ones[s] = 1.f;
    }
  }
  __syncthreads();
  if (tid == 0) {
    plan[0] = emax <= 1 ? 1 : emax <= 2 ? 2 : emax <= 4 ? 4 : 8;
    plan[1] = T;
    plan[2] = base;
    if (anybad && err) *err = 1;
  }
}

// The key of one row: -score.  at(t) is d_t; ne terms, bit t of pos set for a positive one.
template <int EP, class At>
__device__ __forceinline__ float cosmul_key(At at, int ne, unsigned pos) {
  float P = 0.f, N = 1.f;
  bool hp = false, hn = false;
#pragma unroll
  for (int t = 0; t < EP; t++) {
    if (t < ne) {   // (wave-uniform)
      const float s = fmaxf(__fsub_rn(1.f, __fmul_rn(0.25f, at(t))), 0.f);
      if ((pos >> t) & 1u) { P = hp ? __fmul_rn(P, s) : s; hp = true; }
      else { N = hn ? __fmul_rn(N, s) : s; hn = true; }
    }
  }
  return -__fdiv_rn(P, __fadd_rn(N, 0.001f));
}

// A question's number of terms (0: unusable, nothing to answer), the mask of its positive ones and its first term.
__device__ __forceinline__ void question_terms(const int *__restrict__ bad, const int *__restrict__ off,
                                               const float *__restrict__ tw, int q, int b, int cap, int &ne,
                                               unsigned &pos, int &t0) {
  ne = 0; pos = 0u; t0 = 0;
  if (q < b && !bad[q]) {
    t0 = off[q];
    ne = min(off[q + 1] - t0, cap);
    for (int t = 0; t < ne; t++) pos |= tw[t0 + t] > 0.f ? 1u << t : 0u;
  }
  ne = __builtin_amdgcn_readfirstlane(ne);
  pos = (unsigned)__builtin_amdgcn_readfirstlane((int)pos);
  t0 = __builtin_amdgcn_readfirstlane(t0);
}

// ---- exact index ------------------------------------------------------------------------------------------------------

// Qt (exact.hpp) of the term vectors: slot u of a tile is term u % E' of its question u / E'; a slot without a term
// holds zeros.
__global__ void cosmul_transpose(const float *__restrict__ Q1, const int *__restrict__ off, const int *__restrict__ bad,
                                 const int *__restrict__ plan, int b, int d, float *__restrict__ Qt) {
  const int EP = plan[0], QW = KNN_QT / EP, base = plan[2];
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long total = (long long)((b + QW - 1) / QW) * d * KNN_QT;
  if (t >= total) return;
  const int u = (int)(t % KNN_QT);
  const int dim = (int)((t / KNN_QT) % d);
  const int tile = (int)(t / ((long long)KNN_QT * d));
  const int q = tile * QW + u / EP, tt = u % EP;
  float v = 0.f;
  if (q < b && !bad[q]) {
    const int t0 = off[q];
    if (tt < off[q + 1] - t0) v = Q1[(size_t)(t0 - base + tt) * d + dim];
  }
  Qt[t] = v;
}

template <int EP>
__global__ __launch_bounds__(KNN_THREADS) void cosmul_exact_scan(const float *__restrict__ X, int n, int d,
                                                                 const float *__restrict__ Qt,
                                                                 const int *__restrict__ plan,
                                                                 const int *__restrict__ bad,
                                                                 const int *__restrict__ off,
                                                                 const float *__restrict__ tw, int b, int row_from,
                                                                 int row_until, int rows_per_chunk, int nchunks,
                                                                 int keff, float *__restrict__ part_v,
                                                                 int *__restrict__ part_i) {
  if (plan[0] != EP) return;   // (uniform over the launch)
  constexpr int QW = KNN_QT / EP;
  constexpr int NW = KNN_THREADS / 64;
  __shared__ float xs[KNN_THREADS * (KNN_DT + 1)];
  __shared__ float sv[QW * NW * 64];
  __shared__ int si[QW * NW * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tile = blockIdx.x, chunk = blockIdx.y;
  const float *qt = Qt + (size_t)tile * d * KNN_QT;

  int ne[QW];
  unsigned pos[QW];
  WaveList wl[QW];
  int cnt[QW];
#pragma unroll
  for (int u = 0; u < QW; u++) {
    int t0;
    question_terms(bad, off, tw, tile * QW + u, b, EP, ne[u], pos[u], t0);
    wl[u].init(); cnt[u] = 0;
  }

  const int r0 = (row_from / KNN_THREADS) * KNN_THREADS + chunk * rows_per_chunk;
  const int r1 = min(row_until, r0 + rows_per_chunk);
  for (int base = r0; base < r1; base += KNN_THREADS) {
    float acc[KNN_QT];
    exact_tile(X, n, d, qt, xs, tid, [&](int r) { return base + r; }, acc);
    const int row = base + tid;
    const bool valid = row >= row_from && row < row_until;
    const unsigned long long vmask = __ballot(valid);
#pragma unroll
    for (int u = 0; u < QW; u++) {
      if (ne[u] == 0) continue;   // (wave-uniform)
      const float key = cosmul_key<EP>([&](int t) { return acc[u * EP + t]; }, ne[u], pos[u]);
      wave_offer(wl[u], cnt[u], key, valid, vmask, base + wave * 64, keff, lane);
    }
  }
  __syncthreads();
  merge_wave_lists<QW, NW>(wl, sv, si, keff, lane, wave, [&](int u, const WaveList &out) {
    if (lane < keff) {   // (every question slot of the tile has its lists: part_* hold ceil(b / 16) * 16 questions)
      const size_t o = ((size_t)(tile * QW + u) * nchunks + chunk) * keff + lane;
      part_v[o] = out.v;
      part_i[o] = out.i;
    }
  });
}

__global__ void cosmul_negate(float *__restrict__ v, long long n) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) v[t] = -v[t];
}

template <int EP>
void launch_exact_ep(const gulon_dataset *ds, CosmulWork &x, const int *d_off, const float *d_w, int b, int from,
                     int until, int rows_per_chunk, int nchunks, int keff, hipStream_t st) {
  hipLaunchKernelGGL(cosmul_exact_scan<EP>, dim3(ceil_div(b, KNN_QT / EP), nchunks), dim3(KNN_THREADS), 0, st, ds->x.p,
                     ds->n, ds->d, x.qt.p, x.plan.p, x.bad.p, d_off, d_w, b, from, until, rows_per_chunk, nchunks, keff,
                     x.pv.p, x.pi.p);
}

// merge -> drop -> negate: the tail of both forms, for the b questions whose chunk lists are in x.pv / x.pi
void finish_lists(CosmulWork &x, int nchunks, int keff, int b, int kin, int k_nn, const int *d_off, const int *d_rows,
                  int row_base, int *out_idx, float *out_score, int *out_count, hipStream_t st) {
  launch_merge(x.pv.p, x.pi.p, nchunks, (long long)keff, (long long)nchunks * keff, b, kin,
               QueryOut::final_lists(x.oi.p, x.od.p, x.oc.p, nullptr), st);
  launch_drop(x.oi.p, x.od.p, x.oc.p, b, kin, k_nn, d_off, d_rows, row_base, out_idx, out_score, out_count, st);
  const long long bk = (long long)b * k_nn;
  if (bk > 0) {
    hipLaunchKernelGGL(cosmul_negate, dim3(ceil_div(bk, 256)), dim3(256), 0, st, out_score, bk);
    HIP_CHECK(hipGetLastError());
  }
}

void check_dev_shape(int b, int k_nn, const int *d_off, const int *d_rows, const float *d_w, const int *out_idx,
                     const float *out_score) {
  GULON_REQUIRE(b >= 0 && k_nn >= 0, "k and batch size must be non-negative");
  GULON_UNSUPPORTED(k_nn + 1 > GULON_MAX_K, "k_nn + terms = %d + 1 > %d", k_nn, GULON_MAX_K);
  GULON_REQUIRE(b == 0 || (d_off != nullptr && d_rows != nullptr && d_w != nullptr && out_idx != nullptr &&
                           out_score != nullptr), "null argument");
}

// ---- flat index -------------------------------------------------------------------------------------------------------

// A workgroup is (question, row chunk): the tables of the question's ne terms in LDS and the flat table scan over them
// (table_scan.hpp), instantiated for every ne; after the sums the key -score into the question's WaveList.
template <int VEC>
__global__ __launch_bounds__(TABLE_SCAN_THREADS) void cosmul_flat_scan(
    const uint8_t *__restrict__ codes, int ng, int m_pad, const float *__restrict__ tables, const int *__restrict__ plan,
    const int *__restrict__ bad, const int *__restrict__ off, const float *__restrict__ tw, int b, int lds_terms,
    int row_from, int row_until, int row_base, int rb_begin, int rb_end, int rb_per_chunk, int nchunks, int keff,
    float *__restrict__ part_v, int *__restrict__ part_i) {
  constexpr int NW = TABLE_SCAN_THREADS / 64;
  extern __shared__ float4 lds4[];
  __shared__ float sv[NW * 64];
  __shared__ int si[NW * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q = blockIdx.x, chunk = blockIdx.y;
  const int tab = m_pad * 256;
  int ne, t0;
  unsigned pos;
  question_terms(bad, off, tw, q, b, lds_terms, ne, pos, t0);
  WaveList wl;
  wl.init();
  int cnt = 0;
  if (ne > 0) {   // (uniform over the workgroup)
    stage_tables(lds4, tables + (size_t)(t0 - plan[2]) * tab, tab, ne, ne, tid);
    const int rb0 = rb_begin + chunk * rb_per_chunk, rb1 = min(rb_end, rb0 + rb_per_chunk);
    auto rows = [&](auto e) {
      constexpr int E = decltype(e)::value;
      table_scan_rows<E, VEC>(codes, ng, tab, reinterpret_cast<const float *>(lds4), rb0, rb1, lane, wave,
                              [&](int rb, const float (&acc)[E]) {
        const int row = rb * 64 + lane;
        const bool valid = row >= row_from && row < row_until;
        const float key = cosmul_key<E>([&](int t) { return acc[t]; }, E, pos);
        wave_offer(wl, cnt, key, valid, __ballot(valid), rb * 64 + row_base, keff, lane);
      });
    };
#define CF_ROWS(EE) rows(std::integral_constant<int, EE>{})
    switch (ne) {
      case 1: CF_ROWS(1); break;
      case 2: CF_ROWS(2); break;
      case 3: CF_ROWS(3); break;
      case 4: CF_ROWS(4); break;
      case 5: CF_ROWS(5); break;
      case 6: CF_ROWS(6); break;
      case 7: CF_ROWS(7); break;
      default: CF_ROWS(8); break;
    }
#undef CF_ROWS
  }
  merge_wave_lists<1, NW>(&wl, sv, si, keff, lane, wave, [&](int, const WaveList &out) {
    if (lane < keff) {
      const size_t o = ((size_t)q * nchunks + chunk) * keff + lane;
      part_v[o] = out.v;
      part_i[o] = out.i;
    }
  });
}

void rethrow(int32_t rc) {   // a nested entry point has recorded its message
  if (rc != GULON_OK) throw DeviceError{rc};
}

}  // namespace

int check_cosmul_host(const int32_t *off, const int32_t *rows, const float *w, int b, int n, int k_nn, int *emax) {
  GULON_REQUIRE(k_nn >= 0, "k must be non-negative");
  const int terms = check_terms_host(off, rows, w, b, n);
  int em = 0;
  for (int q = 0; q < b; q++) {
    const int E = off[q + 1] - off[q];
    GULON_UNSUPPORTED(E > COSMUL_MAX_TERMS, "expression %d has %d terms, at most %d are supported", q, E,
                      COSMUL_MAX_TERMS);
    bool pos = false;
    for (int t = off[q]; t < off[q + 1]; t++) {
      GULON_REQUIRE(w[t] == 1.f || w[t] == -1.f, "term %d: weight %g, a cosmul term weighs +1 or -1", t, (double)w[t]);
      pos = pos || w[t] > 0.f;
    }
    GULON_REQUIRE(pos, "expression %d has no positive term", q);
    em = std::max(em, E);
  }
  GULON_UNSUPPORTED(b > 0 && k_nn + em > GULON_MAX_K, "k_nn + terms = %d + %d > %d", k_nn, em, GULON_MAX_K);
  if (emax) *emax = em;
  return terms;
}

CosmulShape cosmul_exact_shape(int from, int until, int b) {
  const int nb = std::min(EXACT_SUB_BATCH, b);
  // about 2048 workgroups at four questions each, whatever E' turns out to be
  const RowChunks c = knn_row_chunks(from, until, ceil_div(nb, 4));
  return {EXACT_SUB_BATCH, c.nchunks, c.groups_per_chunk};
}

CosmulShape cosmul_flat_shape(const gulon_index *ix, int from, int until, int b) {
  constexpr int NW = TABLE_SCAN_THREADS / 64;
  const size_t tab = (size_t)ix->m_pad * 256;
  const int sub = (int)std::max<size_t>(1, FLAT_TABLE_BYTES / ((size_t)COSMUL_MAX_TERMS * tab * sizeof(float)));
  const int nb = std::min(sub, b);
  const int rb_total = ceil_div(until, 64) - from / 64;
  const int want = std::max(1, ceil_div(2048, nb));
  const int nchunks_max = std::max(1, rb_total / (2 * NW));
  const int rb_per_chunk = std::max(1, ceil_div(rb_total, std::min(want, nchunks_max)));
  return {sub, std::max(1, ceil_div(rb_total, rb_per_chunk)), rb_per_chunk};
}

void launch_cosmul_exact(const gulon_dataset *ds, int from, int until, CosmulWork &x, const int *d_off, const int *d_rows,
                         const float *d_w, int b, int k_nn, bool normalize, int *out_idx, float *out_score,
                         int *out_count, int *d_err, hipStream_t st) {
  check_dev_shape(b, k_nn, d_off, d_rows, d_w, out_idx, out_score);
  if (b == 0) return;
  const int d = ds->d;
  const int kin = std::min(k_nn + COSMUL_MAX_TERMS, GULON_MAX_K), keff = kin + 1;
  for (int q0 = 0; q0 < b; q0 += EXACT_SUB_BATCH) {
    const int nb = std::min(EXACT_SUB_BATCH, b - q0), tcap = nb * COSMUL_MAX_TERMS;
    const int *off = d_off + q0;
    const CosmulShape shape = cosmul_exact_shape(from, until, nb);
    const int nchunks = shape.nchunks;
    const int rows_per_chunk = shape.per_chunk * KNN_THREADS;
    const int bp = ceil_div(nb, KNN_QT) * KNN_QT;                 // questions the lists are kept for, at any E'
    const size_t qt_len = (size_t)ceil_div(nb, 2) * d * KNN_QT;   // E' = 8: two questions per tile
    x.plan.ensure(3); x.bad.ensure(nb);
    x.uoff.ensure((size_t)tcap + 1); x.urows.ensure(tcap); x.ones.ensure(tcap);
    x.q.ensure((size_t)tcap * d); x.qt.ensure(qt_len);
    x.pv.ensure((size_t)bp * nchunks * keff); x.pi.ensure((size_t)bp * nchunks * keff);
    x.oi.ensure((size_t)nb * kin); x.od.ensure((size_t)nb * kin); x.oc.ensure(nb);
    hipLaunchKernelGGL(cosmul_plan, dim3(1), dim3(PLAN_THREADS), 0, st, off, d_rows, d_w, nb, ds->n, tcap, k_nn,
                       COSMUL_MAX_TERMS, x.plan.p, x.bad.p, x.uoff.p, x.urows.p, x.ones.p, d_err);
    HIP_CHECK(hipGetLastError());
    launch_dataset_compose(ds, x.uoff.p, x.urows.p, x.ones.p, tcap, normalize, normalize, x.q.p, nullptr, st);
    hipLaunchKernelGGL(cosmul_transpose, dim3(ceil_div((long long)qt_len, 256)), dim3(256), 0, st, x.q.p, off, x.bad.p,
                       x.plan.p, nb, d, x.qt.p);
    launch_exact_ep<1>(ds, x, off, d_w, nb, from, until, rows_per_chunk, nchunks, keff, st);
    launch_exact_ep<2>(ds, x, off, d_w, nb, from, until, rows_per_chunk, nchunks, keff, st);
    launch_exact_ep<4>(ds, x, off, d_w, nb, from, until, rows_per_chunk, nchunks, keff, st);
    launch_exact_ep<8>(ds, x, off, d_w, nb, from, until, rows_per_chunk, nchunks, keff, st);
    HIP_CHECK(hipGetLastError());
    finish_lists(x, nchunks, keff, nb, kin, k_nn, off, d_rows, 0, out_idx + (size_t)q0 * k_nn,
                 out_score + (size_t)q0 * k_nn, out_count ? out_count + q0 : nullptr, st);
  }
}

int cosmul_flat_max_terms(const gulon_index *ix) {
  const size_t per_term = (size_t)ix->m_pad * 256 * sizeof(float);
  return (int)std::min<size_t>(COSMUL_MAX_TERMS, TABLE_LDS_BUDGET / per_term);
}

void launch_cosmul_flat(gulon_index *ix, CosmulWork &x, const int *d_off, const int *d_rows, const float *d_w, int b,
                        int k_nn, bool normalize, int from, int until, int lds_terms, int *out_idx, float *out_score,
                        int *out_count, bool dev_rows, hipStream_t st) {
  check_dev_shape(b, k_nn, d_off, d_rows, d_w, out_idx, out_score);
  GULON_UNSUPPORTED(ix->wide, "cosmul queries take byte codes: k = %d > 256 is not supported", ix->k);
  GULON_UNSUPPORTED(ix->is_view, "cosmul queries are not supported on an index view");
  GULON_REQUIRE(from <= until, "expected: from <= until");
  GULON_REQUIRE(from >= 0 && until <= ix->n, "expected: from >= 0 && until <= length");
  const int max_terms = cosmul_flat_max_terms(ix);
  GULON_UNSUPPORTED(max_terms < 1, "m = %d: the tables of one term need %d KiB of LDS, %d KiB are there", ix->m,
                    ix->m_pad, (int)(TABLE_LDS_BUDGET / 1024));
  if (b == 0) return;
  lds_terms = std::min(std::max(lds_terms, 1), max_terms);
  const int kin = std::min(k_nn + COSMUL_MAX_TERMS, GULON_MAX_K), keff = kin + 1;
  const int tab = ix->m_pad * 256;
  const size_t lds_bytes = (size_t)lds_terms * tab * sizeof(float);
  const int rb_begin = from / 64, rb_end = ceil_div(until, 64);
  const int sub = cosmul_flat_shape(ix, from, until, b).per_pass;
  for (int q0 = 0; q0 < b; q0 += sub) {
    const int nb = std::min(sub, b - q0), tcap = nb * COSMUL_MAX_TERMS;
    const int *off = d_off + q0;
    const CosmulShape shape = cosmul_flat_shape(ix, from, until, nb);
    const int rb_per_chunk = shape.per_chunk, nchunks = shape.nchunks;
    {
      std::lock_guard<std::mutex> lock(ix->mu);
      ix->pend_b = -1;
      StreamOrder so(ix, st);
      if (dev_rows) ensure_row_err(ix);
      x.plan.ensure(3); x.bad.ensure(nb);
      x.uoff.ensure((size_t)tcap + 1); x.urows.ensure(tcap); x.ones.ensure(tcap);
      x.q.ensure((size_t)tcap * ix->d);
      x.tables.ensure((size_t)tcap * tab);
      x.pv.ensure((size_t)nb * nchunks * keff); x.pi.ensure((size_t)nb * nchunks * keff);
      x.oi.ensure((size_t)nb * kin); x.od.ensure((size_t)nb * kin); x.oc.ensure(nb);
      hipLaunchKernelGGL(cosmul_plan, dim3(1), dim3(PLAN_THREADS), 0, st, off, d_rows, d_w, nb, ix->n, tcap, k_nn,
                         max_terms, x.plan.p, x.bad.p, x.uoff.p, x.urows.p, x.ones.p,
                         dev_rows ? ix->row_err.p : nullptr);
      HIP_CHECK(hipGetLastError());
      so.done();
    }
    // q_t: the handle's own compose of the one-term expressions (it takes the handle's mutex itself)
    rethrow(gulon_index_compose_rows_dev(ix, x.uoff.p, x.urows.p, x.ones.p, tcap, normalize ? 1 : 0, normalize ? 1 : 0,
                                         x.q.p, st));
    std::lock_guard<std::mutex> lock(ix->mu);
    StreamOrder so(ix, st);
    launch_build_tables(1, ix, x.q.p, tcap, tcap, x.tables.p, st, x.plan.p + 1);   // the slots in use only
#define CF(VEC)                                                                                                       \
  do {                                                                                                                \
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(cosmul_flat_scan<VEC>),                              \
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));                       \
    hipLaunchKernelGGL(cosmul_flat_scan<VEC>, dim3(nb, nchunks), dim3(TABLE_SCAN_THREADS), lds_bytes, st, ix->codes.p, ix->ng, \
                       ix->m_pad, x.tables.p, x.plan.p, x.bad.p, off, d_w, nb, lds_terms, from, until, ix->row_base,   \
                       rb_begin, rb_end, rb_per_chunk, nchunks, keff, x.pv.p, x.pi.p);                                \
  } while (0)
    if (ix->vec == 4) CF(4); else CF(16);
#undef CF
    HIP_CHECK(hipGetLastError());
    finish_lists(x, nchunks, keff, nb, kin, k_nn, off, d_rows, ix->row_base, out_idx + (size_t)q0 * k_nn,
                 out_score + (size_t)q0 * k_nn, out_count ? out_count + q0 : nullptr, st);
    so.done();
  }
}

}  // namespace gulon

using namespace gulon;

GULON_API int32_t gulon_index_query_cosmul_dev(gulon_index *idx, const int32_t *d_term_offsets,
                                               const int32_t *d_term_rows, const float *d_term_weights, int32_t b,
                                               int32_t k_nn, int32_t normalize, int32_t from, int32_t until,
                                               int32_t *d_out_idx, float *d_out_score, int32_t *d_out_count,
                                               void *stream) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    std::lock_guard<std::mutex> work(idx->cosmul.mu);
    launch_cosmul_flat(idx, idx->cosmul, d_term_offsets, d_term_rows, d_term_weights, b, k_nn, normalize != 0, from,
                       until, COSMUL_MAX_TERMS, d_out_idx, d_out_score, d_out_count, true, (hipStream_t)stream);
  });
}

GULON_API int32_t gulon_index_query_cosmul(gulon_index *idx, const int32_t *term_offsets, const int32_t *term_rows,
                                           const float *term_weights, int32_t b, int32_t k_nn, int32_t normalize,
                                           int32_t from, int32_t until, int32_t *out_idx, float *out_score,
                                           int32_t *out_count) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    GULON_REQUIRE(b >= 0, "batch size must be non-negative");
    int emax = 0;
    const int terms = check_cosmul_host(term_offsets, term_rows, term_weights, b, idx->n, k_nn, &emax);
    GULON_UNSUPPORTED(idx->wide, "cosmul queries take byte codes: k = %d > 256 is not supported", idx->k);
    GULON_UNSUPPORTED(idx->is_view, "cosmul queries are not supported on an index view");
    GULON_UNSUPPORTED(emax > cosmul_flat_max_terms(idx),
                      "m = %d, E = %d: the tables of one question need %d KiB of LDS, %d KiB are there", idx->m, emax,
                      emax * idx->m_pad, (int)(TABLE_LDS_BUDGET / 1024));
    CosmulWork &x = idx->cosmul;
    std::lock_guard<std::mutex> work(x.mu);
    const hipStream_t st = nullptr;
    const size_t bk = (size_t)b * (size_t)k_nn;
    {
      std::lock_guard<std::mutex> lock(idx->mu);
      StreamOrder so(idx, st);   // the workspace may still be read by the last call, on another stream
      if (b > 0) {
        x.off.upload(term_offsets, (size_t)b + 1, st);
        x.rows.upload(term_rows, (size_t)terms, st);
        x.w.upload(term_weights, (size_t)terms, st);
      }
      x.fi.ensure(bk + 1); x.fd.ensure(bk + 1); x.fc.ensure((size_t)b + 1);
    }
    launch_cosmul_flat(idx, x, x.off.p, x.rows.p, x.w.p, b, k_nn, normalize != 0, from, until, emax, x.fi.p, x.fd.p,
                       x.fc.p, false, st);
    if (bk) { x.fi.download(out_idx, bk, st); x.fd.download(out_score, bk, st); }
    if (b > 0 && out_count) x.fc.download(out_count, (size_t)b, st);
    HIP_CHECK(hipStreamSynchronize(st));
  });
}

#ifdef GULON_TEST_HOOKS
// Which launch geometry gulon_index_query_cosmul[_dev] takes for b questions over rows [from, until) of `idx`
// (tests/test_gpu_cosmul_paths.py): out = {questions per pass, row chunks of the first pass, 64-row code blocks per
// chunk}, by the launcher's own cosmul_flat_shape.  Host code: nothing is launched.
GULON_API int32_t gulon_selftest_cosmul_flat_shape(const gulon_index *idx, int32_t b, int32_t from, int32_t until,
                                                   int32_t out[3]) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr && out != nullptr && b >= 1, "bad arguments");
    GULON_UNSUPPORTED(idx->wide, "cosmul queries take byte codes: k = %d > 256 is not supported", idx->k);
    GULON_REQUIRE(from >= 0 && from <= until && until <= idx->n, "expected: 0 <= from <= until <= length");
    const CosmulShape s = cosmul_flat_shape(idx, from, until, b);
    out[0] = s.per_pass; out[1] = s.nchunks; out[2] = s.per_chunk;
  });
}
#endif
