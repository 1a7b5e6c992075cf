// The PQIndex handle: its creation from the reference's coder layouts (relayout_codes: [m][n] u8 -> the scan's row
// blocks [n/64][ng][64][VEC]), query contexts and the host-context pool, the tuning knobs, the profile read-outs.
#include "scan.hpp"

namespace gulon {

// ---------------------------------------------------------------------------
// code re-layout
// ---------------------------------------------------------------------------
template <int VEC>
__global__ void relayout_codes(const uint8_t *__restrict__ src /*[m][n]*/, int n, int m, int ng,
                               uint8_t *__restrict__ dst, long long total /* nblk*ng*64 */) {
  long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  int lane = (int)(t & 63);
  long long bg = t >> 6;
  int g = (int)(bg % ng);
  long long rb = bg / ng;
  long long row = rb * 64 + lane;
  uint8_t out[VEC];
#pragma unroll
  for (int b = 0; b < VEC; b++) {
    int j = g * VEC + b;
    out[b] = (row < n && j < m) ? src[(size_t)j * n + row] : (uint8_t)0;
  }
  uint8_t *o = dst + (size_t)t * VEC;
#pragma unroll
  for (int b = 0; b < VEC; b++) o[b] = out[b];
}

// unpack 2/4-bit and 10/12/16-bit Coder layouts to one index per row
// (Coder.scala:110-111,125-126,138-139,163-167)
__global__ void unpack_codes(const uint8_t *__restrict__ packed, int width, int n, int bytes_per_code,
                             int m, uint16_t *__restrict__ out /*[m][n]*/) {
  long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)m * n) return;
  int j = (int)(t / n);
  int i = (int)(t % n);
  const uint8_t *code = packed + (size_t)j * bytes_per_code;
  int lw = width > 8 ? width - 8 : width;
  int off = width > 8 ? n : 0;
  int lo;
  if (lw == 2) lo = (code[off + (i >> 2)] >> ((i & 3) * 2)) & 0x3;
  else if (lw == 4) lo = (code[off + (i >> 1)] >> ((i & 1) * 4)) & 0xF;
  else lo = code[off + i];
  int v = width > 8 ? ((code[i] << lw) | lo) : lo;
  out[t] = (uint16_t)v;
}

__global__ void narrow_codes(const uint16_t *__restrict__ in, long long total, uint8_t *__restrict__ out) {
  long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < total) out[t] = (uint8_t)in[t];
}

ScanTuning::ScanTuning() {
  static const char *keys[] = {"GULON_SCAN_BLOCKS", "GULON_SCAN_PRUNE", "GULON_SCAN_PRUNE_FROM", "GULON_SCAN_FILTER",
                               "GULON_FILTER_MIN_RB", "GULON_FILTER_PERIOD", "GULON_FILTER_STAGE1", "GULON_FILTER_CAP",
                               "GULON_FILTER_NADD", "GULON_FILTER_SAMPLE", "GULON_FILTER_STAGE0", "GULON_FILTER_BLOCKS",
                               "GULON_FILTER_SHARED_STAGE1", "GULON_FILTER_ORDER", "GULON_FILTER_SORT",
                               "GULON_FILTER_PREFIX"};
  for (const char *k : keys)
    if (const char *e = getenv(k)) set(k, atoi(e));
}

bool ScanTuning::set(const char *key, int v) {
  std::string k(key);
  if (k == "GULON_SCAN_BLOCKS") { if (v >= 1) target_blocks = v; }
  else if (k == "GULON_SCAN_PRUNE") prune = v != 0;
  else if (k == "GULON_SCAN_PRUNE_FROM") prune_from = v;
  else if (k == "GULON_SCAN_FILTER") filter = v != 0;
  else if (k == "GULON_FILTER_MIN_RB") filter_min_rb = v < 4 ? 4 : v;
  else if (k == "GULON_FILTER_PERIOD") { if (v >= 3) filter_period = v; }
  else if (k == "GULON_FILTER_STAGE1") { if (v >= 1) filter_stage1 = v; }
  else if (k == "GULON_FILTER_CAP") { if (v >= 64) filter_cap = v; }
  else if (k == "GULON_FILTER_NADD") { if (v == 0 || v == 2 || v == 4) filter_nadd = v; }
  else if (k == "GULON_FILTER_SAMPLE") { if (v >= 1) filter_sample = v; }
  else if (k == "GULON_FILTER_STAGE0") { if (v >= 0) filter_stage0 = v; }
  else if (k == "GULON_FILTER_BLOCKS") { if (v >= 1) filter_blocks = v; }
  else if (k == "GULON_FILTER_SHARED_STAGE1") { if (v >= -1 && v <= 1) filter_shared_stage1 = v; }
  else if (k == "GULON_FILTER_ORDER") { if (v >= 0 && v <= 8) filter_order = v; }
  else if (k == "GULON_FILTER_SORT") filter_sort = v != 0;
  else if (k == "GULON_FILTER_PREFIX") { if (v == 0 || v == FILTER_PREFIX_P) filter_prefix = v; }
  else return false;
  return true;
}

// The knobs have no process-wide mutable state: a handle takes its settings from the ENVIRONMENT when it is created
// (ScanTuning's constructor) and keeps them; gulon_index_tuning changes one handle.  (A null handle: the compiled-in defaults.)
const ScanTuning &tuning_defaults() { static const ScanTuning t; return t; }

}  // namespace gulon

using namespace gulon;

static constexpr size_t LDS_BUDGET = 144 * 1024;

GULON_API int32_t gulon_index_create(const uint8_t *codes, int32_t n, int32_t d, int32_t m, int32_t k,
                                     const float *cents, int32_t row_base, gulon_index **out) {
  return guarded([&] {
    GULON_REQUIRE(out != nullptr, "out is null");
    *out = nullptr;
    GULON_REQUIRE(n >= 0 && d >= 1 && m >= 1 && m <= d && k >= 1, "bad index shape n=%d d=%d m=%d k=%d", n, d, m, k);
    GULON_REQUIRE(cents != nullptr && (codes != nullptr || n == 0), "null input");
    int width = -1;
    GULON_REQUIRE(gulon_coder_width(k, &width) == GULON_OK && width >= 0, "too many clusters: %d", k);  // PQ.scala:12-15
    std::unique_ptr<gulon_index> ix(new gulon_index());
    ix->tune = std::make_shared<ScanTuning>();   // the environment as it is now
    ix->n = n; ix->d = d; ix->m = m; ix->k = k; ix->row_base = row_base;
    if (k > 256) {
      // Coder.BytePlus widths 10/12/16 (Coder.scala:99-127): 16-bit codes, tables in HBM (wide.hip)
      ix->wide = true;
      std::vector<int> from, until, sdim(m);
      subvectors(d, m, from, until);
      for (int j = 0; j < m; j++) sdim[j] = until[j] - from[j];
      ix->from.upload(from.data(), m);
      ix->sdim.upload(sdim.data(), m);
      ix->cents.upload(cents, (size_t)k * d);
      int bytes_per_code = 0;
      gulon_coder_bytes(width, n, &bytes_per_code);
      DevBuf<uint16_t> wide16(std::max<size_t>((size_t)m * n, 1));
      if (n > 0) {
        DevBuf<uint8_t> packed;
        packed.upload(codes, (size_t)m * bytes_per_code);
        const long long tot = (long long)m * n;
        hipLaunchKernelGGL(unpack_codes, dim3(ceil_div(tot, 256)), dim3(256), 0, 0, packed.p, width, n, bytes_per_code, m,
                           wide16.p);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
      }
      wide_store_codes(ix.get(), wide16.p);
      ensure_row_err(ix.get());
      *out = ix.release();
      return;
    }
    ix->vec = (m % 16 == 0) ? 16 : 4;
    ix->ng = ceil_div(m, ix->vec);
    ix->m_pad = ix->ng * ix->vec;
    // queries interleaved per table entry: as many as LDS holds (m = 64 -> 2, m > 72 -> 1)
    ix->w = 4;
    while (ix->w > 1 && (size_t)ix->m_pad * 256 * ix->w * 4 > LDS_BUDGET) ix->w /= 2;
    size_t per_sub = (size_t)ix->m_pad * 256 * ix->w * 4;
    GULON_UNSUPPORTED(per_sub > LDS_BUDGET, "m = %d quantizers need %zu B of LDS for one query's table (> %zu)", m,
                      per_sub, LDS_BUDGET);
    ix->nsub = ix->w < 4 ? 1 : (4 * per_sub <= LDS_BUDGET) ? 4 : (2 * per_sub <= LDS_BUDGET) ? 2 : 1;

    std::vector<int> from, until, sdim(m);
    subvectors(d, m, from, until);
    for (int j = 0; j < m; j++) sdim[j] = until[j] - from[j];
    ix->from.upload(from.data(), m);
    ix->sdim.upload(sdim.data(), m);
    ix->cents.upload(cents, (size_t)k * d);
    ix->cents_absmax = centroid_absmax(ix->cents.p, (long long)k * d);

    int bytes_per_code = 0;
    gulon_coder_bytes(width, n, &bytes_per_code);
    size_t nblk = (size_t)ceil_div(n, 64);
    ix->codes.alloc(std::max<size_t>(nblk * ix->ng * 64 * ix->vec, 16));
    if (n > 0) {
      DevBuf<uint8_t> raw;  // [m][n] one byte per (quantizer,row)
      if (width == 8) {
        raw.upload(codes, (size_t)m * n);
      } else {
        raw.alloc((size_t)m * n);
        if (width == 0) {
          HIP_CHECK(hipMemset(raw.p, 0, (size_t)m * n));
        } else {
          DevBuf<uint8_t> packed;
          packed.upload(codes, (size_t)m * bytes_per_code);
          DevBuf<uint16_t> wide((size_t)m * n);
          long long tot = (long long)m * n;
          hipLaunchKernelGGL(unpack_codes, dim3(ceil_div(tot, 256)), dim3(256), 0, 0, packed.p, width, n,
                             bytes_per_code, m, wide.p);
          hipLaunchKernelGGL(narrow_codes, dim3(ceil_div(tot, 256)), dim3(256), 0, 0, wide.p, tot, raw.p);
          HIP_CHECK(hipGetLastError());
          HIP_CHECK(hipDeviceSynchronize());
        }
      }
      long long total = (long long)nblk * ix->ng * 64;
      if (ix->vec == 16)
        hipLaunchKernelGGL(relayout_codes<16>, dim3(ceil_div(total, 256)), dim3(256), 0, 0, raw.p, n, m, ix->ng,
                           ix->codes.p, total);
      else
        hipLaunchKernelGGL(relayout_codes<4>, dim3(ceil_div(total, 256)), dim3(256), 0, 0, raw.p, n, m, ix->ng,
                           ix->codes.p, total);
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipDeviceSynchronize());
      build_filter_copy(ix.get());
    }
    HIP_CHECK(hipDeviceSynchronize());
    ensure_row_err(ix.get());
    *out = ix.release();
  });
}

namespace gulon {
// the filter's conflict-ordered copy (one 16-byte code word per row; ranges the filter is never used for
// do not need one).  GULON_FILTER_ORDER = rounds of the ordering (0: no copy)
void build_filter_copy(gulon_index *ix) {
  const size_t nblk = (size_t)ceil_div(ix->n, 64);
  const int rounds = ix->tune->filter_order;
  if (rounds > 0 && ix->vec == 16 && ix->ng == 1 && (long long)nblk >= ix->tune->filter_min_rb) {
    ix->fcodes.alloc(nblk * 1024);
    ix->fperm.alloc(nblk * 64);
    launch_conflict_order(ix->codes.p, ix->fcodes.p, ix->fperm.p, (long long)nblk, FILTER_LDS_QUANTIZERS, rounds, 0);
    ix->fwindow = conflict_order_windowed() ? 4 : 1;
    HIP_CHECK(hipDeviceSynchronize());
  }
  // the key-sorted copy (GULON_FILTER_SORT): 16 bytes of codes + a 32-bit row id per row
  if (ix->tune->filter_sort > 0 && ix->vec == 16 && ix->ng == 1 && (long long)nblk >= ix->tune->filter_min_rb) {
    const size_t nwin = (size_t)ceil_div(ix->n, 256);
    ix->scodes.alloc(nwin * 4096);
    ix->sids.alloc(nwin * 256);
    launch_sorted_copy(ix->codes.p, ix->n, ix->scodes.p, ix->sids.p, std::max(1, rounds), 0);
    HIP_CHECK(hipDeviceSynchronize());
  }
}

gulon_index *make_context(gulon_index *parent) {
  std::unique_ptr<gulon_index> c(new gulon_index());
  c->n = parent->n; c->d = parent->d; c->m = parent->m; c->k = parent->k; c->row_base = parent->row_base;
  c->vec = parent->vec; c->ng = parent->ng; c->m_pad = parent->m_pad; c->nsub = parent->nsub; c->w = parent->w;
  c->wide = parent->wide;
  c->cents_absmax = parent->cents_absmax;
  c->tune = parent->tune;
  c->codes.borrow(parent->codes);
  c->fcodes.borrow(parent->fcodes);
  c->fperm.borrow(parent->fperm);
  c->fwindow = parent->fwindow;
  c->scodes.borrow(parent->scodes);
  c->sids.borrow(parent->sids);
  c->wcodes.borrow(parent->wcodes);
  c->cents.borrow(parent->cents);
  c->from.borrow(parent->from);
  c->sdim.borrow(parent->sdim);
  c->is_view = parent->is_view;
  c->view_base = parent->view_base;
  c->vmap.borrow(parent->vmap);
  ensure_row_err(c.get());
  return c.release();
}
}  // namespace gulon

namespace {
void release_index(gulon_index *ix) {
  if (!ix) return;
  if (ix->refs.fetch_sub(1) != 1) return;       // contexts of this index are still alive
  gulon_index *parent = ix->parent;
  delete ix;
  release_index(parent);
}

int host_context_limit() {
  static const int lim = [] { const char *e = getenv("GULON_HOST_CONTEXTS"); int v = e ? atoi(e) : 4; return v < 1 ? 1 : v > 64 ? 64 : v; }();
  return lim;
}
}  // namespace

namespace gulon {
gulon_index *acquire_host_context(gulon_index *idx) {
  std::unique_lock<std::mutex> lk(idx->host_mu);
  for (;;) {
    if (!idx->host_self_busy) { idx->host_self_busy = true; return idx; }
    if (!idx->host_free.empty()) { gulon_index *c = idx->host_free.back(); idx->host_free.pop_back(); return c; }
    if ((int)idx->host_all.size() + 1 < host_context_limit()) {
      gulon_index *c = make_context(idx);
      idx->host_all.push_back(c);
      return c;
    }
    idx->host_cv.wait(lk);
  }
}
void release_host_context(gulon_index *idx, gulon_index *c) {
  {
    std::lock_guard<std::mutex> lk(idx->host_mu);
    if (c == idx) idx->host_self_busy = false; else idx->host_free.push_back(c);
  }
  idx->host_cv.notify_one();
}
}  // namespace gulon

GULON_API int32_t gulon_index_destroy(gulon_index *idx) {
  return guarded([&] { release_index(idx); });
}

GULON_API int32_t gulon_index_context_create(gulon_index *parent, gulon_index **out) {
  return guarded([&] {
    GULON_REQUIRE(parent != nullptr && out != nullptr, "null argument");
    *out = nullptr;
    gulon_index *root = parent->parent ? parent->parent : parent;   // contexts of contexts hang off the owner
    gulon_index *c = make_context(root);
    c->parent = root;
    root->refs.fetch_add(1);
    *out = c;
  });
}

GULON_API int32_t gulon_index_profile(gulon_index *idx, int32_t enable) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    std::lock_guard<std::mutex> lock(idx->mu);
    idx->events.clear();
    idx->ev_next = 0;
    idx->prof_rows = 0;
    idx->profile = enable != 0;
    if (idx->profile)
      while (idx->ev_pool.size() < 512) {
        hipEvent_t e = nullptr;
        HIP_CHECK(hipEventCreate(&e));
        idx->ev_pool.push_back(e);
      }
  });
}

GULON_API int32_t gulon_index_profile_read(gulon_index *idx, double *scan_ms_total, int32_t *launches) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    std::lock_guard<std::mutex> lock(idx->mu);
    double tot = 0;
    for (auto &e : idx->events) {
      HIP_CHECK(hipEventSynchronize(e.second));
      float ms = 0;
      HIP_CHECK(hipEventElapsedTime(&ms, e.first, e.second));
      tot += ms;
    }
    if (scan_ms_total) *scan_ms_total = tot;
    if (launches) *launches = (int32_t)idx->events.size();
  });
}

GULON_API int32_t gulon_index_profile_read_ex(gulon_index *idx, double *ms_total, int32_t *launches,
                                              int64_t *rows_total) {
  int32_t rc = gulon_index_profile_read(idx, ms_total, launches);
  if (rc == GULON_OK && rows_total) *rows_total = idx->prof_rows;
  return rc;
}

GULON_API int32_t gulon_index_filter_stats(gulon_index *idx, int32_t *query_tiles, int32_t *tiles_redone) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    std::lock_guard<std::mutex> lock(idx->mu);
    HIP_CHECK(hipDeviceSynchronize());
    const int nt = idx->last_filter_tiles;
    int redone = 0;
    if (nt > 0) {
      std::vector<int> h((size_t)nt);
      HIP_CHECK(hipMemcpy(h.data(), idx->fb_tile.p, sizeof(int) * h.size(), hipMemcpyDeviceToHost));
      for (int v : h) redone += v != 0;
    }
    if (query_tiles) *query_tiles = nt;
    if (tiles_redone) *tiles_redone = redone;
  });
}

GULON_API int32_t gulon_index_tuning(gulon_index *idx, const char *key, int32_t value) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr && key != nullptr, "null argument");
    std::lock_guard<std::mutex> lock(idx->mu);
    // copy-on-write: contexts created earlier keep the settings they were created with
    auto t = std::make_shared<ScanTuning>(tuning_of(idx));
    GULON_REQUIRE(t->set(key, value), "unknown tuning key");
    idx->tune = t;
  });
}
