// word2vec text -> a device-resident matrix: WordVectors.readWord2Vec (WordVectors.scala:141-252) with the per-token
// work on the device.  The host cuts the text into chunks at line ends and copies them over; per chunk
//   line_count / line_offsets / line_starts  lane = 16 bytes: a line starts after a \n (or at the chunk's start) where
//                                            the byte is not itself a \n -- an empty line takes no row; a prefix sum
//                                            over the workgroups' counts numbers the rows in file order
//   field_scan                               one wavefront per line: the positions of its first d + 1 blanks (fields
//                                            are separated by single blanks; what follows field d is not read), the
//                                            word's extent, and the first line with fewer than d components
//   convert                                  lane = token: ingest_parse.h decides the token's binary32 exactly or
//                                            appends it to the flagged list (the host converts those and hands them
//                                            back to gulon_ingest_finish)
// then, once, patch (the host's values), normalize_rows (MathUtils.normalize, shared with decode.hip) and the hand-over
// of the matrix to a gulon_dataset.  The only round trips per chunk are the row count and the flagged count.
// The chunk buffer is padded with \n up to a whole tile and one more: no kernel tests for the end of the text, and a
// last line without \n ends like any other.
#include "common.hpp"
#include "ingest_parse.h"
#include "normalize.hpp"

namespace gulon {
namespace {

constexpr int LS_THREADS = 256;
constexpr int LS_TILE = LS_THREADS * 16;       // bytes of text per workgroup of the line scan
constexpr int MAX_CHUNK = 1 << 29;             // chunk offsets are ints
constexpr size_t DEFAULT_CHUNK = 64u << 20;
constexpr unsigned FLAG_CAP = 1u << 16;        // flagged tokens kept per chunk before the list is regrown

// bit j: a non-empty line starts at byte base + j (base a multiple of 16)
__device__ __forceinline__ unsigned line_start_mask(const uint8_t *__restrict__ txt, int base) {
  const uint4 v = *(const uint4 *)(txt + base);
  const unsigned w[4] = {v.x, v.y, v.z, v.w};
  unsigned prev = base ? txt[base - 1] : (unsigned)'\n';
  unsigned mask = 0;
#pragma unroll
  for (int j = 0; j < 16; j++) {
    const unsigned c = (w[j >> 2] >> ((j & 3) * 8)) & 0xFFu;
    if (prev == '\n' && c != '\n') mask |= 1u << j;
    prev = c;
  }
  return mask;
}

// exclusive prefix sum of v over the workgroup's LS_THREADS lanes; *total: the sum
__device__ __forceinline__ int block_exclusive_scan(int v, int *total) {
  __shared__ int wsum[LS_THREADS / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o);
    if (lane >= o) inc += t;
  }
  if (lane == 63) wsum[wv] = inc;
  __syncthreads();
  int base = 0, all = 0;
#pragma unroll
  for (int w = 0; w < LS_THREADS / 64; w++) {
    if (w < wv) base += wsum[w];
    all += wsum[w];
  }
  *total = all;
  return base + inc - v;
}

__global__ __launch_bounds__(LS_THREADS) void ingest_line_count(const uint8_t *__restrict__ txt,
                                                                int *__restrict__ counts) {
  int total;
  block_exclusive_scan(__popc(line_start_mask(txt, blockIdx.x * LS_TILE + threadIdx.x * 16)), &total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// exclusive prefix sum of counts[0, nb) (one workgroup); *rows: the total
__global__ __launch_bounds__(1024) void ingest_line_offsets(const int *__restrict__ counts, int nb,
                                                            int *__restrict__ offsets, int *__restrict__ rows) {
  __shared__ int part[1024];
  const int seg = (nb + 1023) / 1024, lo = min(threadIdx.x * seg, nb), hi = min(lo + seg, nb);
  int s = 0;
  for (int i = lo; i < hi; i++) s += counts[i];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int i = 0; i < 1024; i++) { const int t = part[i]; part[i] = run; run += t; }
    *rows = run;
  }
  __syncthreads();
  int run = part[threadIdx.x];
  for (int i = lo; i < hi; i++) { offsets[i] = run; run += counts[i]; }
}

__global__ __launch_bounds__(LS_THREADS) void ingest_line_starts(const uint8_t *__restrict__ txt,
                                                                 const int *__restrict__ offsets, int rows,
                                                                 int *__restrict__ line_start) {
  const int base = blockIdx.x * LS_TILE + threadIdx.x * 16;
  unsigned mask = line_start_mask(txt, base);
  int total;
  int r = offsets[blockIdx.x] + block_exclusive_scan(__popc(mask), &total);
  while (mask) {
    const int j = __ffs(mask) - 1;
    mask &= mask - 1;
    if (r < rows) line_start[r] = base + j;
    r++;
  }
}

// sp[r][s], s = 0 .. d: the position of line r's s-th blank, or of the line's end where it has fewer: token f
// (1 .. d) is [sp[r][f - 1] + 1, sp[r][f]).  One wavefront per line, 64 bytes per step, no LDS.
__global__ __launch_bounds__(256) void ingest_field_scan(const uint8_t *__restrict__ txt,
                                                         const int *__restrict__ line_start, int rows, int d,
                                                         long long chunk_base, long long row_base,
                                                         int *__restrict__ sp, long long *__restrict__ word_begin,
                                                         int *__restrict__ word_len,
                                                         unsigned long long *__restrict__ first_short) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= rows) return;                                   // wave-uniform
  const int s0 = line_start[r];
  int *row_sp = sp + (size_t)r * (d + 1);
  int nsp = 0, first_sp = -1, end = -1;
  for (int pos = s0; nsp <= d; pos += 64) {
    const unsigned c = txt[pos + lane];
    const unsigned long long nl = __ballot(c == '\n');
    const unsigned long long before = nl ? (nl & (0ull - nl)) - 1 : ~0ull;   // the lanes in front of the first \n
    const unsigned long long blanks = __ballot(c == ' ') & before;
    if ((blanks >> lane) & 1) {
      const int s = nsp + __popcll(blanks & ((1ull << lane) - 1));
      if (s <= d) row_sp[s] = pos + lane;
    }
    if (first_sp < 0 && blanks) first_sp = pos + __ffsll((long long)blanks) - 1;
    nsp += __popcll(blanks);
    if (nl) { end = pos + __ffsll((long long)nl) - 1; break; }
  }
  // fewer than d + 1 blanks: the loop ran to the line's end
  for (int s = nsp + lane; s <= d; s += 64) row_sp[s] = end;
  if (lane == 0) {
    word_begin[r] = chunk_base + s0;
    word_len[r] = (first_sp >= 0 ? first_sp : end) - s0;
    if (nsp < d) atomicMin(first_short, (unsigned long long)(row_base + r));
  }
}

struct FlagList {
  unsigned *count;
  unsigned cap;
  long long *row, *begin;
  int *field, *len;
};

__global__ __launch_bounds__(256) void ingest_convert(const uint8_t *__restrict__ txt, const int *__restrict__ sp,
                                                      int rows, int d, long long chunk_base, long long row_base,
                                                      float *__restrict__ x, FlagList fl) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)rows * d) return;
  const int r = (int)(t / d), f = (int)(t - (long long)r * d);
  const int *row_sp = sp + (size_t)r * (d + 1);
  const int b = row_sp[f] + 1, e = row_sp[f + 1];
  uint32_t bits = 0;
  // e < b: a component the line does not have (the host raises for that line); otherwise decide or flag
  if (e >= b && !gulon_parse_f32(txt + b, e - b, &bits)) {
    const unsigned slot = atomicAdd(fl.count, 1u);
    if (slot < fl.cap) {
      fl.row[slot] = row_base + r;
      fl.field[slot] = f;
      fl.begin[slot] = chunk_base + b;
      fl.len[slot] = e - b;
    }
  }
  x[(size_t)(row_base + r) * d + f] = __uint_as_float(bits);
}

__global__ void ingest_patch(float *__restrict__ x, const long long *__restrict__ at, const float *__restrict__ value,
                             long long n) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) x[at[t]] = value[t];
}

// MathUtils.normalize of every row, in place: one wavefront per row, the row staged in LDS
__global__ __launch_bounds__(64) void normalize_rows_kernel(float *__restrict__ x, int d) {
  extern __shared__ float xs[];   // [d]
  float *row = x + (size_t)blockIdx.x * d;
  for (int e = threadIdx.x; e < d; e += 64) xs[e] = row[e];
  __syncthreads();
  normalize_staged_row(xs, d, threadIdx.x, 64, row);
}

template <class T>
void grow(DevBuf<T> &buf, size_t keep, size_t want) {
  if (want <= buf.n) return;
  DevBuf<T> next(want);
  if (keep) HIP_CHECK(hipMemcpy(next.p, buf.p, keep * sizeof(T), hipMemcpyDeviceToDevice));
  buf = std::move(next);
}

}  // namespace
}  // namespace gulon

struct gulon_ingest {
  int32_t d = 0;
  int64_t rows = 0, flagged = 0, first_short = -1;
  gulon::DevBuf<float> x;                     // [rows][d], capacity x.n / d rows
  std::vector<int64_t> word_begin, flag_row, flag_begin;
  std::vector<int32_t> word_len, flag_field, flag_len;
};

using namespace gulon;

namespace {

struct FlagBufs {
  DevBuf<unsigned> count;
  DevBuf<long long> row, begin;
  DevBuf<int> field, len;
  void ensure(size_t cap) { row.ensure(cap); begin.ensure(cap); field.ensure(cap); len.ensure(cap); }
  FlagList list() const { return FlagList{count.p, (unsigned)row.n, row.p, begin.p, field.p, len.p}; }
};

void ingest_run(gulon_ingest *in, const uint8_t *text, uint64_t len, uint64_t offset, size_t chunk_bytes) {
  const int d = in->d;
  DevBuf<uint8_t> txt;
  DevBuf<int> counts, offsets, nrows(1), line_start, sp, wlen;
  DevBuf<long long> wbegin;
  DevBuf<unsigned long long> first_short(1);
  FlagBufs fb;
  fb.count.alloc(1);
  fb.ensure(FLAG_CAP);
  HIP_CHECK(hipMemset(first_short.p, 0xFF, sizeof(unsigned long long)));
  uint64_t pos = offset;
  while (pos < len) {
    // [pos, end): whole lines, chunk_bytes at the most unless one line is longer
    uint64_t end = std::min<uint64_t>(len, pos + chunk_bytes);
    if (end < len) {
      const void *nl = memrchr(text + pos, '\n', (size_t)(end - pos));
      if (!nl) nl = memchr(text + end, '\n', (size_t)(len - end));
      end = nl ? (uint64_t)((const uint8_t *)nl - text) + 1 : len;
    }
    GULON_UNSUPPORTED(end - pos > (uint64_t)MAX_CHUNK, "a line of more than %d bytes", MAX_CHUNK);
    const int m = (int)(end - pos);
    const int nb = ceil_div(m, LS_TILE);
    const size_t padded = (size_t)(nb + 1) * LS_TILE;
    txt.ensure(padded);
    HIP_CHECK(hipMemcpyAsync(txt.p, text + pos, (size_t)m, hipMemcpyHostToDevice, nullptr));
    HIP_CHECK(hipMemsetAsync(txt.p + m, '\n', padded - (size_t)m, nullptr));
    counts.ensure((size_t)nb);
    offsets.ensure((size_t)nb);
    hipLaunchKernelGGL(ingest_line_count, dim3(nb), dim3(LS_THREADS), 0, nullptr, txt.p, counts.p);
    hipLaunchKernelGGL(ingest_line_offsets, dim3(1), dim3(1024), 0, nullptr, counts.p, nb, offsets.p, nrows.p);
    HIP_CHECK(hipGetLastError());
    int rows = 0;
    HIP_CHECK(hipMemcpy(&rows, nrows.p, sizeof(int), hipMemcpyDeviceToHost));
    const int64_t total = in->rows + rows;
    GULON_UNSUPPORTED(total > INT32_MAX, "more than %d rows", INT32_MAX);
    if (rows) {
      // the matrix grows with the text: exactly at the last chunk, else by the density of the rows met so far
      size_t want = (size_t)total;
      if (end < len && want > in->x.n / d)
        want = (size_t)((double)total * (double)(len - offset) / (double)(end - offset) * 1.02) + 1024;
      grow(in->x, (size_t)in->rows * d, want * d);
      line_start.ensure((size_t)rows);
      sp.ensure((size_t)rows * (d + 1));
      wbegin.ensure((size_t)rows);
      wlen.ensure((size_t)rows);
      hipLaunchKernelGGL(ingest_line_starts, dim3(nb), dim3(LS_THREADS), 0, nullptr, txt.p, offsets.p, rows,
                         line_start.p);
      hipLaunchKernelGGL(ingest_field_scan, dim3(ceil_div(rows, 4)), dim3(256), 0, nullptr, txt.p, line_start.p, rows, d,
                         (long long)pos, (long long)in->rows, sp.p, wbegin.p, wlen.p, first_short.p);
      HIP_CHECK(hipGetLastError());
      unsigned nflag = 0;
      for (int pass = 0; pass < 2; pass++) {
        HIP_CHECK(hipMemsetAsync(fb.count.p, 0, sizeof(unsigned), nullptr));
        hipLaunchKernelGGL(ingest_convert, dim3(ceil_div((long long)rows * d, 256)), dim3(256), 0, nullptr, txt.p, sp.p,
                           rows, d, (long long)pos, (long long)in->rows, in->x.p, fb.list());
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(&nflag, fb.count.p, sizeof(unsigned), hipMemcpyDeviceToHost));
        if (nflag <= fb.row.n) break;
        fb.ensure(nflag);                       // more flagged tokens than the list holds: once more, with room
      }
      const size_t w0 = in->word_begin.size(), f0 = in->flag_row.size();
      in->word_begin.resize(w0 + rows);
      in->word_len.resize(w0 + rows);
      wbegin.download((long long *)in->word_begin.data() + w0, (size_t)rows);
      wlen.download(in->word_len.data() + w0, (size_t)rows);
      in->flag_row.resize(f0 + nflag); in->flag_begin.resize(f0 + nflag);
      in->flag_field.resize(f0 + nflag); in->flag_len.resize(f0 + nflag);
      fb.row.download((long long *)in->flag_row.data() + f0, nflag);
      fb.begin.download((long long *)in->flag_begin.data() + f0, nflag);
      fb.field.download(in->flag_field.data() + f0, nflag);
      fb.len.download(in->flag_len.data() + f0, nflag);
      HIP_CHECK(hipStreamSynchronize(nullptr));
      in->rows = total;
      in->flagged += nflag;
    }
    pos = end;
  }
  unsigned long long fs = 0;
  HIP_CHECK(hipMemcpy(&fs, first_short.p, sizeof fs, hipMemcpyDeviceToHost));
  in->first_short = fs == ~0ull ? -1 : (int64_t)fs;
  if (in->x.n == 0) in->x.alloc(1);
}

}  // namespace

GULON_API int32_t gulon_ingest_word2vec(const uint8_t *text, uint64_t len, uint64_t data_offset, int32_t d,
                                        uint64_t chunk_bytes, gulon_ingest **out) {
  return guarded([&] {
    GULON_REQUIRE(out != nullptr, "out is null");
    *out = nullptr;
    GULON_REQUIRE((text != nullptr || len == 0) && data_offset <= len && d >= 1, "bad ingest arguments (d=%d)", d);
    GULON_UNSUPPORTED((size_t)d * sizeof(float) > 64 * 1024, "d = %d: a row does not fit in LDS", d);
    std::unique_ptr<gulon_ingest> in(new gulon_ingest());
    in->d = d;
    const size_t chunk = chunk_bytes ? (size_t)std::min<uint64_t>(chunk_bytes, (uint64_t)MAX_CHUNK) : DEFAULT_CHUNK;
    ingest_run(in.get(), text, len, data_offset, chunk);
    *out = in.release();
  });
}

GULON_API int32_t gulon_ingest_counts(const gulon_ingest *in, int64_t *rows, int64_t *flagged,
                                      int64_t *first_short_row) {
  return guarded([&] {
    GULON_REQUIRE(in != nullptr, "ingest is null");
    if (rows) *rows = in->rows;
    if (flagged) *flagged = in->flagged;
    if (first_short_row) *first_short_row = in->first_short;
  });
}

GULON_API int32_t gulon_ingest_words(const gulon_ingest *in, int64_t *begin, int32_t *length) {
  return guarded([&] {
    GULON_REQUIRE(in != nullptr && (in->rows == 0 || (begin != nullptr && length != nullptr)), "null argument");
    std::copy(in->word_begin.begin(), in->word_begin.end(), begin);
    std::copy(in->word_len.begin(), in->word_len.end(), length);
  });
}

GULON_API int32_t gulon_ingest_flagged(const gulon_ingest *in, int64_t *row, int32_t *field, int64_t *begin,
                                       int32_t *length) {
  return guarded([&] {
    GULON_REQUIRE(in != nullptr && (in->flagged == 0 || (row && field && begin && length)), "null argument");
    std::copy(in->flag_row.begin(), in->flag_row.end(), row);
    std::copy(in->flag_field.begin(), in->flag_field.end(), field);
    std::copy(in->flag_begin.begin(), in->flag_begin.end(), begin);
    std::copy(in->flag_len.begin(), in->flag_len.end(), length);
  });
}

GULON_API int32_t gulon_ingest_finish(gulon_ingest *in, const int64_t *patch_row, const int32_t *patch_field,
                                      const float *patch_value, int64_t n_patch, int32_t normalize,
                                      gulon_dataset **out) {
  return guarded([&] {
    GULON_REQUIRE(in != nullptr && out != nullptr, "null argument");
    *out = nullptr;
    GULON_REQUIRE(in->x.p != nullptr, "the ingest's matrix has been handed over already");
    GULON_REQUIRE(n_patch >= 0 && (n_patch == 0 || (patch_row && patch_field && patch_value)), "bad patch arguments");
    if (n_patch) {
      std::vector<long long> at((size_t)n_patch);
      for (int64_t i = 0; i < n_patch; i++) {
        GULON_REQUIRE(patch_row[i] >= 0 && patch_row[i] < in->rows && patch_field[i] >= 0 && patch_field[i] < in->d,
                      "patch %lld outside the matrix", (long long)i);
        at[(size_t)i] = (long long)patch_row[i] * in->d + patch_field[i];
      }
      DevBuf<long long> d_at;
      DevBuf<float> d_value;
      d_at.upload(at.data(), at.size());
      d_value.upload(patch_value, (size_t)n_patch);
      hipLaunchKernelGGL(ingest_patch, dim3(ceil_div(n_patch, 256)), dim3(256), 0, nullptr, in->x.p, d_at.p, d_value.p,
                         (long long)n_patch);
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipStreamSynchronize(nullptr));
    }
    if (normalize && in->rows) {
      hipLaunchKernelGGL(normalize_rows_kernel, dim3((unsigned)in->rows), dim3(64), (size_t)in->d * sizeof(float),
                         nullptr, in->x.p, in->d);
      HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipStreamSynchronize(nullptr));
    std::unique_ptr<gulon_dataset> ds(new gulon_dataset());
    ds->n = (int32_t)in->rows; ds->d = in->d;
    ds->x = std::move(in->x);
    *out = ds.release();
  });
}

GULON_API int32_t gulon_ingest_destroy(gulon_ingest *in) {
  return guarded([&] { delete in; });
}
