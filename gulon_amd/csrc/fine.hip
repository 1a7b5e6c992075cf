// Fine codes (DESIGN.md "Fine codes"): a second quantizer over the residuals an index leaves, and the index's candidates
// re-ranked against the two-level reconstruction instead of the original vectors.
//   residuals   E[t][e] = V[vector_rows[t]][e] - y_{rows[t]}[e]   (MathUtils.subtract, MathUtils.scala:74-83: one
//               binary32 subtraction per coordinate)                                              -- row_residuals_kernel
//   re-ranking  per query: heap = TopKHeap(k); for every candidate row r in list order:
//                 z_r[e] = y_r[e] + decode_F(fmap[r])[e]           (MathUtils.add, MathUtils.scala:63-71)
//                 heap.update(r, MathUtils.distanceSq(q, z_r))     (MathUtils.scala:85-95: the query subtracted from the
//                                                                   row, e ascending, unfused; TopKHeap.scala:69-79)
//               Result.fromHeap(heap) (Index.scala:83-94)                                         -- refine_codes_kernel
// y_r is the vector the coarse index's distances are about, as in inspect.hip: ProductQuantizer.decode of row r for a
// flat index; centroid(g) + decode(r) -- the centroid first, one binary32 add per coordinate -- for a grouped one, g the
// group whose row range holds r (not the binarySearch rule of GroupedIndex.lookup).  The fine coordinate is added last.
// Codes are read in the layout each handle keeps (row_decode.hpp); the coarse and the fine index share d and nothing
// else.  Both calls use scratch of their own: a handle keeps no trace of them.
#include "refine_replay.hpp"
#include "row_decode.hpp"
#include "row_tile.hpp"

namespace gulon {
namespace {

// One stored row's codes, walked j ascending by one lane: the code word that holds quantizer j is fetched when the
// walk enters it (16 or 4 bytes of the byte layouts, one 16-bit code of the wide one) and kept in registers.  j is
// wave-uniform, so the fetches are too.  A code at or above k (no code of this code book) reads as k - 1, as inspect.hip
// reads it: nothing outside the code book is touched.
struct RowCodes {
  CodeSrc src;
  size_t blk;      // row >> 6
  int sub, k;      // row & 63
  int gi = -1;
  uint4 w = {0u, 0u, 0u, 0u};
  __device__ RowCodes(const CodeSrc &s, int row, int k_) : src(s), blk((size_t)(row >> 6)), sub(row & 63), k(k_) {}
  __device__ int code(int j) {
    int c;
    if (src.wcodes) {
      c = src.wcodes[(blk * src.m + j) * 64 + sub];
    } else if (src.vec == 16) {
      const int g = j >> 4;
      if (g != gi) { w = reinterpret_cast<const uint4 *>(src.codes)[(blk * src.ng + g) * 64 + sub]; gi = g; }
      c = (int)code_byte<16>(w, j & 15);
    } else {
      const int g = j >> 2;
      if (g != gi) { w.x = reinterpret_cast<const uint32_t *>(src.codes)[(blk * src.ng + g) * 64 + sub]; gi = g; }
      c = (int)code_byte<4>(w.x, j & 3);
    }
    return min(c, k - 1);
  }
};

// One decoded row, walked e ascending: value(e) = the row's code-book coordinate e.  The entry of the quantizer that
// holds e is looked up when the walk enters it; quantizers without coordinates (d < m) are passed over.
struct RowWalk {
  RowCodes codes;
  SubvectorMap sv;
  const float *cents, *cj = nullptr;
  int m, j = -1, jfrom = 0, jend = 0;
  __device__ RowWalk(const CodeSrc &s, const float *cents_, int d, int k, int row)
      : codes(s, row, k), sv(d, s.m), cents(cents_), m(s.m) {}
  __device__ float value(int e) {
    while (e >= jend && j + 1 < m) {             // (wave-uniform)
      j++;
      jfrom = jend;
      jend += sv.sdim(j);
      cj = cents + (size_t)codes.k * jfrom + (size_t)codes.code(j) * sv.sdim(j);
    }
    return cj[e - jfrom];
  }
};

// the centroid of the group whose row range [bounds[g], bounds[g + 1]) holds `row` (inspect.hip's rule)
__device__ inline const float *group_centroid(const float *gcent, const int *bounds, int g, int row, int d) {
  int lo = 0, hi = g;
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (bounds[mid] <= row) lo = mid; else hi = mid; }
  return gcent + (size_t)lo * d;
}

struct GroupBase { const float *gcent; const int *bounds; int g; };
GroupBase group_base(const GroupedParts &gp) { return {gp.gcent, gp.bounds, gp.g}; }

// ---- residuals -----------------------------------------------------------------------------------------------------
// One wavefront per tile of 64 list positions, lane = position: lane t decodes row rows[t] of the index while the 64
// originals V[vector_rows[t]] pass through an LDS tile FR_DT coordinates at a time, as in row_errors_kernel -- eight
// lanes read the 128 bytes of one row with a 16-byte load each, so the scattered rows are read coalesced; the tile is
// padded to FR_DT + 1 floats for the lane = row accesses.  The differences go back into the tile and leave it by the
// same pattern, so the stores to E are coalesced too.  Both lists were checked on the host: every entry is in range.
constexpr int FR_DT = 32;

template <bool VEC4>
__global__ __launch_bounds__(64) void row_residuals_kernel(CodeSrc src, const float *__restrict__ cents, int d, int k,
                                                           const float *__restrict__ X, const int *__restrict__ rows,
                                                           const int *__restrict__ vrows, int s, GroupBase gb,
                                                           float *__restrict__ out) {
  __shared__ float xs[64 * (FR_DT + 1)];
  __shared__ int rs[64];
  const int lane = threadIdx.x;
  const int t0 = blockIdx.x * 64, t = t0 + lane;
  const bool active = t < s;
  const int row = active ? rows[t] : 0;
  rs[lane] = active ? vrows[t] : -1;
  const float *base = (active && gb.gcent) ? group_centroid(gb.gcent, gb.bounds, gb.g, row, d) : nullptr;
  RowWalk y(src, cents, d, k, row);
  for (int d0 = 0; d0 < d; d0 += FR_DT) {
    __syncthreads();                            // the previous step's tile has been stored (and rs is written)
    if (VEC4) {
      for (int e = lane; e < 64 * (FR_DT / 4); e += 64) {
        const int r = e / (FR_DT / 4), c = (e % (FR_DT / 4)) * 4;
        const int rr = rs[r];
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (rr >= 0 && d0 + c < d) v = *(const f32x4 *)(X + (size_t)rr * d + d0 + c);
        float *o = xs + r * (FR_DT + 1) + c;
        o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
      }
    } else {
      for (int e = lane; e < 64 * FR_DT; e += 64) {
        const int r = e / FR_DT, c = e % FR_DT;
        const int rr = rs[r];
        xs[r * (FR_DT + 1) + c] = (rr >= 0 && d0 + c < d) ? X[(size_t)rr * d + d0 + c] : 0.f;
      }
    }
    __syncthreads();
    const int dl = min(FR_DT, d - d0);
    if (active) {
      for (int c = 0; c < dl; c++) {
        const int e = d0 + c;
        const float ce = y.value(e);
        const float ye = base ? base[e] + ce : ce;            // MathUtils.add
        xs[lane * (FR_DT + 1) + c] = xs[lane * (FR_DT + 1) + c] - ye;   // MathUtils.subtract
      }
    }
    __syncthreads();
    if (VEC4) {
      for (int e = lane; e < 64 * (FR_DT / 4); e += 64) {
        const int r = e / (FR_DT / 4), c = (e % (FR_DT / 4)) * 4;
        if (t0 + r < s && d0 + c < d) {
          const float *o = xs + r * (FR_DT + 1) + c;
          const f32x4 v = {o[0], o[1], o[2], o[3]};
          *(f32x4 *)(out + (size_t)(t0 + r) * d + d0 + c) = v;
        }
      }
    } else {
      for (int e = lane; e < 64 * FR_DT; e += 64) {
        const int r = e / FR_DT, c = e % FR_DT;
        if (t0 + r < s && d0 + c < d) out[(size_t)(t0 + r) * d + d0 + c] = xs[r * (FR_DT + 1) + c];
      }
    }
  }
}

void row_residuals(gulon_index *ix, GroupBase gb, const gulon_dataset *ds, const int32_t *rows,
                   const int32_t *vector_rows, int32_t s, gulon_dataset **out) {
  GULON_REQUIRE(ds != nullptr, "vectors is null");
  GULON_REQUIRE(out != nullptr, "out is null");
  *out = nullptr;
  GULON_REQUIRE(s >= 0, "s = %d", s);
  GULON_REQUIRE(s == 0 || (rows != nullptr && vector_rows != nullptr), "rows or vector_rows is null");
  GULON_REQUIRE(ds->d == ix->d, "vectors of dimension %d for an index of dimension %d", ds->d, ix->d);
  for (int t = 0; t < s; t++) {
    GULON_REQUIRE(rows[t] >= 0 && rows[t] < ix->n, "rows[%d] = %d outside [0, %d)", t, rows[t], ix->n);
    GULON_REQUIRE(vector_rows[t] >= 0 && vector_rows[t] < ds->n, "vector_rows[%d] = %d outside [0, %d)", t,
                  vector_rows[t], ds->n);
  }
  GULON_REQUIRE(ix->vec == 4 || ix->vec == 16 || ix->wide, "unexpected code word of %d bytes", ix->vec);
  const int d = ix->d;
  std::unique_ptr<gulon_dataset> e(new gulon_dataset());
  e->n = s; e->d = d;
  const size_t total = (size_t)s * d;
  e->x.alloc(std::max<size_t>(total, 1));
  if (total) {
    DevBuf<int> dr, dv;
    dr.upload(rows, (size_t)s);
    dv.upload(vector_rows, (size_t)s);
    const bool v4 = d % 4 == 0 && (uintptr_t)ds->x.p % 16 == 0 && (uintptr_t)e->x.p % 16 == 0;
    auto kern = v4 ? row_residuals_kernel<true> : row_residuals_kernel<false>;
    hipLaunchKernelGGL(kern, dim3(ceil_div(s, 64)), dim3(64), 0, nullptr, code_src(ix), ix->cents.p, d, ix->k, ds->x.p,
                       dr.p, dv.p, s, gb, e->x.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(nullptr));
  }
  *out = e.release();
}

// ---- re-ranking against codes --------------------------------------------------------------------------------------
// One workgroup per query, lane = candidate position, FC_THREADS positions per pass.  The query is staged in LDS
// (FC_QS components at a time; the whole of it, once, for d <= FC_QS).  A lane reads its candidate's coarse and fine
// code words (RowCodes) and walks e ascending: z_e = y_e + f_e, t = z_e - q_e, sum += t * t -- one running binary32 sum
// per lane, nothing reduced across lanes.  The c distances stay in LDS; the first wave replays them through the
// reference's heap (refine_replay.hpp: the ballot against the root, and from the first NaN taken into a filling heap
// every candidate through update itself -- the argument is refine.hip's, unchanged).
// dyn: the query's c distances, then (k > GULON_MAX_K) the LdsHeap's k values and k keys.
// out_count[q] = the result's length, or -1 when a candidate of the query is outside the coarse index or the map, or
// its fine row outside the fine index (see gulon_hip.h).
constexpr int FC_THREADS = 256;
constexpr int FC_QS = 4096;

__global__ __launch_bounds__(FC_THREADS) void refine_codes_kernel(
    CodeSrc csrc, const float *__restrict__ ccents, int ck, int cn, GroupBase gb, CodeSrc fsrc,
    const float *__restrict__ fcents, int fk, int fn, int d, const float *__restrict__ Q, const int *__restrict__ cand,
    int c, const int *__restrict__ fine_map, int map_len, int k, int *__restrict__ out_idx,
    float *__restrict__ out_dist, int *__restrict__ out_count) {
  __shared__ float qs[FC_QS];
  __shared__ int bad;
  extern __shared__ float fc_dyn[];
  float *sd = fc_dyn;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = blockIdx.x;
  const float *query = Q + (size_t)q * d;
  const int *qcand = cand + (size_t)q * c;
  if (tid == 0) bad = 0;                           // (ordered before its writers by the barriers of the first pass)

  const bool whole_query = d <= FC_QS;
  for (int p0 = 0; p0 < c; p0 += FC_THREADS) {
    const int p = p0 + tid;
    const int id = p < c ? qcand[p] : -1;
    int frow = id;
    bool outside = false;
    if (id >= 0) {
      if (fine_map != nullptr) {
        outside = id >= map_len;
        frow = outside ? -1 : fine_map[id];
      }
      outside = outside || id >= cn || frow < 0 || frow >= fn;
    }
    const bool live = id >= 0 && !outside;         // an entry reported below is not read
    const float *base = (live && gb.gcent) ? group_centroid(gb.gcent, gb.bounds, gb.g, id, d) : nullptr;
    RowWalk y(csrc, ccents, d, ck, live ? id : 0), f(fsrc, fcents, d, fk, live ? frow : 0);
    float acc = 0.f;
    for (int s0 = 0; s0 < d; s0 += FC_QS) {
      const int s1 = min(d, s0 + FC_QS);
      if (!whole_query || p0 == 0) {
        __syncthreads();                           // the previous piece of the query has been read
        for (int i = s0 + tid; i < s1; i += FC_THREADS) qs[i - s0] = query[i];
        __syncthreads();
      }
      if (live) {
        for (int e = s0; e < s1; e++) {
          const float ce = y.value(e);
          const float ye = base ? base[e] + ce : ce;          // MathUtils.add: y_r first
          const float ze = ye + f.value(e);                   // then the fine coordinate
          const float t = ze - qs[e - s0];                    // MathUtils.distanceSq: unfused, e ascending
          acc += t * t;
        }
      }
    }
    if (outside) bad = 1;
    if (p < c) sd[p] = acc;
  }
  __syncthreads();
  if (wave != 0) return;

  int *oi = out_idx + (size_t)q * k;
  float *od = out_dist + (size_t)q * k;
  int count;
  auto put = [&](int i, int kk, float x) {
    if (lane == 0) { oi[i] = kk; od[i] = x; }
  };
  if (k <= GULON_MAX_K) {
    RegHeap h(k, lane);
    refine_replay(h, qcand, sd, c, lane);
    count = h.size;
    h.drain(put);
  } else {
    LdsHeap h(fc_dyn + c, (int *)(fc_dyn + c + k), k, lane);
    refine_replay(h, qcand, sd, c, lane);
    count = h.size;
    h.drain(put);
  }
  for (int i = count + lane; i < k; i += 64) { oi[i] = -1; od[i] = 0.f; }
  if (lane == 0) out_count[q] = bad ? -1 : count;
}

size_t refine_codes_dyn_lds(int c, int k) {
  return sizeof(float) * ((size_t)c + (k > GULON_MAX_K ? 2 * (size_t)k : 0));
}

void check_refine_codes_args(const gulon_index *coarse, const gulon_index *fine, int32_t b, int32_t c,
                             const int32_t *fine_map, int32_t map_len, int32_t k_nn) {
  GULON_REQUIRE(fine != nullptr, "fine index is null");
  GULON_REQUIRE(coarse->d == fine->d, "a fine index of dimension %d for an index of dimension %d", fine->d, coarse->d);
  GULON_REQUIRE(b >= 0 && k_nn >= 1 && c >= k_nn, "bad arguments b=%d c=%d k_nn=%d (1 <= k_nn <= c)", b, c, k_nn);
  GULON_REQUIRE(fine_map == nullptr || map_len >= 0, "map_len = %d", map_len);
  GULON_UNSUPPORTED(c > GULON_MAX_K_PEELED, "c = %d > %d", c, GULON_MAX_K_PEELED);
  for (const gulon_index *ix : {coarse, fine})
    GULON_REQUIRE(ix->vec == 4 || ix->vec == 16 || ix->wide, "unexpected code word of %d bytes", ix->vec);
  // the query piece, the c distances and the heap of k > GULON_MAX_K share one workgroup's LDS (160 KiB on gfx950)
  static_assert(sizeof(float) * FC_QS + 64 + sizeof(float) * 3 * (size_t)GULON_MAX_K_PEELED <= 160 * 1024, "LDS");
}

void refine_codes_dev(gulon_index *coarse, GroupBase gb, gulon_index *fine, const float *d_queries, int32_t b,
                      const int32_t *d_cand_rows, int32_t c, const int32_t *d_fine_map, int32_t map_len, int32_t k_nn,
                      int32_t *d_out_idx, float *d_out_dist, int32_t *d_out_count, hipStream_t st) {
  check_refine_codes_args(coarse, fine, b, c, d_fine_map, map_len, k_nn);
  if (b == 0) return;
  GULON_REQUIRE(d_queries && d_cand_rows && d_out_idx && d_out_dist && d_out_count, "null argument");
  const size_t lds = refine_codes_dyn_lds(c, k_nn);
  HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(refine_codes_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(refine_codes_kernel, dim3(b), dim3(FC_THREADS), lds, st, code_src(coarse), coarse->cents.p,
                     coarse->k, coarse->n, gb, code_src(fine), fine->cents.p, fine->k, fine->n, coarse->d, d_queries,
                     d_cand_rows, c, d_fine_map, map_len, k_nn, d_out_idx, d_out_dist, d_out_count);
  HIP_CHECK(hipGetLastError());
}

void refine_codes_host(gulon_index *coarse, GroupBase gb, gulon_index *fine, const float *queries, int32_t b,
                       const int32_t *cand_rows, int32_t c, const int32_t *fine_map, int32_t map_len, int32_t k_nn,
                       int32_t *out_idx, float *out_dist, int32_t *out_count) {
  check_refine_codes_args(coarse, fine, b, c, fine_map, map_len, k_nn);
  if (b == 0) return;
  GULON_REQUIRE(queries && cand_rows && out_idx && out_dist && out_count, "null argument");
  const size_t bc = (size_t)b * c, bk = (size_t)b * k_nn;
  DevBuf<float> dq, dod(bk);
  DevBuf<int> dc, dmap, doi(bk), doc((size_t)b);
  dq.upload(queries, (size_t)b * coarse->d);
  dc.upload(cand_rows, bc);
  if (fine_map != nullptr) dmap.upload(fine_map, (size_t)map_len);
  // (an empty map still has to read as a map: every candidate is then outside it)
  const int32_t *map_arg = fine_map == nullptr ? nullptr : (map_len ? dmap.p : (const int32_t *)dc.p);
  refine_codes_dev(coarse, gb, fine, dq.p, b, dc.p, c, map_arg, map_len, k_nn, doi.p, dod.p, doc.p, nullptr);
  doi.download(out_idx, bk);
  dod.download(out_dist, bk);
  doc.download(out_count, (size_t)b);
  HIP_CHECK(hipDeviceSynchronize());
  for (int q = 0; q < b; q++) {
    if (out_count[q] >= 0) continue;
    for (int p = 0; p < c; p++) {                  // name the offender
      const int id = cand_rows[(size_t)q * c + p];
      if (id < 0) continue;
      GULON_REQUIRE(id < coarse->n, "row %d out of range [0,%d)", id, coarse->n);
      GULON_REQUIRE(fine_map == nullptr || id < map_len, "candidate row %d outside the fine map [0,%d)", id, map_len);
      const int frow = fine_map ? fine_map[id] : id;
      GULON_REQUIRE(frow >= 0 && frow < fine->n, "fine row %d out of range [0,%d)", frow, fine->n);
    }
    GULON_REQUIRE(false, "query %d has a candidate row outside the indexes", q);
  }
}

const GroupBase FLAT{nullptr, nullptr, 0};

}  // namespace
}  // namespace gulon

using namespace gulon;

GULON_API int32_t gulon_index_row_residuals(gulon_index *idx, const gulon_dataset *vectors, const int32_t *rows,
                                            const int32_t *vector_rows, int32_t s, gulon_dataset **out) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    row_residuals(idx, FLAT, vectors, rows, vector_rows, s, out);
  });
}

GULON_API int32_t gulon_grouped_index_row_residuals(gulon_grouped_index *idx, const gulon_dataset *vectors,
                                                    const int32_t *rows, const int32_t *vector_rows, int32_t s,
                                                    gulon_dataset **out) {
  return guarded([&] {
    GULON_REQUIRE(idx != nullptr, "index is null");
    const GroupedParts gp = grouped_parts(idx);
    row_residuals(gp.pq, group_base(gp), vectors, rows, vector_rows, s, out);
  });
}

GULON_API int32_t gulon_index_refine_codes_topk(gulon_index *coarse, gulon_index *fine, const float *queries, int32_t b,
                                                const int32_t *cand_rows, int32_t c, const int32_t *fine_map,
                                                int32_t map_len, int32_t k_nn, int32_t *out_idx, float *out_dist,
                                                int32_t *out_count) {
  return guarded([&] {
    GULON_REQUIRE(coarse != nullptr, "index is null");
    refine_codes_host(coarse, FLAT, fine, queries, b, cand_rows, c, fine_map, map_len, k_nn, out_idx, out_dist,
                      out_count);
  });
}

GULON_API int32_t gulon_index_refine_codes_topk_dev(gulon_index *coarse, gulon_index *fine, const float *d_queries,
                                                    int32_t b, const int32_t *d_cand_rows, int32_t c,
                                                    const int32_t *d_fine_map, int32_t map_len, int32_t k_nn,
                                                    int32_t *d_out_idx, float *d_out_dist, int32_t *d_out_count,
                                                    void *stream) {
  return guarded([&] {
    GULON_REQUIRE(coarse != nullptr, "index is null");
    refine_codes_dev(coarse, FLAT, fine, d_queries, b, d_cand_rows, c, d_fine_map, map_len, k_nn, d_out_idx, d_out_dist,
                     d_out_count, (hipStream_t)stream);
  });
}

GULON_API int32_t gulon_grouped_index_refine_codes_topk(gulon_grouped_index *coarse, gulon_index *fine,
                                                        const float *queries, int32_t b, const int32_t *cand_rows,
                                                        int32_t c, const int32_t *fine_map, int32_t map_len,
                                                        int32_t k_nn, int32_t *out_idx, float *out_dist,
                                                        int32_t *out_count) {
  return guarded([&] {
    GULON_REQUIRE(coarse != nullptr, "index is null");
    const GroupedParts gp = grouped_parts(coarse);
    refine_codes_host(gp.pq, group_base(gp), fine, queries, b, cand_rows, c, fine_map, map_len, k_nn, out_idx, out_dist,
                      out_count);
  });
}

GULON_API int32_t gulon_grouped_index_refine_codes_topk_dev(gulon_grouped_index *coarse, gulon_index *fine,
                                                            const float *d_queries, int32_t b,
                                                            const int32_t *d_cand_rows, int32_t c,
                                                            const int32_t *d_fine_map, int32_t map_len, int32_t k_nn,
                                                            int32_t *d_out_idx, float *d_out_dist,
                                                            int32_t *d_out_count, void *stream) {
  return guarded([&] {
    GULON_REQUIRE(coarse != nullptr, "index is null");
    const GroupedParts gp = grouped_parts(coarse);
    refine_codes_dev(gp.pq, group_base(gp), fine, d_queries, b, d_cand_rows, c, d_fine_map, map_len, k_nn, d_out_idx,
                     d_out_dist, d_out_count, (hipStream_t)stream);
  });
}
