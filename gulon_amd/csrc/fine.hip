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
// group whose row range holds r (row_decode.hpp group_centroid, not the binarySearch rule of GroupedIndex.lookup).  The
// fine coordinate is added last.  Rows are read through row_decode.hpp's RowWalk over RowCodes, in the layout each
// handle keeps, clamped to the code book; the coarse and the fine index share d and nothing else.  The originals pass
// through row_tile.hpp's tile, the replay and its stores are refine_replay.hpp's.  Both calls use scratch of their own:
// a handle keeps no trace of them.
#include "refine_replay.hpp"
#include "row_decode.hpp"
#include "row_tile.hpp"

namespace gulon {
namespace {

// ---- residuals -----------------------------------------------------------------------------------------------------
// One wavefront per tile of 64 list positions, lane = position: lane t decodes row rows[t] of the index while the 64
// originals V[vector_rows[t]] pass through the gathered tile (row_tile.hpp tile_load), so the scattered rows are read
// coalesced.  The differences go back into the tile and leave it by the same pattern (tile_store), so the stores to E
// are coalesced too.  Both lists were checked on the host: every entry is in range.
template <bool VEC4>
__global__ __launch_bounds__(64) void row_residuals_kernel(CodeSrc src, const float *__restrict__ cents, int d, int k,
                                                           const float *__restrict__ X, const int *__restrict__ rows,
                                                           const int *__restrict__ vrows, int s, GroupBase gb,
                                                           float *__restrict__ out) {
  __shared__ float xs[tile_floats(64)];
  __shared__ int rs[64];
  const int lane = threadIdx.x;
  const int t0 = blockIdx.x * 64, t = t0 + lane;
  const bool active = t < s;
  const int row = active ? rows[t] : 0;
  rs[lane] = active ? vrows[t] : -1;
  const float *base = (active && gb.gcent) ? group_centroid(gb, row, d) : nullptr;
  RowWalk<RowCodes> y(RowCodes(src, row), cents, d, src.m, k, k - 1);   // a code at or above k reads as k - 1
  for (int d0 = 0; d0 < d; d0 += RC_DT) {
    __syncthreads();                            // the previous step's tile has been stored (and rs is written)
    tile_load<64, VEC4>(xs, rs, X, d, d0, d);
    __syncthreads();
    const int dl = min(RC_DT, d - d0);
    if (active) {
      for (int c = 0; c < dl; c++) {
        const int e = d0 + c;
        const float ce = y.value(e);
        const float ye = base ? base[e] + ce : ce;            // MathUtils.add
        tile_at(xs, lane, c) = tile_at(xs, lane, c) - ye;     // MathUtils.subtract
      }
    }
    __syncthreads();
    tile_store<64, VEC4>(xs, out, t0, s - t0, d, d0);
  }
}

void row_residuals(const IndexRef &r, const gulon_dataset *ds, const int32_t *rows,
                   const int32_t *vector_rows, int32_t s, gulon_dataset **out) {
  gulon_index *ix = r.ix;
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
  require_code_layout(ix);
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
                       dr.p, dv.p, s, r.gb, e->x.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(nullptr));
  }
  *out = e.release();
}

// ---- re-ranking against codes --------------------------------------------------------------------------------------
// One workgroup per query, lane = candidate position, FC_THREADS positions per pass.  The query is staged in LDS
// (FC_QS components at a time; the whole of it, once, for d <= FC_QS).  A lane reads its candidate's coarse and fine
// code words (two RowWalks) and walks e ascending: z_e = y_e + f_e, t = z_e - q_e, sum += t * t -- one running binary32
// sum per lane, nothing reduced across lanes.  The c distances stay in LDS; the first wave replays them through the
// reference's heap (refine_replay.hpp: the ballot against the root, and from the first NaN taken into a filling heap
// every candidate through update itself).  dyn: refine_dyn_lds.
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
    const Candidate fc = resolve_candidate(id, fine_map, map_len, fn);
    const bool outside = fc.outside || id >= cn;
    const bool live = id >= 0 && !outside;         // an entry reported below is not read
    const float *base = (live && gb.gcent) ? group_centroid(gb, id, d) : nullptr;
    // (a code at or above its code book's k reads as k - 1)
    RowWalk<RowCodes> y(RowCodes(csrc, live ? id : 0), ccents, d, csrc.m, ck, ck - 1);
    RowWalk<RowCodes> f(RowCodes(fsrc, live ? fc.row : 0), fcents, d, fsrc.m, fk, fk - 1);
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

  refine_replay_store(qcand, sd, c, k, lane, bad != 0, out_idx + (size_t)q * k, out_dist + (size_t)q * k,
                      out_count + q);
}

void check_refine_codes_args(const gulon_index *coarse, const gulon_index *fine, int32_t b, int32_t c,
                             const int32_t *fine_map, int32_t map_len, int32_t k_nn) {
  GULON_REQUIRE(fine != nullptr, "fine index is null");
  GULON_REQUIRE(coarse->d == fine->d, "a fine index of dimension %d for an index of dimension %d", fine->d, coarse->d);
  check_refine_shape(b, c, fine_map != nullptr, map_len, k_nn);
  require_code_layout(coarse);
  require_code_layout(fine);
  // the query piece, the c distances and the heap of k > GULON_MAX_K share one workgroup's LDS (160 KiB on gfx950)
  static_assert(sizeof(float) * FC_QS + 64 + sizeof(float) * 3 * (size_t)GULON_MAX_K_PEELED <= 160 * 1024, "LDS");
}

void refine_codes_dev(const IndexRef &cr, gulon_index *fine, const float *d_queries, int32_t b,
                      const int32_t *d_cand_rows, int32_t c, const int32_t *d_fine_map, int32_t map_len, int32_t k_nn,
                      int32_t *d_out_idx, float *d_out_dist, int32_t *d_out_count, hipStream_t st) {
  gulon_index *coarse = cr.ix;
  check_refine_codes_args(coarse, fine, b, c, d_fine_map, map_len, k_nn);
  if (b == 0) return;
  GULON_REQUIRE(d_queries && d_cand_rows && d_out_idx && d_out_dist && d_out_count, "null argument");
  const size_t lds = refine_dyn_lds(c, k_nn);
  HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(refine_codes_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(refine_codes_kernel, dim3(b), dim3(FC_THREADS), lds, st, code_src(coarse), coarse->cents.p,
                     coarse->k, coarse->n, cr.gb, code_src(fine), fine->cents.p, fine->k, fine->n, coarse->d, d_queries,
                     d_cand_rows, c, d_fine_map, map_len, k_nn, d_out_idx, d_out_dist, d_out_count);
  HIP_CHECK(hipGetLastError());
}

void refine_codes_host(const IndexRef &cr, gulon_index *fine, const float *queries, int32_t b,
                       const int32_t *cand_rows, int32_t c, const int32_t *fine_map, int32_t map_len, int32_t k_nn,
                       int32_t *out_idx, float *out_dist, int32_t *out_count) {
  gulon_index *coarse = cr.ix;
  check_refine_codes_args(coarse, fine, b, c, fine_map, map_len, k_nn);
  refine_host_form(coarse->d, queries, b, cand_rows, c, fine_map, map_len, k_nn, out_idx, out_dist, out_count,
                   [&](const float *dq, const int *dc, const int *dmap, int *doi, float *dod, int *doc) {
                     refine_codes_dev(cr, fine, dq, b, dc, c, dmap, map_len, k_nn, doi, dod, doc, nullptr);
                   });
  name_refine_offender(out_count, cand_rows, b, c, "indexes", [&](int id) {
    GULON_REQUIRE(id < coarse->n, "row %d out of range [0,%d)", id, coarse->n);
    GULON_REQUIRE(fine_map == nullptr || id < map_len, "candidate row %d outside the fine map [0,%d)", id, map_len);
    const int frow = fine_map ? fine_map[id] : id;
    GULON_REQUIRE(frow >= 0 && frow < fine->n, "fine row %d out of range [0,%d)", frow, fine->n);
  });
}

}  // namespace
}  // namespace gulon

using namespace gulon;

GULON_API int32_t gulon_index_row_residuals(gulon_index *idx, const gulon_dataset *vectors, const int32_t *rows,
                                            const int32_t *vector_rows, int32_t s, gulon_dataset **out) {
  return guarded([&] { row_residuals(index_ref(idx), vectors, rows, vector_rows, s, out); });
}

GULON_API int32_t gulon_grouped_index_row_residuals(gulon_grouped_index *idx, const gulon_dataset *vectors,
                                                    const int32_t *rows, const int32_t *vector_rows, int32_t s,
                                                    gulon_dataset **out) {
  return guarded([&] { row_residuals(index_ref(idx), vectors, rows, vector_rows, s, out); });
}

GULON_API int32_t gulon_index_refine_codes_topk(gulon_index *coarse, gulon_index *fine, const float *queries, int32_t b,
                                                const int32_t *cand_rows, int32_t c, const int32_t *fine_map,
                                                int32_t map_len, int32_t k_nn, int32_t *out_idx, float *out_dist,
                                                int32_t *out_count) {
  return guarded([&] {
    refine_codes_host(index_ref(coarse), fine, queries, b, cand_rows, c, fine_map, map_len, k_nn, out_idx, out_dist,
                      out_count);
  });
}

GULON_API int32_t gulon_index_refine_codes_topk_dev(gulon_index *coarse, gulon_index *fine, const float *d_queries,
                                                    int32_t b, const int32_t *d_cand_rows, int32_t c,
                                                    const int32_t *d_fine_map, int32_t map_len, int32_t k_nn,
                                                    int32_t *d_out_idx, float *d_out_dist, int32_t *d_out_count,
                                                    void *stream) {
  return guarded([&] {
    refine_codes_dev(index_ref(coarse), fine, d_queries, b, d_cand_rows, c, d_fine_map, map_len, k_nn, d_out_idx,
                     d_out_dist, d_out_count, (hipStream_t)stream);
  });
}

GULON_API int32_t gulon_grouped_index_refine_codes_topk(gulon_grouped_index *coarse, gulon_index *fine,
                                                        const float *queries, int32_t b, const int32_t *cand_rows,
                                                        int32_t c, const int32_t *fine_map, int32_t map_len,
                                                        int32_t k_nn, int32_t *out_idx, float *out_dist,
                                                        int32_t *out_count) {
  return guarded([&] {
    refine_codes_host(index_ref(coarse), fine, queries, b, cand_rows, c, fine_map, map_len, k_nn, out_idx, out_dist,
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
    refine_codes_dev(index_ref(coarse), fine, d_queries, b, d_cand_rows, c, d_fine_map, map_len, k_nn, d_out_idx,
                     d_out_dist, d_out_count, (hipStream_t)stream);
  });
}
