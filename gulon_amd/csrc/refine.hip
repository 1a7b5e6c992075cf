// Exact re-ranking of an index's candidates against the original vectors (DESIGN.md "Refined queries"): for every query
//   heap = TopKHeap(k); for p = 0 .. c-1 in order: heap.update(cand[p], MathUtils.distanceSq(query, V[map[cand[p]]]));
//   Result.fromHeap(heap)
// (TopKHeap.scala:69-79, MathUtils.scala:85-95, Index.scala:83-94).  One workgroup per query: all of it gathers the
// candidates' rows and sums their distances (row_tile.hpp, the bits of gulon_recall_counts), the c distances stay in
// LDS, and the workgroup's first wave then replays them through the reference's heap in candidate order
// (refine_replay.hpp, shared with fine.hip: resolve_candidate, the replay and its stores, the argument checks).
#include "row_tile.hpp"
#include "refine_replay.hpp"

namespace gulon {

// dyn: refine_dyn_lds.
// out_count[q] = the result's length, or -1 when a candidate of the query has no row in X (see gulon_hip.h).
template <bool VEC4>
__global__ __launch_bounds__(RC_THREADS) void refine_topk_kernel(
    const float *__restrict__ X, int n, int d, const float *__restrict__ Q, const int *__restrict__ cand, int c,
    const int *__restrict__ row_map, int map_len, int k, int *__restrict__ out_idx, float *__restrict__ out_dist,
    int *__restrict__ out_count) {
  __shared__ RowTile tile;
  __shared__ int bad;
  extern __shared__ float rf_dyn[];
  float *sd = rf_dyn;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = blockIdx.x;
  const float *query = Q + (size_t)q * d;
  const int *qcand = cand + (size_t)q * c;
  if (tid == 0) bad = 0;                           // (ordered before its readers by the barriers of the first pass)

  const bool whole_query = d <= RC_QS;
  for (int p0 = 0; p0 < c; p0 += RC_THREADS) {
    const int p = p0 + tid;
    const int id = p < c ? qcand[p] : -1;
    const Candidate cd = resolve_candidate(id, row_map, map_len, n);   // outside: reported below, not read
    const float acc = tile_distance_sq<VEC4>(tile, X, d, query, cd.row, !whole_query || p0 == 0);
    if (cd.outside) bad = 1;
    if (p < c) sd[p] = acc;
  }
  __syncthreads();
  if (wave != 0) return;

  refine_replay_store(qcand, sd, c, k, lane, bad != 0, out_idx + (size_t)q * k, out_dist + (size_t)q * k,
                      out_count + q);
}

static void check_refine_args(const gulon_dataset *ds, int32_t b, int32_t c, const int32_t *row_map, int32_t map_len,
                              int32_t k_nn) {
  GULON_REQUIRE(ds != nullptr, "dataset is null");
  check_refine_shape(b, c, row_map != nullptr, map_len, k_nn);
  // the tile, the c distances and the heap of k > GULON_MAX_K share one workgroup's LDS (160 KiB on gfx950)
  static_assert(sizeof(RowTile) + 64 + sizeof(float) * 3 * (size_t)GULON_MAX_K_PEELED <= 160 * 1024, "LDS");
}

}  // namespace gulon

using namespace gulon;

GULON_API int32_t gulon_refine_topk_dev(const gulon_dataset *ds, const float *d_queries, int32_t b,
                                        const int32_t *d_cand_rows, int32_t c, const int32_t *d_row_map,
                                        int32_t map_len, int32_t k_nn, int32_t *d_out_idx, float *d_out_dist,
                                        int32_t *d_out_count, void *stream) {
  return guarded([&] {
    check_refine_args(ds, b, c, d_row_map, map_len, k_nn);
    if (b == 0) return;
    GULON_REQUIRE(d_queries && d_cand_rows && d_out_idx && d_out_dist && d_out_count, "null argument");
    const int d = ds->d;
    const size_t lds = refine_dyn_lds(c, k_nn);
    const bool vec4 = d % 4 == 0 && (uintptr_t)ds->x.p % 16 == 0;
    auto kern = vec4 ? refine_topk_kernel<true> : refine_topk_kernel<false>;
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds));
    hipLaunchKernelGGL(kern, dim3(b), dim3(RC_THREADS), lds, (hipStream_t)stream, ds->x.p, ds->n, d, d_queries,
                       d_cand_rows, c, d_row_map, map_len, k_nn, d_out_idx, d_out_dist, d_out_count);
    HIP_CHECK(hipGetLastError());
  });
}

GULON_API int32_t gulon_refine_topk(const gulon_dataset *ds, const float *queries, int32_t b, const int32_t *cand_rows,
                                    int32_t c, const int32_t *row_map, int32_t map_len, int32_t k_nn, int32_t *out_idx,
                                    float *out_dist, int32_t *out_count) {
  return guarded([&] {
    check_refine_args(ds, b, c, row_map, map_len, k_nn);
    refine_host_form(ds->d, queries, b, cand_rows, c, row_map, map_len, k_nn, out_idx, out_dist, out_count,
                     [&](const float *dq, const int *dc, const int *dmap, int *doi, float *dod, int *doc) {
                       const int32_t rc =
                           gulon_refine_topk_dev(ds, dq, b, dc, c, dmap, map_len, k_nn, doi, dod, doc, nullptr);
                       if (rc != GULON_OK) throw DeviceError{rc};
                     });
    name_refine_offender(out_count, cand_rows, b, c, "dataset", [&](int id) {
      GULON_REQUIRE(row_map == nullptr || id < map_len, "candidate row %d outside the row map [0,%d)", id, map_len);
      const int row = row_map ? row_map[id] : id;
      GULON_REQUIRE(row >= 0 && row < ds->n, "row %d out of range [0,%d)", row, ds->n);
    });
  });
}
