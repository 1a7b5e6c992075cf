// What refine.hip and fine.hip share (DESIGN.md "Row reading"): a candidate resolved to its row, a query's distances,
// already in LDS, offered to the reference's TopKHeap (topk_heap.hpp) in candidate order by one wavefront, the result
// stored, and the host-side checks of the common arguments.
#pragma once

#include "topk_heap.hpp"

namespace gulon {

// The replay is not c serial updates.  update(key, x) on a FULL heap does nothing unless root > x, so a candidate can be
// left out as soon as `root > x` is known to be false AT THE MOMENT THE REFERENCE WOULD INSPECT IT.  While the heap
// holds no NaN it is a max-heap in the ordinary sense: its root is its largest value, and an effective update replaces
// that by something smaller, so the root never increases -- a candidate that fails `root > x` against the root of NOW
// fails it against every later root too.  The wave therefore ballots 64 candidates at a time against the current root
// and runs update only for the set bits, lowest position first, asking again after every update (the root fell: more
// bits may clear).  The updates that run are the reference's effective ones in its order, those left out are no-ops:
// the same heap arrangement.  +-inf are ordinary values here, and a NaN candidate fails `root > NaN` like any no-op.
// A NaN INSIDE the heap (it can only get in while the heap fills) ends the argument: comparisons with it are false, so
// percolateUp stops below it and a value larger than the root can sit under it; delete moves the last slot to the
// root, which can then RISE.  From the first NaN taken in, every candidate goes through update itself, one by one,
// which makes the reference's own test at the reference's own moment.
template <class Heap>
__device__ void refine_replay(Heap &h, const int *__restrict__ qcand, const float *sd, int c, int lane) {
  bool nan_inside = false;
  for (int base = 0; base < c; base += 64) {
    const int p = base + lane;
    const int id = p < c ? qcand[p] : -1;
    const float x = p < c ? sd[p] : 0.f;
    unsigned long long pend = __ballot(id >= 0);           // a negative candidate is padding: never offered
    while (pend) {
      if (h.size == h.cap && !nan_inside) {
        pend &= __ballot(h.val(0) > x);
        if (!pend) break;
      }
      const int j = __builtin_amdgcn_readfirstlane(__ffsll((long long)pend) - 1);
      pend &= pend - 1;
      const float xj = readlane_f(x, j);
      if (h.size < h.cap && xj != xj) nan_inside = true;
      h.update(readlane_i(id, j), xj);
    }
  }
}

// Candidate id -> (row map) -> row of a table of n rows.  outside: the id is beyond the map, or its row beyond the
// table -- the caller reports it through `bad` and reads nothing for it (row = -1).  A negative id is padding: it stays
// as it is and is not outside.
struct Candidate { int row; bool outside; };
__device__ inline Candidate resolve_candidate(int id, const int *__restrict__ map, int map_len, int n) {
  int row = id;
  bool outside = false;
  if (id >= 0) {
    if (map != nullptr) {
      outside = id >= map_len;
      row = outside ? -1 : map[id];
    }
    outside = outside || row < 0 || row >= n;
    if (outside) row = -1;
  }
  return {row, outside};
}

// The tail of a re-ranking kernel, run by the workgroup's first wave once the c distances are in dyn[0..c): the replay
// through a heap of k (in registers up to GULON_MAX_K, else in dyn[c..c + 2k)), Result.fromHeap into oi / od, padded
// with -1 / 0.f, and the result's length -- or -1 when `bad` -- into *out_count.
__device__ inline void refine_replay_store(const int *__restrict__ qcand, float *dyn, int c, int k, int lane, bool bad,
                                           int *__restrict__ oi, float *__restrict__ od, int *__restrict__ out_count) {
  int count;
  auto put = [&](int i, int kk, float x) {
    if (lane == 0) { oi[i] = kk; od[i] = x; }
  };
  if (k <= GULON_MAX_K) {
    RegHeap h(k, lane);
    refine_replay(h, qcand, dyn, c, lane);
    count = h.size;
    h.drain(put);
  } else {
    LdsHeap h(dyn + c, (int *)(dyn + c + k), k, lane);
    refine_replay(h, qcand, dyn, c, lane);
    count = h.size;
    h.drain(put);
  }
  for (int i = count + lane; i < k; i += 64) { oi[i] = -1; od[i] = 0.f; }
  if (lane == 0) *out_count = bad ? -1 : count;
}

// dyn: the query's c distances, then (k > GULON_MAX_K) the LdsHeap's k values and k keys
inline size_t refine_dyn_lds(int c, int k) { return sizeof(float) * ((size_t)c + (k > GULON_MAX_K ? 2 * (size_t)k : 0)); }

inline void check_refine_shape(int32_t b, int32_t c, bool have_map, int32_t map_len, int32_t k_nn) {
  GULON_REQUIRE(b >= 0 && k_nn >= 1 && c >= k_nn, "bad arguments b=%d c=%d k_nn=%d (1 <= k_nn <= c)", b, c, k_nn);
  GULON_REQUIRE(!have_map || map_len >= 0, "map_len = %d", map_len);
  GULON_UNSUPPORTED(c > GULON_MAX_K_PEELED, "c = %d > %d", c, GULON_MAX_K_PEELED);
}

// The host form of a re-ranking call: the arguments go up, launch(d_queries, d_cand, d_map, d_idx, d_dist, d_count) runs
// the device form on the null stream, the results come down.  d: the queries' dimension.
template <class Launch>
void refine_host_form(int d, const float *queries, int32_t b, const int32_t *cand_rows, int32_t c, const int32_t *map,
                      int32_t map_len, int32_t k_nn, int32_t *out_idx, float *out_dist, int32_t *out_count,
                      Launch launch) {
  if (b == 0) return;
  GULON_REQUIRE(queries && cand_rows && out_idx && out_dist && out_count, "null argument");
  const size_t bc = (size_t)b * c, bk = (size_t)b * k_nn;
  DevBuf<float> dq, dod(bk);
  DevBuf<int> dc, dmap, doi(bk), doc((size_t)b);
  dq.upload(queries, (size_t)b * d);
  dc.upload(cand_rows, bc);
  if (map != nullptr) dmap.upload(map, (size_t)map_len);
  // (an empty map still has to read as a map: every candidate is then outside it)
  const int32_t *map_arg = map == nullptr ? nullptr : (map_len ? dmap.p : (const int32_t *)dc.p);
  launch(dq.p, dc.p, map_arg, doi.p, dod.p, doc.p);
  doi.download(out_idx, bk);
  dod.download(out_dist, bk);
  doc.download(out_count, (size_t)b);
  HIP_CHECK(hipDeviceSynchronize());
}

// The host forms after out_count[q] < 0: check(id) names the offender among the query's candidates (it throws)
template <class Check>
void name_refine_offender(const int32_t *out_count, const int32_t *cand_rows, int b, int c, const char *tables,
                          Check check) {
  for (int q = 0; q < b; q++) {
    if (out_count[q] >= 0) continue;
    for (int p = 0; p < c; p++) {
      const int id = cand_rows[(size_t)q * c + p];
      if (id >= 0) check(id);
    }
    GULON_REQUIRE(false, "query %d has a candidate row outside the %s", q, tables);
  }
}

}  // namespace gulon
