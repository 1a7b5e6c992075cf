// Offset queries: what offset.hip offers the handles that answer them, and the slot and shape rules and
// the pass driver of its flat scan, which the rank queries (rank.hip) launch by as well.
#pragma once
#include "table_scan.hpp"

namespace gulon {

// LDS of one query slot: its table while the rows are scanned, then the NW wave lists of the slot for the merge
constexpr size_t flat_slot_bytes(int m_pad) {
  const size_t table = (size_t)m_pad * 256 * sizeof(float), lists = (size_t)(TABLE_SCAN_THREADS / 64) * 64 * 8;
  return table > lists ? table : lists;
}

// the queries of one pass, the row chunks and the 64-row code blocks of one chunk, for b queries E to a workgroup
struct FlatShape { int per_pass, nchunks, rb_per_chunk; };
inline FlatShape offset_flat_shape(const gulon_index *ix, int from, int until, int b, int E) {
  constexpr int NW = TABLE_SCAN_THREADS / 64;
  const size_t tab = (size_t)ix->m_pad * 256;
  int sub = (int)std::max<size_t>(1, FLAT_TABLE_BYTES / (tab * sizeof(float)));
  sub = std::max(sub / E * E, E);
  const int groups = ceil_div(std::min(sub, b), E);
  const int rb_total = ceil_div(until, 64) - from / 64;
  const int want = std::max(1, ceil_div(2048, groups));
  const int nchunks_max = std::max(1, rb_total / (2 * NW));
  const int rb_per_chunk = std::max(1, ceil_div(rb_total, std::min(want, nchunks_max)));
  return {sub, std::max(1, ceil_div(rb_total, rb_per_chunk)), rb_per_chunk};
}

// the query slots of a workgroup: the largest of 8, 4, 2, 1 that fit the LDS budget, 0 if not even one does
inline int offset_flat_max_e(const gulon_index *ix) {
  const size_t fit = TABLE_LDS_BUDGET / flat_slot_bytes(ix->m_pad);
  return fit >= 8 ? 8 : fit >= 4 ? 4 : fit >= 2 ? 2 : (int)fit;
}
// ... and of a batch of b: no more slots than a small batch fills
inline int offset_flat_slots(const gulon_index *ix, int b) {
  int E = offset_flat_max_e(ix);
  while (E > 1 && E / 2 >= b) E /= 2;
  return E;
}

inline void check_flat(const gulon_index *ix, int b, int k_nn, int from, int until) {
  GULON_REQUIRE(b >= 0, "batch size must be non-negative");
  GULON_UNSUPPORTED(k_nn < 1 || k_nn > GULON_MAX_K, "k_nn = %d outside [1, %d]", k_nn, GULON_MAX_K);
  GULON_UNSUPPORTED(ix->wide, "offset queries take byte codes: k = %d > 256 is not supported", ix->k);
  GULON_UNSUPPORTED(ix->is_view, "offset queries are not supported on an index view");
  GULON_REQUIRE(from <= until, "expected: from <= until");
  GULON_REQUIRE(from >= 0 && until <= ix->n, "expected: from >= 0 && until <= length");
  GULON_UNSUPPORTED(offset_flat_max_e(ix) < 1, "m = %d: the tables of one query need %d KiB of LDS, %d KiB are there",
                    ix->m, ix->m_pad, (int)(TABLE_LDS_BUDGET / 1024));
}

// The passes of a flat scan over the b queries at d_q, rows [from, until): under the handle's mutex and one StreamOrder
// on `st`, per pass of nb queries from q0 on their Index.prepareQuery tables into `tables` (launch_build_tables), then
// pass(q0, nb, E, shape) -- the family's buffers, kernels and tail.  Called with the workspace's mutex held and the
// handle's free.
template <class Pass>
void flat_passes(gulon_index *ix, DevBuf<float> &tables, const float *d_q, int b, int from, int until, hipStream_t st,
                 Pass pass) {
  const int E = offset_flat_slots(ix, b);
  const int sub = offset_flat_shape(ix, from, until, b, E).per_pass;
  std::lock_guard<std::mutex> lock(ix->mu);
  ix->pend_b = -1;
  StreamOrder so(ix, st);
  for (int q0 = 0; q0 < b; q0 += sub) {
    const int nb = std::min(sub, b - q0);
    const FlatShape s = offset_flat_shape(ix, from, until, nb, E);
    tables.ensure((size_t)nb * ix->m_pad * 256);
    launch_build_tables(1, ix, d_q + (size_t)q0 * ix->d, nb, nb, tables.p, st);
    pass(q0, nb, E, s);
  }
  so.done();
}

// The host-pointer forms check everything before anything is launched (GULON_ERR_INVALID_ARGUMENT naming the first bad
// entry).  check_rows_host: no NaN or -inf among the `rows` offsets (null only where `nullable`: +0 for every row), and
// every exclude[q] (nullable) either -1 or in [id_base, id_base + rows).  check_offset_host: b >= 0,
// 1 <= k_nn <= GULON_MAX_K (GULON_ERR_UNSUPPORTED), then that.
void check_rows_host(const float *offsets, bool nullable, int rows, const int *exclude, int b, int id_base);
void check_offset_host(const float *offsets, int rows, const int *exclude, int b, int k_nn, int id_base);

// Rows [from, until) of `ds` against the b queries at d_q [b][d]: t = distance + d_offsets[row], the finite ones that
// are not d_exclude[q] (nullable) by (t, row), the first k_nn to out_idx / out_key [b][k_nn] and out_count [b]
// (nullable), all on `st`.  The caller holds the handle's mutex and orders the stream.
void launch_offset_exact(const gulon_dataset *ds, int from, int until, OffsetWork &x, const float *d_q, int b, int k_nn,
                         const float *d_offsets, const int *d_exclude, int *out_idx, float *out_key, int *out_count,
                         hipStream_t st);

}  // namespace gulon
