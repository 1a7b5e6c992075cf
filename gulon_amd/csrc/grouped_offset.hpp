// Offset queries on the grouped index: what grouped_offset.hip offers grouped.hip, which owns the handle.
#pragma once
#include "scan.hpp"

namespace gulon {

// Workspace of the offset queries of one grouped handle, used under the handle's mutex.
struct GroupedOffsetWork {
  DevBuf<float> off, pv;   // the row offsets of the host form; per (query, searched-group slot) lists of keys
  DevBuf<int> ex, pi;      // the excluded rows of the host form; the lists' rows
};

constexpr int GROUPED_OFFSET_SUB_BATCH = 1024;              // queries per pass: bounds the per-slot lists ...
constexpr long long GROUPED_OFFSET_LIST_ENTRIES = 1ll << 26;   // ... as does this, where a query searches very many groups
// queries of one pass for `slots` searched groups per query at most and lists of keff entries
inline int grouped_offset_pass(int slots, int keff) {
  const long long fit = GROUPED_OFFSET_LIST_ENTRIES / ((long long)(slots > 1 ? slots : 1) * keff);
  return (int)(fit < 1 ? 1 : fit < GROUPED_OFFSET_SUB_BATCH ? fit : GROUPED_OFFSET_SUB_BATCH);
}

// The residual index, the groups and one pass's coarse result (grouped.hip's coarse_stage): query q < nb searches groups
// nn[q * nn_stride + t], t < nn_cnt[q] <= stride.
struct GroupedOffsetPass {
  const gulon_index *pq;
  const float *gcent;      // [g][d]
  const int *bounds;       // [g + 1]
  const float *d_q;        // [nb][d]
  int nb;
  const int *nn, *nn_cnt;
  int nn_stride, stride;
  size_t lds_bytes;        // gq_group_scan's LDS for k_nn <= 63 (grouped.hip's group_scan_lds)
};

// Every row r of the searched groups of every query: t = distance + d_offsets[r] (indexed by grouped row position), the
// finite ones that are not d_exclude[q] (nullable) by (t, row), the first k_nn to out_idx / out_key [nb][k_nn] padded with
// -1 / +inf and out_count [nb] (nullable), all on `st`.  The caller has checked the arguments, holds the handle's mutex
// and orders the stream.
void launch_grouped_offset(const GroupedOffsetPass &p, GroupedOffsetWork &x, int k_nn, const float *d_offsets,
                           const int *d_exclude, int *out_idx, float *out_key, int *out_count, hipStream_t st);

}  // namespace gulon
