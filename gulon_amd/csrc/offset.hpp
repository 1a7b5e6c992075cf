// Offset queries: what offset.hip offers the handles that answer them.
#pragma once
#include "scan.hpp"

namespace gulon {

// The host-pointer forms check everything before anything is launched: b >= 0 (GULON_ERR_INVALID_ARGUMENT),
// 1 <= k_nn <= GULON_MAX_K (GULON_ERR_UNSUPPORTED), no NaN or -inf among the `rows` offsets, and every exclude[q]
// (nullable) either -1 or in [id_base, id_base + rows).
void check_offset_host(const float *offsets, int rows, const int *exclude, int b, int k_nn, int id_base);

// Rows [from, until) of `ds` against the b queries at d_q [b][d]: t = distance + d_offsets[row], the finite ones that
// are not d_exclude[q] (nullable) by (t, row), the first k_nn to out_idx / out_key [b][k_nn] and out_count [b]
// (nullable), all on `st`.  The caller holds the handle's mutex and orders the stream.
void launch_offset_exact(const gulon_dataset *ds, int from, int until, OffsetWork &x, const float *d_q, int b, int k_nn,
                         const float *d_offsets, const int *d_exclude, int *out_idx, float *out_key, int *out_count,
                         hipStream_t st);

}  // namespace gulon
