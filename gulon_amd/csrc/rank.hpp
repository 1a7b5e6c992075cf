// Rank queries: what rank.hip offers the handles that answer them.
#pragma once
#include "offset.hpp"

namespace gulon {

// The host-pointer forms check everything before anything is launched (GULON_ERR_INVALID_ARGUMENT naming the first bad
// entry): b >= 0; no NaN or -inf among the `rows` offsets (nullable: +0 for every row); every exclude[q] (nullable)
// either -1 or in [id_base, id_base + rows); gold_offsets[0] == 0 and non-decreasing; every gold row in
// [id_base, id_base + rows).  Returns the number of gold rows, gold_offsets[b].
int check_rank_host(const float *offsets, int rows, const int *exclude, const int *gold_offsets, const int *gold_rows,
                    int b, int id_base);

// Rows [from, until) of `ds` against the b queries at d_q [b][d], all on `st`: per query the best gold row of its list
// (d_gold_off [b + 1], d_gold_rows) by (t, row) among the candidates -- t = distance + d_offsets[row] (d_offsets
// nullable: +0) finite, the row not d_exclude[q] (nullable) -- to out_row / out_key [b] (-1 / +inf: none), the number
// of candidates ahead of it to out_rank [b] (-1: none) and the number of candidates to out_total [b] (nullable).
// `gold` = the number of gold rows (host).  The caller holds the handle's mutex and orders the stream.
void launch_rank_exact(const gulon_dataset *ds, int from, int until, RankWork &x, const float *d_q, int b,
                       const float *d_offsets, const int *d_exclude, const int *d_gold_off, const int *d_gold_rows,
                       int gold, int *out_rank, int *out_row, float *out_key, int *out_total, hipStream_t st);

// The same over rows [from, until) of a flat byte-code index, ids row_base + r; called with x.mu held and the handle's
// mutex free.  The arguments are checked (check_flat) by the caller.
void launch_rank_flat(gulon_index *ix, RankWork &x, const float *d_q, int b, int from, int until, const float *d_offsets,
                      const int *d_exclude, const int *d_gold_off, const int *d_gold_rows, int *out_rank, int *out_row,
                      float *out_key, int *out_total, hipStream_t st);

}  // namespace gulon
