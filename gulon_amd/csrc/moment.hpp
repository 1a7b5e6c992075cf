// The binary64 cross moment (rotate.hip) as alignment.hip asks it: over a list of row pairs instead of every row.
#pragma once
#include "common.hpp"

namespace gulon {

// out[p * db + q] = sum_i a[ra(i)][p] * b[rb(i)][q] over i in [0, n), binary64, to host memory; null stream, returns
// after the result has arrived.  d_rows_a == nullptr: ra(i) = rb(i) = i (gulon_dataset_moment).  Otherwise both are
// device lists of n rows, ra(i) = d_rows_a[i], rb(i) = d_rows_b[i], and an i with a negative row on either side stages
// zeros; rows at or above their matrix's row count are not checked.  The list is cut by position into chunks of
// rotate.hip's MOMENT_ROWS, each summed i ascending from 0.0, the chunks added in ascending order: with the identity
// lists the bits are gulon_dataset_moment's.  n = 0 gives zeros; n outside what the chunk counter holds is refused.
void moment_rows(const float *d_a, int da, const float *d_b, int db, const int *d_rows_a, const int *d_rows_b,
                 long long n, double *out);

}  // namespace gulon
