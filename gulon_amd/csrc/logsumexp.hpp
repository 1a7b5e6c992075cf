// The log-sum-exp scan of the exact index: what logsumexp.hip offers the handle that answers it.
#pragma once
#include "exact.hpp"

namespace gulon {

// Workspace of the log-sum-exp queries of one handle, used under the handle's mutex.
struct LseWork {
  DevBuf<float> qt;             // the queries transposed per workgroup [tile][d][16]
  DevBuf<double> part;          // the sum of every (query, row chunk)
  DevBuf<int> cnt;              // the terms of every (query, row chunk)
  DevBuf<float> q;              // the host-pointer form: queries
  DevBuf<int> ex, ft;           // ... the excluded rows, final term counts
  DevBuf<double> fl;            // ... final L
};

// Rows [from, until) of `ds` against the b queries at d_q [b][d], all on `st`.  Per query q and row r, d the distance
// bits of exact_tile: r is a term if and only if d is finite and r != d_exclude[q] (nullable; -1 excludes nothing);
// z = (double)d * zscale in one binary64 product, e = exp(z), S_q the sum of e over the terms, out_lse[q] = log(S_q)
// (-inf without a term, and where every term underflows to 0), out_terms[q] the number of terms.  Neither output is
// null.  The sum has a fixed order -- per lane the 256-row steps of its chunk ascending, the lanes of a wave by an xor
// butterfly 32 down to 1, the waves in wave order, the chunks ascending -- and no atomics: the bits are a function of
// (range, queries, b, zscale) alone.  The number of chunks follows the number of query tiles (knn_row_chunks), so the
// same query in a batch of another size may differ in its last bits.  The caller holds the handle's mutex and orders
// the stream.
void launch_logsumexp_exact(const gulon_dataset *ds, int from, int until, LseWork &x, const float *d_q, int b,
                            double zscale, const int *d_exclude, double *out_lse, int *out_terms, hipStream_t st);

}  // namespace gulon
