// Multiplicative analogy queries, 3CosMul: what cosmul.hip offers the handles that answer them.
#pragma once
#include "compose.hpp"
#include "table_scan.hpp"   // TABLE_LDS_BUDGET, the tables of one question of the flat form

namespace gulon {

constexpr int COSMUL_MAX_TERMS = 8;                  // terms of one expression

// The host-pointer forms check everything before anything is launched (GULON_ERR_INVALID_ARGUMENT, or
// GULON_ERR_UNSUPPORTED for a limit); returns the number of terms and, in *emax, the largest E of the batch.
int check_cosmul_host(const int32_t *off, const int32_t *rows, const float *w, int b, int n, int k_nn, int *emax);

// Rows [from, until) of `ds` scored against the expressions (device CSR lists) and the first k_nn that are no term rows
// written to out_idx / out_score [b][k_nn] and out_count [b] (nullable), all on `st`.  *d_err (nullable) is set when
// an expression is unusable: no term, more than COSMUL_MAX_TERMS, no positive term, k_nn + E > GULON_MAX_K, a row
// outside the dataset; such an expression gets count 0 and padding.
void launch_cosmul_exact(const gulon_dataset *ds, int from, int until, CosmulWork &x, const int *d_off, const int *d_rows,
                         const float *d_w, int b, int k_nn, bool normalize, int *out_idx, float *out_score,
                         int *out_count, int *d_err, hipStream_t st);

// The same over rows [from, until) of a flat byte-code index; called with x.mu held and the handle's mutex free.
// lds_terms: the most terms a question's tables are given LDS for (the host forms: the largest E of the batch).
// dev_rows: an unusable expression sets the index's row-error word.
void launch_cosmul_flat(gulon_index *ix, CosmulWork &x, const int *d_off, const int *d_rows, const float *d_w, int b,
                        int k_nn, bool normalize, int from, int until, int lds_terms, int *out_idx, float *out_score,
                        int *out_count, bool dev_rows, hipStream_t st);
int cosmul_flat_max_terms(const gulon_index *ix);   // the E whose tables fit TABLE_LDS_BUDGET, at most COSMUL_MAX_TERMS

// The launch geometry of the two launchers, which take it from here: the questions of one pass, and for a pass whose
// first question has b questions from it on (a pass takes the first per_pass of them) the row chunks and what one chunk
// holds -- 256-row groups on the exact index, 64-row code blocks on the flat one.  b >= 1.
struct CosmulShape { int per_pass, nchunks, per_chunk; };
CosmulShape cosmul_exact_shape(int from, int until, int b);
CosmulShape cosmul_flat_shape(const gulon_index *ix, int from, int until, int b);

}  // namespace gulon
