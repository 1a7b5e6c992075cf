// What the exact index (exact.hip) shares with the brute-force kNN (knn.hip): the shape of its row tile and the two
// kernels of the single-pass / peeled path, which exact.hip launches for small k_nn and as its fallback.
#pragma once
#include "scan.hpp"

namespace gulon {

constexpr int KNN_QT = 16;       // queries per workgroup
constexpr int KNN_DT = 32;       // dims staged per step
constexpr int KNN_THREADS = 256; // 4 waves, lane = row

// Qt[tile][t][KNN_QT]: queries transposed so one uniform (scalar) load serves a wave
__global__ void transpose_queries(const float *__restrict__ Q, int B, int d, int ntiles, float *__restrict__ Qt);
// knn.hip: the keff smallest (distance, row id) of every chunk of [row_from, row_until) per query, after (lbv, lbi)
__global__ __launch_bounds__(KNN_THREADS) void knn_kernel(const float *__restrict__ X, int n, int d,
                                                          const float *__restrict__ Qt, int row_from, int row_until,
                                                          int rows_per_chunk, int nchunks, int keff,
                                                          float *__restrict__ part_v, int *__restrict__ part_i,
                                                          const float *__restrict__ lbv, const int *__restrict__ lbi);

}  // namespace gulon
