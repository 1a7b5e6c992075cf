// MathUtils.normalize (MathUtils.scala:100-120) of one row staged in LDS -- shared by the row decode (decode.hip) and
// the word2vec ingest (ingest.hip).
#pragma once

#include "common.hpp"

namespace gulon {

// xs[0, d): the row, visible to every calling lane (the caller has synchronised).  MathUtils.distance(xs): sequential
// fp32 sum of x * x in coordinate order (every lane computes it; the LDS reads are broadcasts), math.sqrt in double,
// .toFloat; then one division per coordinate, lane `lane` of `lanes` writing o[lane], o[lane + lanes], ...
__device__ __forceinline__ void normalize_staged_row(const float *xs, int d, int lane, int lanes, float *o) {
  float sum = 0.f;
  for (int e = 0; e < d; e++) { const float x = xs[e]; sum += x * x; }
  const float dist = (float)__dsqrt_rn((double)sum);
  for (int e = lane; e < d; e += lanes) o[e] = __fdiv_rn(xs[e], dist);
}

}  // namespace gulon
