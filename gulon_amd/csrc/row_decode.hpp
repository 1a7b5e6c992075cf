// Reading one stored row back out of a device-resident PQIndex -- shared by the row decode (decode.hip) and the
// expression composition (compose.hip).  Codes are read in the layout the handle keeps (scan.hip / wide.hip):
//   byte codes (widths 0/2/4/8): codes[(((i >> 6) * ng + j / vec) * 64 + (i & 63)) * vec + j % vec]
//   wide codes (10/12/16):       wcodes[((i >> 6) * m + j) * 64 + (i & 63)]
#pragma once

#include "scan.hpp"

namespace gulon {

// Vectors.subvectors (Vectors.scala:84-104) inverted: the quantizer that coordinate e belongs to.  The first `full`
// quantizers are `ideal` wide, the rest ideal - 1 (common.hpp subvectors, from which ix->from / ix->sdim are made).
struct SubvectorMap {
  int ideal, full;
  __host__ __device__ SubvectorMap(int d, int m) : ideal((d + m - 1) / m), full(m - ((d + m - 1) / m * m - d)) {}
  __device__ int quantizer(int e) const {
    const int split = full * ideal;
    return e < split ? e / ideal : full + (e - split) / (ideal - 1);
  }
  __device__ int from(int j) const { return j < full ? j * ideal : full * ideal + (j - full) * (ideal - 1); }
  __device__ int sdim(int j) const { return j < full ? ideal : ideal - 1; }
};

struct CodeSrc {
  const uint8_t *codes;     // byte layout (nullptr when wide)
  const uint16_t *wcodes;   // wide layout
  int ng, vec, m;
  __device__ int code(long long i, int j) const {
    if (wcodes) return wcodes[((size_t)(i >> 6) * m + j) * 64 + (i & 63)];
    return codes[(((size_t)(i >> 6) * ng + j / vec) * 64 + (i & 63)) * vec + j % vec];
  }
};

inline CodeSrc code_src(const gulon_index *ix) {
  CodeSrc s;
  s.codes = ix->wide ? nullptr : ix->codes.p;
  s.wcodes = ix->wide ? ix->wcodes.p : nullptr;
  s.ng = ix->ng; s.vec = ix->vec; s.m = ix->m;
  return s;
}

// java.util.Arrays.binarySearch(int[] a, int key), restated literally (an empty group repeats an offset: the
// search may land on any of the equal entries, which is what the reference's lookup then uses).
__device__ inline int java_binary_search(const int *__restrict__ a, int len, int key) {
  int low = 0, high = len - 1;
  while (low <= high) {
    const int mid = (int)((unsigned)(low + high) >> 1);
    const int v = a[mid];
    if (v < key) low = mid + 1;
    else if (v > key) high = mid - 1;
    else return mid;
  }
  return -(low + 1);
}

// GroupedIndex.lookup's partition of a row (Index.scala:247-253): the centroid the reference adds to its decode
__device__ inline const float *lookup_base(const float *__restrict__ gcent, const int *__restrict__ offsets,
                                           int n_offsets, int row, int d) {
  const int i = java_binary_search(offsets, n_offsets, row);
  return gcent + (size_t)(i < 0 ? -i - 1 : i + 1) * d;
}

// Coordinate e of row `row`: a copy of a codebook entry, plus base[e] (one fp32 add) for the grouped lookup
__device__ inline float decoded_coordinate(const CodeSrc &src, const SubvectorMap &sv, const float *__restrict__ cents,
                                           int k, int row, int e, const float *__restrict__ base) {
  const int j = sv.quantizer(e), fr = sv.from(j), sj = sv.sdim(j);
  const float c = cents[(size_t)k * fr + (size_t)src.code(row, j) * sj + (e - fr)];
  return base ? base[e] + c : c;
}

}  // namespace gulon
