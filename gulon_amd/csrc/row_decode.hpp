// Reading stored rows back out of a device-resident PQIndex: the one place that knows the code layouts on the read
// side (DESIGN.md "Row reading").  Used by the row decode (decode.hip), the expression composition (compose.hip), the
// diagnostics (inspect.hip) and the fine codes (fine.hip).  The layouts are the ones the handle keeps (scan.hip /
// wide.hip):
//   byte codes (widths 0/2/4/8): codes[(((i >> 6) * ng + j / vec) * 64 + (i & 63)) * vec + j % vec]
//   wide codes (10/12/16):       wcodes[((i >> 6) * m + j) * 64 + (i & 63)]
// Three readers, by access pattern: CodeSrc::code (one code, anywhere), RowCodes (one row, j ascending, the code word
// kept in registers) and StagedCodes (one 64-row block copied to LDS).  None of them clamps: a reader of rows that may
// hold a code at or above k (no code of this code book) says so itself -- RowWalk's `top`.
#pragma once

#include <type_traits>

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

// the code words RowCodes and the histogram read whole: 16 or 4 bytes, or the wide layout
inline void require_code_layout(const gulon_index *ix) {
  GULON_REQUIRE(ix->vec == 4 || ix->vec == 16 || ix->wide, "unexpected code word of %d bytes", ix->vec);
}

// Two run-time flags as template arguments: f(std::bool_constant<a>, std::bool_constant<b>) -- the WIDE x VEC4 (or
// WIDE x IN_LDS) choice of a kernel instantiation, written once
template <class F>
void dispatch_flags(bool a, bool b, F f) {
  if (a) { if (b) f(std::true_type{}, std::true_type{}); else f(std::true_type{}, std::false_type{}); }
  else { if (b) f(std::false_type{}, std::true_type{}); else f(std::false_type{}, std::false_type{}); }
}

// One stored row's codes, walked j ascending by one lane: the code word that holds quantizer j is fetched when the
// walk enters it (16 or 4 bytes of the byte layouts, one 16-bit code of the wide one) and kept in registers.  Where j
// is wave-uniform the fetches are too.
struct RowCodes {
  CodeSrc src;
  size_t blk;      // row >> 6
  int sub;         // row & 63
  int gi = -1;
  uint4 w = {0u, 0u, 0u, 0u};
  __device__ RowCodes(const CodeSrc &s, int row) : src(s), blk((size_t)(row >> 6)), sub(row & 63) {}
  __device__ int code(int j) {
    if (src.wcodes) return src.wcodes[(blk * src.m + j) * 64 + sub];
    if (src.vec == 16) {
      const int g = j >> 4;
      if (g != gi) { w = reinterpret_cast<const uint4 *>(src.codes)[(blk * src.ng + g) * 64 + sub]; gi = g; }
      return (int)code_byte<16>(w, j & 15);
    }
    const int g = j >> 2;
    if (g != gi) { w.x = reinterpret_cast<const uint32_t *>(src.codes)[(blk * src.ng + g) * 64 + sub]; gi = g; }
    return (int)code_byte<4>(w.x, j & 3);
  }
};

// One 64-row block's codes staged in LDS: byte layout [ng][64][vec] bytes, wide [m][64] uint16 -- both contiguous per
// block and multiples of 16 bytes, so the copy is 16-byte loads.  lds: block_code_bytes(ix) bytes, 16-byte aligned.
inline size_t block_code_bytes(const gulon_index *ix) {
  return ix->wide ? (size_t)ix->m * 128 : (size_t)ix->ng * 64 * ix->vec;
}

template <bool WIDE>
struct StagedCodes {
  uint8_t *lds;
  int vec;
  // cooperative: all `threads` threads of the workgroup, and a barrier before the first code()
  __device__ __forceinline__ void stage(const CodeSrc &src, int block, int tid, int threads) const {
    const int chunk = WIDE ? src.m * 128 : src.ng * 64 * src.vec;
    const uint4 *g = WIDE ? (const uint4 *)(src.wcodes + (size_t)block * src.m * 64)
                          : (const uint4 *)(src.codes + (size_t)block * chunk);
    for (int t = tid; t < chunk / 16; t += threads) ((uint4 *)lds)[t] = g[t];
  }
  __device__ int code(int l, int j) const {       // row l (0..63) of the block
    if (WIDE) return ((const uint16_t *)lds)[j * 64 + l];
    return lds[(j / vec) * 64 * vec + l * vec + j % vec];
  }
};

// one row of a staged block, as a code source of RowWalk
template <bool WIDE>
struct StagedRow {
  StagedCodes<WIDE> block;
  int l;
  __device__ int code(int j) const { return block.code(l, j); }
};

// One decoded row, walked e ascending: value(e) = the row's code-book coordinate e.  The entry of the quantizer that
// holds e is looked up when the walk enters it.  Every quantizer has a coordinate (every index is made with m <= d), so
// the walk enters at most one quantizer per coordinate.  Codes: RowCodes or StagedRow.  top: the largest code let
// through -- k - 1 makes a code at or above k read as the code book's last entry: nothing outside it is touched.
// A caller that has something to do at a quantizer's end takes the steps of value() itself: if (behind(e)) { ...;
// enter_next(); }, then at(e).  Taken with the same e by all lanes of a wave the steps are wave-uniform, so that work
// may reduce across lanes (row_errors_kernel).
template <class Codes>
struct RowWalk {
  Codes codes;
  SubvectorMap sv;
  const float *cents, *cj = nullptr;
  int k, top, j = -1, jfrom = 0, jend = 0;
  __device__ RowWalk(const Codes &codes_, const float *cents_, int d, int m, int k_, int top_)
      : codes(codes_), sv(d, m), cents(cents_), k(k_), top(top_) {}
  __device__ bool behind(int e) const { return e >= jend; }   // e lies beyond quantizer j
  __device__ void enter_next() {
    j++;
    jfrom = jend;
    jend += sv.sdim(j);
    cj = cents + (size_t)k * jfrom + (size_t)min(codes.code(j), top) * sv.sdim(j);
  }
  __device__ float at(int e) const { return cj[e - jfrom]; }   // once !behind(e)
  __device__ float value(int e) {
    if (behind(e)) enter_next();
    return at(e);
  }
};

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

// A grouped index's row is centroid(c) + decode(row), one fp32 add per coordinate (MathUtils.add, the centroid first).
// There are two rules for c, on purpose:
//   lookup_base     GroupedIndex.lookup's partition (Index.scala:247-253): Arrays.binarySearch over the raw offsets.
//                   It is the reference's answer for `lookup`, and decode.hip / compose.hip reproduce it.
//   group_centroid  the group whose range [bounds[c], bounds[c + 1]) holds the row -- the group a query scans the row
//                   in, hence the centroid its distances are computed with.  Where offsets repeat (empty groups) the
//                   binarySearch rule can name another group, whose centroid no query ever pairs with the row; so
//                   whatever measures or refines the index's distances (inspect.hip, fine.hip) uses this rule.
__device__ inline const float *lookup_base(const float *__restrict__ gcent, const int *__restrict__ offsets,
                                           int n_offsets, int row, int d) {
  const int i = java_binary_search(offsets, n_offsets, row);
  return gcent + (size_t)(i < 0 ? -i - 1 : i + 1) * d;
}

struct GroupBase { const float *gcent; const int *bounds; int g; };   // gcent == nullptr: a flat index
const GroupBase FLAT{nullptr, nullptr, 0};
inline GroupBase group_base(const GroupedParts &gp) { return {gp.gcent, gp.bounds, gp.g}; }

// What an exported call resolves its handle to: the PQ index whose rows are read, the lock of the handle the caller was
// given, and the groups
struct IndexRef { gulon_index *ix; std::mutex *mu; GroupBase gb; };
inline IndexRef index_ref(gulon_index *idx) {
  GULON_REQUIRE(idx != nullptr, "index is null");
  return {idx, &idx->mu, FLAT};
}
inline IndexRef index_ref(gulon_grouped_index *idx) {
  GULON_REQUIRE(idx != nullptr, "index is null");
  const GroupedParts gp = grouped_parts(idx);
  return {gp.pq, gp.mu, group_base(gp)};
}

__device__ inline const float *group_centroid(const GroupBase &gb, int row, int d) {
  int lo = 0, hi = gb.g;                          // largest c with bounds[c] <= row
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (gb.bounds[mid] <= row) lo = mid; else hi = mid; }
  return gb.gcent + (size_t)lo * d;
}

// Coordinate e of row `row`: a copy of a codebook entry, plus base[e] (one fp32 add) for the grouped lookup
__device__ inline float decoded_coordinate(const CodeSrc &src, const SubvectorMap &sv, const float *__restrict__ cents,
                                           int k, int row, int e, const float *__restrict__ base) {
  const int j = sv.quantizer(e), fr = sv.from(j), sj = sv.sdim(j);
  const float c = cents[(size_t)k * fr + (size_t)src.code(row, j) * sj + (e - fr)];
  return base ? base[e] + c : c;
}

}  // namespace gulon
