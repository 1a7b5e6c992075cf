// Analogy accuracy, the per-batch part: where the expected row of every question stands in its answer
// list, and the per-section counters of the questions asked and of those answered within each k of the caller's list.
// One wavefront per question: the lanes read 64 entries of the list per step, a ballot finds the first match, lane 0
// adds to the integer counters.  Integer atomics only, so the counters do not depend on the order of the questions.
#include "common.hpp"

namespace gulon {

constexpr int AC_MAX_KS = 16;

namespace {

// idx_lists [b][kin] with counts[q] live entries; expected[q] >= 0, so the -1 padding of a list never matches.
// hits [nsections][nks] and asked [nsections] accumulate; a section outside [0, nsections) counts nowhere.
__global__ __launch_bounds__(64) void analogy_counts_kernel(const int *__restrict__ idx_lists,
                                                            const int *__restrict__ counts, int kin,
                                                            const int *__restrict__ expected,
                                                            const int *__restrict__ section, const int *__restrict__ ks,
                                                            int nks, int nsections, int *__restrict__ hits,
                                                            int *__restrict__ asked, int *__restrict__ out_rank) {
  const int q = blockIdx.x, lane = threadIdx.x;
  const int live = min(max(counts[q], 0), kin);
  const int want = expected[q];
  const int *ii = idx_lists + (size_t)q * kin;
  int rank = -1;
  for (int c0 = 0; c0 < live && rank < 0; c0 += 64) {
    const int p = c0 + lane;
    const unsigned long long mask = __ballot(want >= 0 && p < live && ii[p] == want);
    if (mask) rank = c0 + __ffsll((long long)mask) - 1;
  }
  if (lane != 0) return;
  if (out_rank) out_rank[q] = rank;
  const int s = section[q];
  if (s < 0 || s >= nsections) return;
  atomicAdd(&asked[s], 1);
  for (int j = 0; j < nks; j++)
    if (rank >= 0 && rank < ks[j]) atomicAdd(&hits[(size_t)s * nks + j], 1);
}

void check_shape(int b, int kin, int nks, int nsections) {
  GULON_REQUIRE(b >= 0 && kin >= 0 && nks >= 0 && nks <= AC_MAX_KS && nsections >= 0,
                "bad arguments b=%d kin=%d nks=%d (<= %d) nsections=%d", b, kin, nks, AC_MAX_KS, nsections);
}

void launch_counts(const int *idx_lists, const int *counts, int b, int kin, const int *expected, const int *section,
                   const int *ks, int nks, int nsections, int *hits, int *asked, int *out_rank, hipStream_t st) {
  if (b == 0) return;
  GULON_REQUIRE(counts && expected && section && asked && (idx_lists || kin == 0) && (nks == 0 || (ks && hits)),
                "null argument");
  hipLaunchKernelGGL(analogy_counts_kernel, dim3(b), dim3(64), 0, st, idx_lists, counts, kin, expected, section, ks, nks,
                     nsections, hits, asked, out_rank);
  HIP_CHECK(hipGetLastError());
}

}  // namespace
}  // namespace gulon

using namespace gulon;

GULON_API int32_t gulon_analogy_counts_dev(const int32_t *d_idx_lists, const int32_t *d_counts, int32_t b, int32_t kin,
                                           const int32_t *d_expected, const int32_t *d_section, const int32_t *d_ks,
                                           int32_t nks, int32_t nsections, int32_t *d_hits, int32_t *d_asked,
                                           int32_t *d_out_rank, void *stream) {
  return guarded([&] {
    check_shape(b, kin, nks, nsections);
    launch_counts(d_idx_lists, d_counts, b, kin, d_expected, d_section, d_ks, nks, nsections, d_hits, d_asked,
                  d_out_rank, (hipStream_t)stream);
  });
}

GULON_API int32_t gulon_analogy_counts(const int32_t *idx_lists, const int32_t *counts, int32_t b, int32_t kin,
                                       const int32_t *expected, const int32_t *section, const int32_t *ks, int32_t nks,
                                       int32_t nsections, int32_t *hits, int32_t *asked, int32_t *out_rank) {
  return guarded([&] {
    check_shape(b, kin, nks, nsections);
    GULON_REQUIRE(nks == 0 || ks != nullptr, "ks is null");
    for (int j = 0; j < nks; j++)
      GULON_REQUIRE(ks[j] >= 1 && ks[j] <= kin && (j == 0 || ks[j] > ks[j - 1]),
                    "ks must ascend within [1, kin = %d]: ks[%d] = %d", kin, j, ks[j]);
    if (b == 0) return;
    GULON_REQUIRE(counts && expected && section && asked && (idx_lists || kin == 0) && (nks == 0 || hits),
                  "null argument");
    for (int q = 0; q < b; q++) {
      GULON_REQUIRE(section[q] >= 0 && section[q] < nsections, "section[%d] = %d outside [0, %d)", q, section[q],
                    nsections);
      GULON_REQUIRE(expected[q] >= 0, "expected[%d] = %d is negative", q, expected[q]);
    }
    const size_t bk = (size_t)b * kin, nh = (size_t)nsections * nks;
    DevBuf<int> dl, dc, de, ds, dks, dh, da, dr(out_rank ? (size_t)b : 0);
    dl.upload(idx_lists, bk);
    dc.upload(counts, (size_t)b);
    de.upload(expected, (size_t)b);
    ds.upload(section, (size_t)b);
    dks.upload(ks, (size_t)nks);
    dh.upload(hits, nh);
    da.upload(asked, (size_t)nsections);
    launch_counts(dl.p, dc.p, b, kin, de.p, ds.p, dks.p, nks, nsections, dh.p, da.p, dr.p, nullptr);
    dh.download(hits, nh);
    da.download(asked, (size_t)nsections);
    if (out_rank) dr.download(out_rank, (size_t)b);
    HIP_CHECK(hipStreamSynchronize(nullptr));
  });
}
