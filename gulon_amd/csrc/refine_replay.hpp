// The candidate replay that refine.hip and fine.hip share: a query's distances, already in LDS, offered to the
// reference's TopKHeap (topk_heap.hpp) in candidate order by one wavefront.
#pragma once

#include "topk_heap.hpp"

namespace gulon {

// The replay is not c serial updates.  update(key, x) on a FULL heap does nothing unless root > x, so a candidate can be
// left out as soon as `root > x` is known to be false AT THE MOMENT THE REFERENCE WOULD INSPECT IT.  While the heap
// holds no NaN it is a max-heap in the ordinary sense: its root is its largest value, and an effective update replaces
// that by something smaller, so the root never increases -- a candidate that fails `root > x` against the root of NOW
// fails it against every later root too.  The wave therefore ballots 64 candidates at a time against the current root
// and runs update only for the set bits, lowest position first, asking again after every update (the root fell: more
// bits may clear).  The updates that run are the reference's effective ones in its order, those left out are no-ops:
// the same heap arrangement.  +-inf are ordinary values here, and a NaN candidate fails `root > NaN` like any no-op.
// A NaN INSIDE the heap (it can only get in while the heap fills) ends the argument: comparisons with it are false, so
// percolateUp stops below it and a value larger than the root can sit under it; delete moves the last slot to the
// root, which can then RISE.  From the first NaN taken in, every candidate goes through update itself, one by one,
// which makes the reference's own test at the reference's own moment.
template <class Heap>
__device__ void refine_replay(Heap &h, const int *__restrict__ qcand, const float *sd, int c, int lane) {
  bool nan_inside = false;
  for (int base = 0; base < c; base += 64) {
    const int p = base + lane;
    const int id = p < c ? qcand[p] : -1;
    const float x = p < c ? sd[p] : 0.f;
    unsigned long long pend = __ballot(id >= 0);           // a negative candidate is padding: never offered
    while (pend) {
      if (h.size == h.cap && !nan_inside) {
        pend &= __ballot(h.val(0) > x);
        if (!pend) break;
      }
      const int j = __builtin_amdgcn_readfirstlane(__ffsll((long long)pend) - 1);
      pend &= pend - 1;
      const float xj = readlane_f(x, j);
      if (h.size < h.cap && xj != xj) nan_inside = true;
      h.update(readlane_i(id, j), xj);
    }
  }
}

}  // namespace gulon
