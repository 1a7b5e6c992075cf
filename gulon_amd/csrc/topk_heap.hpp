// The reference's TopKHeap (TopKHeap.scala:3-94) on one wavefront: every answer under ties or non-finite distances
// follows its rules -- strict `>` in update, the left child preferred in percolateDown, delete moving the last slot
// to the root, Result.fromHeap / deleteAll filling from the back.  All members are called by the whole wave with
// wave-uniform arguments.
#pragma once

#include "common.hpp"

namespace gulon {

// TopKHeap.scala with lane = slot storage (cap <= GULON_MAX_K = 63); every index is wave-uniform.
// The reference's chains of swaps move ONE entry down (or up) the tree; here that entry travels in registers and the
// entries it passes are shifted into the hole it leaves: three lane reads per level instead of eight (a batch's group
// selection with LimitGroups(50) over 1001 groups is ~200 serial updates per query on one wavefront: 234 us of a
// 0.51 ms batch with the swaps).  This hole form and down_root are still the reference's heap: they make the same
// comparisons in the same order -- also with NaN, where every comparison is false in both forms -- and so reach the
// same final arrangement.
struct RegHeap {
  float v = 0.f;
  int k = 0;
  int size = 0;
  int cap;
  int lane;
  __device__ RegHeap(int cap_, int lane_) : cap(cap_), lane(lane_) {}
  __device__ float val(int i) const { return readlane_f(v, i); }
  __device__ int key(int i) const { return readlane_i(k, i); }
  // percolateDown (TopKHeap.scala:30-42) from the ROOT with every lane working: lane l looks at its own two children
  // and decides where an entry of value `cur` standing at slot l would go next (the reference's two comparisons, in its
  // order); the path from the root is then a chase through those answers -- one lane read per level -- and every slot
  // on the path takes its chosen child's entry at once.
  __device__ void down_root(float cur, int curk) {
    const int lc = 2 * lane + 1, rc = 2 * lane + 2;
    const float a0 = __int_as_float(__builtin_amdgcn_ds_bpermute(4 * (lc & 63), __float_as_int(v)));
    const float b0 = __int_as_float(__builtin_amdgcn_ds_bpermute(4 * (rc & 63), __float_as_int(v)));
    const bool ha = lc < size, hb = rc < size;
    // top = l; if (lc < size && val(top) < val(lc)) top = lc; if (rc < size && val(top) < val(rc)) top = rc;
    int nxt = -1;
    float nv = cur;
    if (ha && nv < a0) { nv = a0; nxt = lc; }
    if (hb && nv < b0) { nv = b0; nxt = rc; }
    const int kc = __builtin_amdgcn_ds_bpermute(4 * (max(nxt, 0) & 63), k);
    unsigned long long path = 0ull;
    int node = 0;
    for (;;) {
      const int n2 = readlane_i(nxt, node);
      if (n2 < 0) break;
      path |= 1ull << node;
      node = n2;
    }
    if ((path >> lane) & 1ull) { v = nv; k = kc; }
    if (lane == node) { v = cur; k = curk; }
  }
  __device__ void del() {                                   // delete, TopKHeap.scala:57-67 (drain reads the root)
    size -= 1;
    down_root(val(size), key(size));
  }
  __device__ bool would_insert(float x) const { return size < cap || val(0) > x; }
  __device__ void update(int kk, float x) {                 // update, TopKHeap.scala:69-79
    if (size == cap && val(0) > x) del();
    if (size < cap) {
      int i = size;
      while (i > 0) {                                       // percolateUp, TopKHeap.scala:21-28
        const int p = (i - 1) / 2;
        const float pv = val(p);
        if (x > pv) {
          const int pk = key(p);
          if (lane == i) { v = pv; k = pk; }
          i = p;
        } else break;
      }
      if (lane == i) { v = x; k = kk; }
      size += 1;
    }
  }
  // Result.fromHeap (Index.scala:83-94) and deleteAll (TopKHeap.scala:81-89): the root, then delete, filling slot i
  // from the back; put(i, key, value) runs after the delete, when slot i is outside the heap
  template <class Put>
  __device__ void drain(Put put) {
    for (int i = size - 1; i >= 0; i--) {
      const int kk = key(0);
      const float x = val(0);
      del();
      put(i, kk, x);
    }
  }
};

// TopKHeap.scala with the arrays in LDS (one heap per wave), for heaps of more than 63 slots: k_nn > 63 (a fallback:
// Tests.scala asks for up to 1000 neighbours, the benchmarks for 10) and gq_literal_groups' selection of groups.
// Every lane runs the same wave-uniform code and reads the same entries; lane 0 stores.  (LDS operations of a wave
// execute in order.)
struct LdsHeap {
  volatile float *hv;
  volatile int *hk;
  int size = 0;
  int cap;
  int lane;
  __device__ LdsHeap(float *v_, int *k_, int cap_, int lane_) : hv(v_), hk(k_), cap(cap_), lane(lane_) {}
  __device__ float val(int i) const { return hv[i]; }
  __device__ int key(int i) const { return hk[i]; }
  __device__ void put(int i, int kk, float x) { if (lane == 0) { hv[i] = x; hk[i] = kk; } }
  __device__ void swp(int a, int b) {
    const float va = val(a), vb = val(b);
    const int ka = key(a), kb = key(b);
    put(a, kb, vb);
    put(b, ka, va);
  }
  __device__ void down(int i) {                             // percolateDown, TopKHeap.scala:30-42
    for (;;) {
      int top = i;
      const int lc = 2 * i + 1, rc = 2 * i + 2;
      if (lc < size && val(top) < val(lc)) top = lc;
      if (rc < size && val(top) < val(rc)) top = rc;
      if (top == i) break;
      swp(i, top);
      i = top;
    }
  }
  __device__ void del() {                                   // delete, TopKHeap.scala:57-67 (drain reads the root)
    size -= 1;
    put(0, key(size), val(size));
    down(0);
  }
  __device__ bool would_insert(float x) const { return size < cap || val(0) > x; }
  __device__ void update(int kk, float x) {                 // update, TopKHeap.scala:69-79
    if (size == cap && val(0) > x) del();
    if (size < cap) {
      put(size, kk, x);
      int i = size;
      while (i > 0) {                                       // percolateUp, TopKHeap.scala:21-28
        const int p = (i - 1) / 2;
        if (val(i) > val(p)) { swp(i, p); i = p; } else break;
      }
      size += 1;
    }
  }
  template <class Put>                                      // Result.fromHeap / deleteAll, as RegHeap::drain
  __device__ void drain(Put put) {
    for (int i = size - 1; i >= 0; i--) {
      const int kk = key(0);
      const float x = val(0);
      del();
      put(i, kk, x);
    }
  }
};

}  // namespace gulon
