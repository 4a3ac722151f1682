// Union-find by smaller index, for the connected components of csrc/obstacles.hip (Statement O of include/objcavit_hip.h).  One
// definition for the device -- on an LDS array (a tile's local indices) and on a global one (an image's linear cell indices), with
// concurrent callers -- and for plain host C++ (tests/test_obstacles_host.py builds a stand-alone driver around it and runs it under
// the address and undefined-behaviour sanitizers).
//
// THE INVARIANT: parent[i] <= i for every i, and a stored parent only ever DECREASES (the one store is a min).  So
//   uf_find   follows strictly decreasing indices and ends after at most i steps, whatever other callers do meanwhile;
//   uf_union  replaces one of its two indices by a strictly smaller one in every round (a root found below it, or the parent another
//             caller stored first), so the pair's sum decreases and it ends after at most a + b rounds.
// No loop here waits for another caller.  The larger root is always hung under the smaller, so when every union is done the root of a
// component is its smallest index.  A union that loses the race for a root (the min found somebody else's smaller parent there) has
// lowered that root's parent to min(theirs, ours) and goes on to join theirs with ours, so no link is ever lost.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define OCV_UF_FN __host__ __device__ inline
#else
#define OCV_UF_FN inline
#endif

// parent[i], read so that a concurrent store of another caller is seen on the next read (no stale register copy)
OCV_UF_FN int uf_load(const int* parent, int i) { return __atomic_load_n(parent + i, __ATOMIC_RELAXED); }

// parent[i] = min(parent[i], v) in one step; -> what was there
OCV_UF_FN int uf_store_min(int* parent, int i, int v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return atomicMin(parent + i, v);
#else
  const int old = parent[i];
  if (v < old) parent[i] = v;
  return old;
#endif
}

OCV_UF_FN int uf_find(const int* parent, int i) {
  for (int p = uf_load(parent, i); p >= 0 && p < i; p = uf_load(parent, i)) i = p;      // i strictly decreases and stays >= 0
  return i;
}

OCV_UF_FN void uf_union(int* parent, int a, int b) {
  for (;;) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }          // a: the larger root, to hang under b
    const int old = uf_store_min(parent, a, b);
    if (old == a) return;                                   // a was still a root: done
    a = old;                                                // another caller hung a under old < a first: join old with b
  }
}
