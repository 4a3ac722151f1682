// Runs of consecutive lanes of a wave that carry the same key, and the segmented reduction over them: the on-chip merge in front of the
// LDS tables of csrc/ground_grid.hip (key = the point's cell) and csrc/obstacles.hip (key = the cell's root).  One definition, included by
// both.  One ballot of the run heads, then six steps; in every step EVERY lane shuffles its values down by o (the caller's `step`, which
// owns the values and their joins) and a lane takes what arrives iff lane + o still belongs to its own run.  After the last step the
// first lane of a run holds the join of the whole run; the other lanes hold joins of their run's tails, which nobody reads.
#pragma once
#include "common.hpp"

struct SegRuns {
  bool head;                                               // this lane starts a run
  unsigned long long above;                                // bit j: lane + 1 + j starts a run
};

__device__ __forceinline__ SegRuns seg_runs(int key, int lane) {
  const int before = __shfl_up(key, 1, OCV_WAVE);
  SegRuns r;
  r.head = lane == 0 || before != key;
  const unsigned long long heads = __ballot(r.head);
  r.above = lane == OCV_WAVE - 1 ? 0ull : heads >> (lane + 1);
  return r;
}

// step(o, take): shuffle every value down by o (all lanes), join what arrived iff `take`
template <class Step>
__device__ __forceinline__ void seg_reduce(const SegRuns& r, int lane, Step&& step) {
#pragma unroll
  for (int o = 1; o < OCV_WAVE; o <<= 1) step(o, lane + o < OCV_WAVE && (r.above & ((1ull << o) - 1ull)) == 0ull);
}
