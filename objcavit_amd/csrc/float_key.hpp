// Order-preserving image of a float in the unsigned integers (a < b  <=>  key(a) < key(b), -0 below +0), so that a float extreme can be
// joined by an unsigned integer atomic max: csrc/ground_grid.hip (a cell's heights) and csrc/obstacles.hip (a component's h_max).  The key
// of every float is above 0, so an all-zero record means "nothing joined yet".
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ unsigned gg_key(float v) {
  const unsigned u = __float_as_uint(v);
  return (u >> 31) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float gg_unkey(unsigned k) { return __uint_as_float((k >> 31) ? (k & 0x7fffffffu) : ~k); }
