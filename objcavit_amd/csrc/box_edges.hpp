// Which pixels a detection box owns, shared by csrc/object_depth.hip and csrc/object_metrics.hip (the rule is stated in
// include/objcavit_hip.h at ocv_object_depth_fwd; the tests' statement is tests/object_depth_ref.py).
#pragma once

#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>

// [lo, hi) of the pixels whose centre lies in [c - half * size, c + half * size): every statement rounded to fp32 on its own (the
// library is built with contraction on: a fused half * size would move an edge by a pixel against the plain statement)
__device__ __forceinline__ bool od_edges(float c, float size, float half, int limit, int& lo, int& hi) {
  const float hs = __fmul_rn(half, size);
  float a = ceilf(__fsub_rn(__fsub_rn(c, hs), 0.5f));
  float b = ceilf(__fsub_rn(__fadd_rn(c, hs), 0.5f));
  if (!(fabsf(a) <= FLT_MAX) || !(fabsf(b) <= FLT_MAX)) return false;      // NaN or inf
  a = fminf(fmaxf(a, 0.f), (float)limit);
  b = fminf(fmaxf(b, 0.f), (float)limit);
  lo = (int)a;
  hi = (int)b;
  return hi > lo;
}
