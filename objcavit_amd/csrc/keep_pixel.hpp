// The per-pixel KEEP rule of the outputs that read the final map point by point: the point cloud (csrc/point_cloud.hip) and the ground grid
// (csrc/ground_grid.hip).  One statement, included by both, so the two cannot drift apart (include/objcavit_hip.h, ocv_depth_unproject_fwd):
//   the image's camera is usable (fx, fy finite and > 0, cx, cy finite), and
//   z is finite with near <= z <= far, confidence >= min_confidence and depth_std <= max_std where those maps are given (NaN fails both).
#pragma once
#include <hip/hip_runtime.h>

#include <float.h>

__device__ __forceinline__ bool up_finite(float v) { return fabsf(v) <= FLT_MAX; }

// k = fx, fy, cx, cy
__device__ __forceinline__ bool up_camera_ok(const float4 k) {
  return up_finite(k.x) && k.x > 0.f && up_finite(k.y) && k.y > 0.f && up_finite(k.z) && up_finite(k.w);
}

// in: the candidate exists (inside the strided grid, usable camera); cf / sd are read only where their map is given
__device__ __forceinline__ bool up_keep(bool in, float z, float cf, float sd, bool has_conf, bool has_std, float near, float far,
                                        float min_conf, float max_std) {
  bool on = in && up_finite(z) && near <= z && z <= far;
  if (has_conf) on = on && cf >= min_conf;                                   // (NaN fails both)
  if (has_std) on = on && sd <= max_std;
  return on;
}
