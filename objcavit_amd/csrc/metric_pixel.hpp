// The per-pixel statement of the validation metrics, shared by csrc/metrics.hip (one record per image) and csrc/object_metrics.hip
// (one record per detection box / per region): what the reference does to ONE pixel between the model output and its eight numbers --
//   clamp that keeps NaN, un-mirrored average with the mirrored forward          modules/GraphBinsLM.py:159-181
//   the ATen align_corners = True bilinear taps (identity at equal sizes),
//   nan -> min_depth, +-inf -> max_depth                                         metrics/MetricsPreprocess.py:14-24
//   the nine terms abs_rel, sq_rel, sq, sq_log, log10, d1, d2, d3, count         metrics/AbsRel.py ... AccThresh.py
// -- and what turns nine sums into a record.  Nothing here knows its caller: which pixels are valid, and where the terms are added,
// is the including kernel's business.
#pragma once

#include <hip/hip_runtime.h>

namespace ocv_metric {

constexpr int NSUM = 9;           // abs_rel, sq_rel, sq, sq_log, log10, d1, d2, d3, count

// the two model outputs' geometry against the ground truth's, and the depth range
struct MapView {
  int h, w, H, W;
  float sh, sw, dmin, dmax;
};

inline MapView map_view(int h, int w, int H, int W, float min_depth, float max_depth) {
  return MapView{h, w, H, W, H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.f, W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.f,
                 min_depth, max_depth};
}

// workgroups per image of a two-stage pass over B maps of P pixels
inline int metric_tiles(int B, long P) {
  long t = (2048 + B - 1) / B;                         // ~2048 workgroups per launch
  const long maxt = (P + 4095) / 4096;                 // at least 16 pixels per thread
  if (t > maxt) t = maxt;
  return (int)(t < 1 ? 1 : t);
}

// torch.clamp semantics: NaN stays NaN (fminf / fmaxf would drop it)
__device__ __forceinline__ float clamp_keep_nan(float v, float lo, float hi) { return v != v ? v : fminf(fmaxf(v, lo), hi); }

__device__ __forceinline__ float tap(const MapView& p, const float* pb, const float* mb, int y, int x) {
  const float a = clamp_keep_nan(pb[y * p.w + x], p.dmin, p.dmax);
  if (mb == nullptr) return a;
  return 0.5f * (a + clamp_keep_nan(mb[y * p.w + (p.w - 1 - x)], p.dmin, p.dmax));
}

// the prediction at ground-truth pixel (Y, X), BEFORE the nan / inf fix: ATen upsample_bilinear2d, align_corners = True
__device__ __forceinline__ float resized(const MapView& p, const float* pb, const float* mb, int Y, int X) {
  const float sy = p.sh * Y, sx = p.sw * X;
  const int ya = (int)sy, xa = (int)sx;
  const int yb = ya + (ya < p.h - 1 ? 1 : 0), xb = xa + (xa < p.w - 1 ? 1 : 0);
  const float h1 = sy - (float)ya, h0 = 1.0f - h1, w1 = sx - (float)xa, w0 = 1.0f - w1;
  // (all four terms always, so a NaN tap reaches its neighbours through a zero weight exactly as in ATen; equal
  // sizes are ATen's identity short-cut, where it does not)
  return (p.h == p.H && p.w == p.W)
             ? tap(p, pb, mb, Y, X)
             : h0 * (w0 * tap(p, pb, mb, ya, xa) + w1 * tap(p, pb, mb, ya, xb)) +
                   h1 * (w0 * tap(p, pb, mb, yb, xa) + w1 * tap(p, pb, mb, yb, xb));
}

// nan_to_num(nan = min, posinf = neginf = max)
__device__ __forceinline__ float fixed(const MapView& p, float v) {
  if (v != v) return p.dmin;
  if (__builtin_isinf(v)) return p.dmax;
  return v;
}

// the nine terms of one valid pixel: ground truth g, fixed prediction v
__device__ __forceinline__ void terms(float g, float v, float t[NSUM]) {
  const float d = g - v, ratio = fmaxf(g / v, v / g);
  const float dl = logf(g) - logf(v);
  t[0] = fabsf(d) / g;
  t[1] = d * d / g;
  t[2] = d * d;
  t[3] = dl * dl;
  t[4] = fabsf(log10f(g) - log10f(v));
  t[5] = ratio < 1.25f ? 1.f : 0.f;
  t[6] = ratio < 1.25f * 1.25f ? 1.f : 0.f;
  t[7] = ratio < 1.25f * 1.25f * 1.25f ? 1.f : 0.f;
  t[8] = 1.f;
}

// nine totals -> r[0 .. 8]: the eight means (the two RMSEs square-rooted) and the count; all zero without a pixel
__device__ __forceinline__ void record(const double tot[NSUM], float* r) {
  const double n = tot[8] > 0.0 ? tot[8] : 1.0;
  r[0] = (float)(tot[0] / n);
  r[1] = (float)(tot[1] / n);
  r[2] = (float)sqrt(tot[2] / n);
  r[3] = (float)sqrt(tot[3] / n);
  r[4] = (float)(tot[4] / n);
  r[5] = (float)(tot[5] / n);
  r[6] = (float)(tot[6] / n);
  r[7] = (float)(tot[7] / n);
  r[8] = (float)tot[8];
}

}  // namespace ocv_metric
