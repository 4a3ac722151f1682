// Depth ERROR per detection box, and over objects against background: the segmented form of the validation
// metrics of csrc/metrics.hip, on the device.
//   pred (+ pred_mirror) [B][1][h][w], gt [B][1][H][W], boxes xywh [B][cap][>= 4] in pixels of the ground-truth grid, counts [B]
//   -> boxes   [B][cap][10] = abs_rel, sq_rel, rmse, rmse_log, log10, delta1, delta2, delta3, n_valid, gt_mean  per box
//      regions [B][2][10]   the same record over the valid pixels under ANY of the image's boxes (row 0) and under none (row 1)
// (the record is defined in include/objcavit_hip.h).  The per-pixel statement -- clamp, un-mirrored average, bilinear taps, nan / inf
// fix, the nine terms -- is csrc/metric_pixel.hpp's, the one csrc/metrics.hip evaluates; which pixels a box owns is csrc/box_edges.hpp's
// rule, the one csrc/object_depth.hip reads the final map by.  The resized prediction is never materialised.
//
// Box pass: one workgroup per (image, box row), laid over the box as object_depth_kernel is (TW columns x 256 / TW rows of threads, a
// column loop beyond 256, four rows of ground truth in flight per thread).  Region pass: (tiles, B) workgroups over flat pixel ranges,
// as the image record's partial kernel; a workgroup first writes the image's boxes as integer pixel ranges into LDS, keeping only those
// whose rows meet its own (compacted by ballot: the order differs from run to run, membership does not), then tests every valid pixel
// against that list until the first hit; a finish launch adds the tiles in order.  The five real sums and the sum of gt are float64
// from the first add, the three delta counts and n are integers.  Per-thread partials over the thread's fixed pixels, xor shuffles,
// the waves' partials from LDS in wave order: two calls give the same bytes; no float atomic, no workgroup waits for another.
#include "box_edges.hpp"
#include "common.hpp"
#include "metric_pixel.hpp"
#include "../../include/objcavit_hip.h"

namespace {

using namespace ocv_metric;

constexpr int OM_THREADS = 256, OM_WAVES = OM_THREADS / OCV_WAVE, OM_ROWS = 4, OM_FIELDS = 10;
constexpr int OM_REAL = 6;        // float64 sums: abs_rel, sq_rel, sq, sq_log, log10, gt
constexpr int OM_INT = 4;         // integer sums: d1, d2, d3, count
constexpr int OM_MAX_BOXES = OCV_OBJECT_METRICS_MAX_BOXES;
constexpr int OM_FINISH_THREADS = OCV_WAVE * OM_FIELDS;

struct ObjMetArgs : MapView {
  const float *pred, *mirror, *gt, *xywh;
  const int* counts;
  float *boxes, *regions;
  double* part;                   // [B][tiles][2][OM_FIELDS]: per set the five real sums, d1, d2, d3, count, sum of gt
  long xywh_row_stride;
  int B, cap, y0, y1, x0, x1, tiles;
  float half;
};

struct Sums {
  double f[OM_REAL];
  unsigned c[OM_INT];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int i = 0; i < OM_REAL; ++i) f[i] = 0.0;
#pragma unroll
    for (int i = 0; i < OM_INT; ++i) c[i] = 0u;
  }
  // the terms t of a pixel with ground truth g, where `on` (off: nothing changes -- no branch, no indexed register)
  __device__ __forceinline__ void add(const float t[NSUM], float g, bool on) {
#pragma unroll
    for (int i = 0; i < 5; ++i) f[i] += on ? (double)t[i] : 0.0;
    f[5] += on ? (double)g : 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) c[i] += (on && t[5 + i] != 0.f) ? 1u : 0u;
    c[3] += on ? 1u : 0u;
  }
  __device__ __forceinline__ void wave_reduce() {
#pragma unroll
    for (int i = 0; i < OM_REAL; ++i) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) f[i] += __shfl_xor(f[i], o, OCV_WAVE);
    }
#pragma unroll
    for (int i = 0; i < OM_INT; ++i) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) c[i] += (unsigned)__shfl_xor((int)c[i], o, OCV_WAVE);
    }
  }
};

// ten totals (the layout of `part`) -> a record
__device__ __forceinline__ void om_record(const double tot[OM_FIELDS], float* r) {
  record(tot, r);
  r[9] = tot[8] > 0.0 ? (float)(tot[9] / tot[8]) : 0.f;
}

__global__ __launch_bounds__(OM_THREADS) void object_metrics_box_kernel(ObjMetArgs p) {
  __shared__ double s_f[OM_REAL][OM_WAVES];
  __shared__ unsigned s_c[OM_INT][OM_WAVES];

  const int tid = threadIdx.x, lane = tid & (OCV_WAVE - 1), wave = tid / OCV_WAVE;
  const long row = blockIdx.x;
  const int b = (int)(row / p.cap), j = (int)(row - (long)b * p.cap);
  float* out = p.boxes + row * OM_FIELDS;

  // everything up to the barrier is uniform over the workgroup
  int x0 = 0, x1 = 0, y0 = 0, y1 = 0;
  bool live = j < p.counts[b];
  if (live) {
    const float* box = p.xywh + row * p.xywh_row_stride;
    const bool okx = od_edges(box[0], box[2], p.half, p.W, x0, x1);
    const bool oky = od_edges(box[1], box[3], p.half, p.H, y0, y1);
    // (no pixel outside the crop box is valid: the box is read only where the two meet)
    x0 = max(x0, p.x0); x1 = min(x1, p.x1); y0 = max(y0, p.y0); y1 = min(y1, p.y1);
    live = okx && oky && x1 > x0 && y1 > y0;
  }
  if (!live) {
    if (tid < OM_FIELDS) out[tid] = 0.f;
    return;
  }

  int log_tw = 0;
  while ((1 << log_tw) < x1 - x0 && (1 << log_tw) < OM_THREADS) ++log_tw;
  const int TW = 1 << log_tw, TH = OM_THREADS >> log_tw;
  const int tx = tid & (TW - 1), ty = tid >> log_tw;
  const float* pb = p.pred + (long)b * p.h * p.w;
  const float* mb = p.mirror != nullptr ? p.mirror + (long)b * p.h * p.w : nullptr;
  const float* gb = p.gt + (long)b * p.H * p.W;
  const float nan = __uint_as_float(0x7fc00000u);

  Sums s;
  s.clear();
  for (int yb = y0; yb < y1; yb += OM_ROWS * TH) {
    for (int xb = x0; xb < x1; xb += TW) {
      const int x = xb + tx;
      float g[OM_ROWS];
#pragma unroll
      for (int u = 0; u < OM_ROWS; ++u) {
        const int y = yb + ty + u * TH;
        g[u] = (x < x1 && y < y1) ? gb[(long)y * p.W + x] : nan;              // NaN is outside every depth range
      }
#pragma unroll
      for (int u = 0; u < OM_ROWS; ++u) {
        if (g[u] > p.dmin && g[u] <= p.dmax) {
          const float v = fixed(p, resized(p, pb, mb, yb + ty + u * TH, x));
          float t[NSUM];
          terms(g[u], v, t);
          s.add(t, g[u], true);
        }
      }
    }
  }
  s.wave_reduce();
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < OM_REAL; ++i) s_f[i][wave] = s.f[i];
#pragma unroll
    for (int i = 0; i < OM_INT; ++i) s_c[i][wave] = s.c[i];
  }
  __syncthreads();
  if (tid != 0) return;
  double tot[OM_FIELDS];
#pragma unroll
  for (int i = 0; i < 5; ++i) tot[i] = ((s_f[i][0] + s_f[i][1]) + s_f[i][2]) + s_f[i][3];
#pragma unroll
  for (int i = 0; i < OM_INT; ++i) tot[5 + i] = (double)(s_c[i][0] + s_c[i][1] + s_c[i][2] + s_c[i][3]);
  tot[9] = ((s_f[5][0] + s_f[5][1]) + s_f[5][2]) + s_f[5][3];
  om_record(tot, out);
}

__global__ __launch_bounds__(OM_THREADS) void object_regions_partial_kernel(ObjMetArgs p) {
  __shared__ int4 s_box[OM_MAX_BOXES];                                        // x0, x1, y0, y1 of the boxes that meet this tile's rows
  __shared__ int s_n;
  __shared__ double s_f[2][OM_REAL][OM_WAVES];
  __shared__ unsigned s_c[2][OM_INT][OM_WAVES];

  const int tid = threadIdx.x, lane = tid & (OCV_WAVE - 1), wave = tid / OCV_WAVE, tile = blockIdx.x;
  const long b = blockIdx.y;
  const long P = (long)p.H * p.W;
  const long per = (P + p.tiles - 1) / p.tiles;
  const long lo = tile * per, hi = min(P, lo + per);
  // the rows this tile's valid pixels can lie in
  const int ylo = max(lo < hi ? (int)(lo / p.W) : 0, p.y0), yhi = min(lo < hi ? (int)((hi - 1) / p.W) + 1 : 0, p.y1);
  const float* pb = p.pred + b * (long)p.h * p.w;
  const float* mb = p.mirror != nullptr ? p.mirror + b * (long)p.h * p.w : nullptr;
  const float* gb = p.gt + b * P;

  if (tid == 0) s_n = 0;
  __syncthreads();
  const int cnt = min(p.counts[b], p.cap);
  for (int j0 = 0; j0 < cnt; j0 += OM_THREADS) {                              // (uniform trip count)
    const int j = j0 + tid;
    int4 e = make_int4(0, 0, 0, 0);
    bool keep = false;
    if (j < cnt) {
      const float* box = p.xywh + (b * p.cap + j) * p.xywh_row_stride;
      const bool okx = od_edges(box[0], box[2], p.half, p.W, e.x, e.y);
      const bool oky = od_edges(box[1], box[3], p.half, p.H, e.z, e.w);
      keep = okx && oky && e.z < yhi && e.w > ylo && e.x < p.x1 && e.y > p.x0;
    }
    const unsigned long long m = __ballot(keep);
    int base = 0;
    if (lane == 0 && m != 0ull) base = atomicAdd(&s_n, __popcll(m));           // integer, LDS: which wave comes first does not matter
    base = __shfl(base, 0, OCV_WAVE);
    if (keep) s_box[base + __popcll(m & ((1ull << lane) - 1ull))] = e;
  }
  __syncthreads();
  const int n = s_n;

  Sums in, bg;
  in.clear();
  bg.clear();
#pragma unroll 2
  for (long pix = lo + tid; pix < hi; pix += OM_THREADS) {
    const float g = gb[pix];
    const int Y = (int)(pix / p.W), X = (int)(pix - (long)Y * p.W);
    if (g > p.dmin && g <= p.dmax && Y >= p.y0 && Y < p.y1 && X >= p.x0 && X < p.x1) {
      bool inside = false;
      for (int k = 0; k < n; ++k) {                                           // every lane reads the same LDS words: a broadcast
        const int4 e = s_box[k];
        if (X >= e.x && X < e.y && Y >= e.z && Y < e.w) { inside = true; break; }
      }
      const float v = fixed(p, resized(p, pb, mb, Y, X));
      float t[NSUM];
      terms(g, v, t);
      in.add(t, g, inside);
      bg.add(t, g, !inside);
    }
  }
  in.wave_reduce();
  bg.wave_reduce();
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < OM_REAL; ++i) { s_f[0][i][wave] = in.f[i]; s_f[1][i][wave] = bg.f[i]; }
#pragma unroll
    for (int i = 0; i < OM_INT; ++i) { s_c[0][i][wave] = in.c[i]; s_c[1][i][wave] = bg.c[i]; }
  }
  __syncthreads();
  if (tid < 2 * OM_FIELDS) {
    const int set = tid / OM_FIELDS, q = tid - set * OM_FIELDS;
    double v;
    if (q >= 5 && q < 9) {
      const unsigned* c = s_c[set][q - 5];
      v = (double)(c[0] + c[1] + c[2] + c[3]);
    } else {
      const double* f = s_f[set][q < 5 ? q : 5];
      v = ((f[0] + f[1]) + f[2]) + f[3];
    }
    p.part[((b * p.tiles + tile) * 2 + set) * OM_FIELDS + q] = v;
  }
}

// one workgroup per image, one wavefront per column of `part` (both sets): lanes stride over the tiles, a fixed xor-tree adds the lanes
__global__ __launch_bounds__(OM_FINISH_THREADS) void object_regions_finish_kernel(const double* __restrict__ part, int tiles,
                                                                                 float* __restrict__ regions) {
  __shared__ double tot[2][OM_FIELDS];
  const int b = blockIdx.x, q = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double s0 = 0.0, s1 = 0.0;
  for (int t = lane; t < tiles; t += 64) {
    const double* pt = part + ((long)b * tiles + t) * 2 * OM_FIELDS;
    s0 += pt[q];
    s1 += pt[OM_FIELDS + q];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { s0 += __shfl_xor(s0, o, 64); s1 += __shfl_xor(s1, o, 64); }
  if (lane == 0) { tot[0][q] = s0; tot[1][q] = s1; }
  __syncthreads();
  if (threadIdx.x < 2) om_record(tot[threadIdx.x], regions + ((long)b * 2 + threadIdx.x) * OM_FIELDS);
}

}  // namespace

extern "C" size_t ocv_object_metrics_workspace_bytes(int B, int H, int W) {
  if (B < 1 || H < 1 || W < 1) return 0;
  return (size_t)B * metric_tiles(B, (long)H * W) * 2 * OM_FIELDS * sizeof(double);
}

extern "C" int ocv_object_metrics_fwd(const float* pred, const float* pred_mirror, int h, int w, const float* gt, int H, int W,
                                      float min_depth, float max_depth, int crop_y0, int crop_y1, int crop_x0, int crop_x1,
                                      const float* xywh, long xywh_row_stride, const int* counts, int B, int cap, float half,
                                      float* boxes_out, float* regions_out, void* workspace, size_t workspace_bytes,
                                      ocv_stream_t stream) {
  OCV_CHECK_ARG(pred && gt && xywh && counts && boxes_out, "ocv_object_metrics_fwd: null pointer (pred, gt, xywh, counts, boxes_out)");
  OCV_CHECK_ARG(regions_out == nullptr || workspace != nullptr, "ocv_object_metrics_fwd: null pointer (the region pass needs a workspace)");
  OCV_CHECK_ARG(B >= 1 && B <= 65535 && cap >= 1 && h >= 1 && w >= 1 && H >= 1 && W >= 1,
                "ocv_object_metrics_fwd: bad sizes (B 1 .. 65535; cap, h, w, H, W must be >= 1)");
  OCV_CHECK_ARG(H <= (1 << 24) && W <= (1 << 24) && (long)H * W <= 0x7fffffffL && (long)h * w <= 0x7fffffffL && (long)B * cap <= 0x7fffffffL,
                "ocv_object_metrics_fwd: bad sizes (H, W <= 2^24; H * W, h * w and B * cap below 2^31)");
  OCV_CHECK_ARG(min_depth < max_depth, "ocv_object_metrics_fwd: min_depth must be below max_depth");
  OCV_CHECK_ARG(crop_y0 >= 0 && crop_y0 <= crop_y1 && crop_y1 <= H && crop_x0 >= 0 && crop_x0 <= crop_x1 && crop_x1 <= W,
                "ocv_object_metrics_fwd: crop box outside the ground-truth map (pass 0, H, 0, W for no crop)");
  OCV_CHECK_ARG(half > 0.f && half <= 0.5f, "ocv_object_metrics_fwd: half = 0.5 * shrink must be in (0, 0.5]");
  OCV_CHECK_ARG(xywh_row_stride >= 4, "ocv_object_metrics_fwd: xywh_row_stride must be >= 4 (cx, cy, w, h)");
  OCV_CHECK_ARG(regions_out == nullptr || cap <= OM_MAX_BOXES,
                "ocv_object_metrics_fwd: cap = %d boxes per image; the region pass takes at most %d (pass regions_out = null for the "
                "boxes alone)", cap, OM_MAX_BOXES);
  OCV_CHECK_ARG((reinterpret_cast<uintptr_t>(pred) & 3) == 0 && (reinterpret_cast<uintptr_t>(pred_mirror) & 3) == 0 &&
                (reinterpret_cast<uintptr_t>(gt) & 3) == 0 && (reinterpret_cast<uintptr_t>(xywh) & 3) == 0 &&
                (reinterpret_cast<uintptr_t>(counts) & 3) == 0 && (reinterpret_cast<uintptr_t>(boxes_out) & 3) == 0 &&
                (reinterpret_cast<uintptr_t>(regions_out) & 3) == 0, "ocv_object_metrics_fwd: misaligned pointer");
  OCV_CHECK_ARG(regions_out == nullptr || (workspace_bytes >= ocv_object_metrics_workspace_bytes(B, H, W) &&
                                           (reinterpret_cast<uintptr_t>(workspace) & 7) == 0),
                "ocv_object_metrics_fwd: workspace too small or misaligned");
  const int tiles = metric_tiles(B, (long)H * W);
  ObjMetArgs a{map_view(h, w, H, W, min_depth, max_depth), pred, pred_mirror, gt, xywh, counts, boxes_out, regions_out,
               (double*)workspace, xywh_row_stride, B, cap, crop_y0, crop_y1, crop_x0, crop_x1, tiles, half};
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(object_metrics_box_kernel, dim3((unsigned)((long)B * cap)), dim3(OM_THREADS), 0, st, a);
  OCV_CHECK_LAUNCH("ocv_object_metrics_fwd(boxes)");
  if (regions_out == nullptr) return 0;
  hipLaunchKernelGGL(object_regions_partial_kernel, dim3(tiles, B), dim3(OM_THREADS), 0, st, a);
  OCV_CHECK_LAUNCH("ocv_object_metrics_fwd(regions partial)");
  hipLaunchKernelGGL(object_regions_finish_kernel, dim3(B), dim3(OM_FINISH_THREADS), 0, st, (const double*)workspace, tiles, regions_out);
  OCV_CHECK_LAUNCH("ocv_object_metrics_fwd(regions finish)");
  return 0;
}
