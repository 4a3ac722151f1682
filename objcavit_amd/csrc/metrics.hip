// Validation-step arithmetic on the device, one pass (row N2 of SURVEY.md section 8f): what the reference does between
// the model output and its eight logged numbers --
//   flip-TTA average 0.5 (clamp(d) + clamp(flip(d_mirror)))                  modules/GraphBinsLM.py:159-181
//   bilinear align_corners resize to the ground-truth size, nan -> min_depth,
//   +-inf -> max_depth, validity mask min < gt <= max, Garg / Eigen crop      metrics/MetricsPreprocess.py:14-45
//   abs_rel, sq_rel, rmse, rmse_log, log10, delta 1.25 / 1.25^2 / 1.25^3      metrics/AbsRel.py:44-52, SqRel.py:45-52,
//                                                                            RMSE.py:48-55, RMSELog.py:45-52,
//                                                                            Log10.py:52-61, AccThresh.py:59-66
// -- as ONE record of 10 floats per image (objcavit_amd/dp.py RECORD_FIELDS), so that a data-parallel job needs a
// single all-gather (the reference: ~10 element-wise passes over B x H x W, a boolean gather, 16 torchmetrics states
// and 32 scalar collectives).  The resized prediction is never materialised: a thread evaluates the four low-resolution
// taps of its pixel (clamped, averaged with the mirrored tap) straight from the two model outputs.
// Two stages, fixed order, no float atomics: (tiles, B) workgroups reduce 9 double-precision sums each, a second tiny
// launch adds the tiles in order and finishes the means / square roots.  HBM-bound: 4 B of ground truth per pixel.
#include "common.hpp"
#include "metric_pixel.hpp"
#include "../../include/objcavit_hip.h"

namespace {

using namespace ocv_metric;       // NSUM, MapView, the per-pixel statement, record, metric_tiles (shared with csrc/object_metrics.hip)

constexpr int NLOSS = 4;          // sum g, sum g^2 (g = log p - log gt), sum_t min_k (t - c_k)^2, masked count
constexpr int MAX_BINS = 1024;
constexpr unsigned NO_TARGET_LO = 0xFFFFFFFFu, NO_TARGET_HI = 0u;   // empty interval: above / below every valid target's bit pattern

struct MetArgs : MapView {
  const float *pred, *mirror, *gt;
  double* part;                   // [B][tiles][NSUM]
  int y0, y1, x0, x1, tiles;
};

// The validation loss rides on the same pass (ocv_depth_metrics_loss_fwd: losses/SILogLoss.py:28-56, losses/BinsChamferLoss.py:21-37).
struct LossArgs {
  const float* edges;             // [B][n_bins + 1]
  double* lpart;                  // [B][tiles][NLOSS]
  unsigned* slab;                 // [B][tiles][2][n_bins + 1]: smallest / largest target per interval between sorted centres
  int n_bins;
};

// Bin centres 0.5 (e[k+1] + e[k]) of one image, sorted ascending into `cen` (rank sort: every thread counts the centres below its
// own, ties by index; all lanes read the same LDS word per step).  The edges may come in any order: a scanned cumsum is not
// guaranteed monotone in fp32.  `cen64` (nullable): the same centres unrounded (a sum of two floats is exact in double), in the same
// order -- rounding to fp32 is monotone, and no fp32 target lies strictly between a centre and its fp32 image, so the targets
// below / at-or-above the rounded centre are those below / at-or-above the exact one.  Ends with a barrier.
__device__ __forceinline__ void sorted_centres(const float* __restrict__ eb, int n, float* craw, float* cen, double* cen64, int tid,
                                               int nthr) {
  // A NaN centre is taken as +inf (ranks would collide otherwise and leave sorted slots unwritten).  The tail up to a multiple of
  // four is +inf too, for whole float4 reads: below no centre, and beyond every k in the tie rule.
  const int n4 = (n + 3) & ~3;
  for (int k = tid; k < n4; k += nthr) {
    const float v = k < n ? 0.5f * (eb[k + 1] + eb[k]) : __builtin_inff();
    craw[k] = v == v ? v : __builtin_inff();
  }
  __syncthreads();
  for (int k = tid; k < n; k += nthr) {
    const float c = craw[k];
    int r = 0;
#pragma unroll 4                                                  // vector LDS reads, several in flight
    for (int i = 0; i < n4; i += 4) {
      const float4 o = *reinterpret_cast<const float4*>(craw + i);
      r += (o.x < c || (o.x == c && i < k)) ? 1 : 0;
      r += (o.y < c || (o.y == c && i + 1 < k)) ? 1 : 0;
      r += (o.z < c || (o.z == c && i + 2 < k)) ? 1 : 0;
      r += (o.w < c || (o.w == c && i + 3 < k)) ? 1 : 0;
    }
    cen[r] = c;
    if (cen64 != nullptr) {
      const double v = 0.5 * ((double)eb[k + 1] + (double)eb[k]);
      cen64[r] = v == v ? v : (double)__builtin_inff();
    }
  }
  __syncthreads();
}

// LOSS = false is ocv_depth_metrics_fwd's kernel; LOSS = true adds, on the same read of gt, the SILog sums over the mask WITHOUT the
// crop and without nan_to_num, the Chamfer term of the targets (nearest sorted centre: 1-D, so one of the two that bracket t), and
// per interval between centres the smallest / largest target seen (their bit patterns order as unsigned: targets are > min_depth >= 0).
// The metric sums see the same pixels in the same order with the same flush points in both instantiations.
template <bool LOSS>
__global__ __launch_bounds__(256) void depth_metrics_partial_kernel(MetArgs p, LossArgs q) {
  __shared__ double red[NSUM][4];
  __shared__ __attribute__((aligned(16))) float craw[LOSS ? MAX_BINS : 4];
  __shared__ float cen[LOSS ? MAX_BINS : 1];
  __shared__ unsigned tlo[LOSS ? MAX_BINS + 1 : 1], thi[LOSS ? MAX_BINS + 1 : 1];
  __shared__ double lred[LOSS ? NLOSS : 1][4];
  const int tid = threadIdx.x, tile = blockIdx.x;
  const long b = blockIdx.y;
  const long P = (long)p.H * p.W;
  const long per = (P + p.tiles - 1) / p.tiles;
  const long lo = tile * per, hi = min(P, lo + per);
  const float* pb = p.pred + b * (long)p.h * p.w;
  const float* mb = p.mirror != nullptr ? p.mirror + b * (long)p.h * p.w : nullptr;
  const float* gb = p.gt + b * P;
  float s[NSUM];
#pragma unroll
  for (int i = 0; i < NSUM; ++i) s[i] = 0.f;
  double acc[NSUM];
#pragma unroll
  for (int i = 0; i < NSUM; ++i) acc[i] = 0.0;
  int pending = 0;
  double lacc[3] = {0.0, 0.0, 0.0};
  int lcount = 0;
  const int n = q.n_bins;
  if constexpr (LOSS) {
    for (int j = tid; j <= n; j += 256) { tlo[j] = NO_TARGET_LO; thi[j] = NO_TARGET_HI; }
    sorted_centres(q.edges + b * (n + 1), n, craw, cen, nullptr, tid, 256);
  }
#pragma unroll 4
  for (long pix = lo + tid; pix < hi; pix += 256) {
    const float g = gb[pix];
    const int Y = (int)(pix / p.W), X = (int)(pix - (long)Y * p.W);
    const bool mask = g > p.dmin && g <= p.dmax;
    const bool valid = mask && Y >= p.y0 && Y < p.y1 && X >= p.x0 && X < p.x1;
    if (LOSS ? mask : valid) {
      float v = resized(p, pb, mb, Y, X);
      if constexpr (LOSS) {
        const float gl = logf(v) - logf(g);                       // a NaN prediction stays NaN here, as in the reference
        lacc[0] += (double)gl;
        lacc[1] += (double)gl * (double)gl;
        int j = 0;                                                // number of centres <= g
        for (int len = n; len > 0;) {
          const int half = len >> 1;
          if (cen[j + half] <= g) { j += half + 1; len -= half + 1; } else len = half;
        }
        const float dl0 = g - cen[j > 0 ? j - 1 : 0], dr0 = g - cen[j < n ? j : n - 1];
        lacc[2] += (double)fminf(dl0 * dl0, dr0 * dr0);
        ++lcount;
        const unsigned bits = __float_as_uint(g);
        if (bits < tlo[j]) atomicMin(&tlo[j], bits);              // read first: a smooth depth map rarely moves an interval's ends
        if (bits > thi[j]) atomicMax(&thi[j], bits);
      }
      if (LOSS && !valid) continue;
      v = fixed(p, v);
      float t[NSUM];
      terms(g, v, t);
#pragma unroll
      for (int i = 0; i < NSUM; ++i) s[i] += t[i];
      if (++pending == 64) {                                    // short fp32 runs, double-precision totals
#pragma unroll
        for (int i = 0; i < NSUM; ++i) { acc[i] += (double)s[i]; s[i] = 0.f; }
        pending = 0;
      }
    }
  }
  // workgroup totals: a fixed xor-tree over each wavefront's 64 lanes, then the four wavefronts in order (one thread walking 256 LDS
  // doubles per sum was a third of the launch)
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int i = 0; i < NSUM; ++i) {
    double t = acc[i] + (double)s[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
    if (lane == 0) red[i][wave] = t;
  }
  if constexpr (LOSS) {
#pragma unroll
    for (int i = 0; i < NLOSS; ++i) {
      double t = i < 3 ? lacc[i] : (double)lcount;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
      if (lane == 0) lred[i][wave] = t;
    }
  }
  __syncthreads();
  if (tid < NSUM) p.part[((b * p.tiles) + tile) * NSUM + tid] = ((red[tid][0] + red[tid][1]) + red[tid][2]) + red[tid][3];
  if constexpr (LOSS) {
    if (tid < NLOSS) q.lpart[((b * p.tiles) + tile) * NLOSS + tid] = ((lred[tid][0] + lred[tid][1]) + lred[tid][2]) + lred[tid][3];
    unsigned* sl = q.slab + ((b * p.tiles) + tile) * 2 * (long)(n + 1);
    for (int j = tid; j <= n; j += 256) { sl[j] = tlo[j]; sl[n + 1 + j] = thi[j]; }
  }
}

// one workgroup per image, one wavefront per sum: lanes stride over the tiles, then a fixed xor-tree adds the 64 lanes
__global__ __launch_bounds__(64 * NSUM) void depth_metrics_finish_kernel(const double* __restrict__ part, int tiles,
                                                                       float* __restrict__ rec, int B, long first_id) {
  __shared__ double tot[NSUM];
  const int b = blockIdx.x, i = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double s = 0.0;
  for (int t = lane; t < tiles; t += 64) s += part[((long)b * tiles + t) * NSUM + i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) tot[i] = s;
  __syncthreads();
  if (threadIdx.x != 0) return;
  float* r = rec + (long)b * 10;
  record(tot, r);
  r[9] = (float)(first_id + b);
}

// Loss record of one image (one workgroup of 1024): the tiles' four sums in order; the tiles' interval slabs (min / max of unsigned: exact in any
// order); then every sorted centre's nearest target = the nearer of the largest target below it (prefix-max of hi over the intervals up to
// its own) and the smallest at or above it (suffix-min of lo over the intervals beyond), however many empty intervals lie between.
__global__ __launch_bounds__(1024) void val_loss_finish_kernel(LossArgs q, int tiles, float* __restrict__ lrec, long first_id) {
  __shared__ __attribute__((aligned(16))) float craw[MAX_BINS];
  __shared__ float cen[MAX_BINS];
  __shared__ double cen64[MAX_BINS];
  __shared__ unsigned slo[4][MAX_BINS + 1], shi[4][MAX_BINS + 1];
  __shared__ double tot[NLOSS], xred[16];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = q.n_bins;
  if (wave < NLOSS) {
    double s = 0.0;
    for (int t = lane; t < tiles; t += 64) s += q.lpart[((long)b * tiles + t) * NLOSS + wave];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) tot[wave] = s;
  }
  {
    const int grp = tid >> 8;                                    // four groups of 256 threads share the tiles
    for (int j = tid & 255; j <= n; j += 256) {
      unsigned l = NO_TARGET_LO, h = NO_TARGET_HI;
#pragma unroll 8                                                 // independent loads in flight
      for (int t = grp; t < tiles; t += 4) {
        const unsigned* sl = q.slab + ((long)b * tiles + t) * 2 * (long)(n + 1);
        l = min(l, sl[j]);
        h = max(h, sl[n + 1 + j]);
      }
      slo[grp][j] = l;
      shi[grp][j] = h;
    }
  }
  sorted_centres(q.edges + (long)b * (n + 1), n, craw, cen, cen64, tid, 1024);
  for (int j = tid; j <= n; j += 1024) {
    slo[0][j] = min(min(slo[0][j], slo[1][j]), min(slo[2][j], slo[3][j]));
    shi[0][j] = max(max(shi[0][j], shi[1][j]), max(shi[2][j], shi[3][j]));
  }
  __syncthreads();
  int cur = 0;                                                   // Hillis-Steele scans, ping-pong between rows cur and cur ^ 1
  for (int o = 1; o <= n; o <<= 1) {
    for (int j = tid; j <= n; j += 1024) {
      shi[cur ^ 1][j] = j >= o ? max(shi[cur][j], shi[cur][j - o]) : shi[cur][j];
      slo[cur ^ 1][j] = j + o <= n ? min(slo[cur][j], slo[cur][j + o]) : slo[cur][j];
    }
    __syncthreads();
    cur ^= 1;
  }
  double sx = 0.0;
  for (int k = tid; k < n; k += 1024) {
    // in double from the exact centre: where the targets are dense the nearest one sits within a few ulps of the fp32 centre, and
    // (c - t)^2 from the ROUNDED centre is then off by per cent (profiles/val_loss.txt, section 1)
    const double c = cen64[k];
    const unsigned hb = shi[cur][k], lb = slo[cur][k + 1];       // targets below c: intervals 0 .. k; at or above: k + 1 .. n
    double dx = (double)__builtin_inff();
    if (hb != NO_TARGET_HI) { const double d = c - (double)__uint_as_float(hb); dx = d * d; }
    if (lb != NO_TARGET_LO) { const double d = (double)__uint_as_float(lb) - c; dx = fmin(dx, d * d); }
    sx += dx;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sx += __shfl_xor(sx, o, 64);
  if (lane == 0) xred[wave] = sx;
  __syncthreads();
  if (tid != 0) return;
  double x = 0.0;
  for (int i = 0; i < 16; ++i) x += xred[i];
  const double cnt = tot[3], m = cnt > 0.0 ? cnt : 1.0;
  float* r = lrec + (long)b * 6;
  r[0] = (float)(tot[0] / m);
  r[1] = (float)(tot[1] / m);
  r[2] = (float)cnt;
  r[3] = cnt > 0.0 ? (float)(x / (double)n) : 0.f;               // an image without targets: both Chamfer terms 0
  r[4] = (float)(tot[2] / m);
  r[5] = (float)(first_id + b);
}

}  // namespace

extern "C" size_t ocv_depth_metrics_workspace_bytes(int B, int H, int W) {
  if (B < 1 || H < 1 || W < 1) return 0;
  return (size_t)B * metric_tiles(B, (long)H * W) * NSUM * sizeof(double);
}

extern "C" int ocv_depth_metrics_fwd(const float* pred, const float* pred_mirror, int h, int w, const float* gt, int H, int W,
                                     float min_depth, float max_depth, int crop_y0, int crop_y1, int crop_x0, int crop_x1,
                                     long first_image_id, float* records, int B, void* workspace, size_t workspace_bytes,
                                     ocv_stream_t stream) {
  OCV_CHECK_ARG(pred && gt && records && workspace, "ocv_depth_metrics_fwd: null pointer");
  OCV_CHECK_ARG(B >= 1 && B <= 65535 && h >= 1 && w >= 1 && H >= 1 && W >= 1, "ocv_depth_metrics_fwd: bad sizes");
  OCV_CHECK_ARG(min_depth < max_depth, "ocv_depth_metrics_fwd: min_depth must be below max_depth");
  OCV_CHECK_ARG(crop_y0 >= 0 && crop_y0 <= crop_y1 && crop_y1 <= H && crop_x0 >= 0 && crop_x0 <= crop_x1 && crop_x1 <= W,
                "ocv_depth_metrics_fwd: crop box outside the ground-truth map (pass 0, H, 0, W for no crop)");
  OCV_CHECK_ARG(workspace_bytes >= ocv_depth_metrics_workspace_bytes(B, H, W) && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
                "ocv_depth_metrics_fwd: workspace too small or misaligned");
  const int tiles = metric_tiles(B, (long)H * W);
  MetArgs a{map_view(h, w, H, W, min_depth, max_depth), pred, pred_mirror, gt, (double*)workspace, crop_y0, crop_y1, crop_x0, crop_x1, tiles};
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(depth_metrics_partial_kernel<false>, dim3(tiles, B), dim3(256), 0, st, a, LossArgs{nullptr, nullptr, nullptr, 0});
  OCV_CHECK_LAUNCH("ocv_depth_metrics_fwd(partial)");
  hipLaunchKernelGGL(depth_metrics_finish_kernel, dim3(B), dim3(64 * NSUM), 0, st, (const double*)workspace, tiles, records, B,
                     first_image_id);
  OCV_CHECK_LAUNCH("ocv_depth_metrics_fwd(finish)");
  return 0;
}

extern "C" size_t ocv_depth_metrics_loss_workspace_bytes(int B, int H, int W, int n_bins) {
  if (B < 1 || H < 1 || W < 1 || n_bins < 1 || n_bins > MAX_BINS) return 0;
  const size_t wg = (size_t)B * metric_tiles(B, (long)H * W);
  return wg * (NSUM + NLOSS) * sizeof(double) + wg * 2 * (size_t)(n_bins + 1) * sizeof(unsigned);
}

extern "C" int ocv_depth_metrics_loss_fwd(const float* pred, const float* pred_mirror, int h, int w, const float* gt, int H, int W,
                                          float min_depth, float max_depth, int crop_y0, int crop_y1, int crop_x0, int crop_x1,
                                          const float* bin_edges, int n_bins, long first_image_id, float* records,
                                          float* loss_records, int B, void* workspace, size_t workspace_bytes, ocv_stream_t stream) {
  OCV_CHECK_ARG(pred && gt && bin_edges && records && loss_records && workspace, "ocv_depth_metrics_loss_fwd: null pointer");
  OCV_CHECK_ARG(B >= 1 && B <= 65535 && h >= 1 && w >= 1 && H >= 1 && W >= 1, "ocv_depth_metrics_loss_fwd: bad sizes");
  OCV_CHECK_ARG(n_bins >= 1 && n_bins <= MAX_BINS, "ocv_depth_metrics_loss_fwd: n_bins must be 1 .. 1024");
  OCV_CHECK_ARG(min_depth >= 0.f && min_depth < max_depth,
                "ocv_depth_metrics_loss_fwd: need 0 <= min_depth < max_depth (targets are ordered by their bit patterns)");
  OCV_CHECK_ARG(crop_y0 >= 0 && crop_y0 <= crop_y1 && crop_y1 <= H && crop_x0 >= 0 && crop_x0 <= crop_x1 && crop_x1 <= W,
                "ocv_depth_metrics_loss_fwd: crop box outside the ground-truth map (pass 0, H, 0, W for no crop)");
  OCV_CHECK_ARG(workspace_bytes >= ocv_depth_metrics_loss_workspace_bytes(B, H, W, n_bins) &&
                    (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
                "ocv_depth_metrics_loss_fwd: workspace too small or misaligned");
  const int tiles = metric_tiles(B, (long)H * W);
  const size_t wg = (size_t)B * tiles;
  double* part = (double*)workspace;
  MetArgs a{map_view(h, w, H, W, min_depth, max_depth), pred, pred_mirror, gt, part, crop_y0, crop_y1, crop_x0, crop_x1, tiles};
  LossArgs q{bin_edges, part + wg * NSUM, (unsigned*)(part + wg * (NSUM + NLOSS)), n_bins};
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(depth_metrics_partial_kernel<true>, dim3(tiles, B), dim3(256), 0, st, a, q);
  OCV_CHECK_LAUNCH("ocv_depth_metrics_loss_fwd(partial)");
  hipLaunchKernelGGL(depth_metrics_finish_kernel, dim3(B), dim3(64 * NSUM), 0, st, (const double*)part, tiles, records, B, first_image_id);
  OCV_CHECK_LAUNCH("ocv_depth_metrics_loss_fwd(finish)");
  hipLaunchKernelGGL(val_loss_finish_kernel, dim3(B), dim3(1024), 0, st, q, tiles, loss_records, first_image_id);
  OCV_CHECK_LAUNCH("ocv_depth_metrics_loss_fwd(loss finish)");
  return 0;
}
