// Output end of the predict path (row N5 of DESIGN.md section 6b): the model's half-resolution, unclamped depth_pred -> the map a user
// wants, WRITTEN OUT (csrc/metrics.hip forms the same map per pixel and never stores it):
//   flip-TTA average 0.5 (clamp(d) + clamp(flip(d_mirror))), or clamp(d) alone           modules/GraphBinsLM.py:159-183, :295-301 (predict: no TTA)
//   bilinear align_corners resize to H x W, nan -> min_depth, +-inf -> max_depth           metrics/MetricsPreprocess.py:17-24
// in up to three forms from one evaluation: fp32 metres, the datasets' 16-bit PNG convention (x 1000 NYU, x 256 KITTI, round to
// nearest even, saturated), and a colour-mapped RGB picture through a caller-supplied 256-entry table (matplotlib Normalize + colormap
// call, modules/GraphBinsLM.py:367).  The per-pixel arithmetic is csrc/metrics.hip's, statement for statement (same taps, same
// weights, all four terms always: a NaN tap reaches its neighbours through a zero weight exactly as in ATen), so the materialised map
// is the one the metrics were computed on.  One launch; the low-resolution source (a quarter of the output's pixels) is staged in
// LDS per output tile, the outputs are streamed: 4 + 2 + 3 B per pixel.
#include "common.hpp"
#include "../../include/objcavit_hip.h"

namespace {

struct FinArgs {
  const float *pred, *mirror;
  float* depth;                       // [B][1][H][W] or null
  uint16_t* u16;                      // [B][H][W] or null
  uint8_t* rgb;                       // [B][H][W][3] or null
  const uint8_t* cmap;                // [256][3]
  int h, w, H, W, B;
  float sh, sw, dmin, dmax, u16_scale, vmin, cscale;
};

// torch.clamp semantics: NaN stays NaN (fminf / fmaxf would drop it)
__device__ __forceinline__ float clamp_keep_nan(float v, float lo, float hi) { return v != v ? v : fminf(fmaxf(v, lo), hi); }

__device__ __forceinline__ float tap(const FinArgs& p, const float* pb, const float* mb, int y, int x) {
  const float a = clamp_keep_nan(pb[y * p.w + x], p.dmin, p.dmax);
  if (mb == nullptr) return a;
  return 0.5f * (a + clamp_keep_nan(mb[y * p.w + (p.w - 1 - x)], p.dmin, p.dmax));
}

// nan_to_num(nan = min, posinf = neginf = max)
__device__ __forceinline__ float fix_non_finite(const FinArgs& p, float v) {
  if (v != v) return p.dmin;
  return __builtin_isinf(v) ? p.dmax : v;
}

// One output pixel.  `fetch(y, x)` returns the clamped (and TTA-averaged) source pixel: from global memory, or from a tile staged in LDS.
template <typename Fetch>
__device__ __forceinline__ float final_depth(const FinArgs& p, Fetch fetch, int Y, int X) {
  if (p.h == p.H && p.w == p.W) return fix_non_finite(p, fetch(Y, X));      // ATen's identity short-cut for equal sizes
  // ATen upsample_bilinear2d, align_corners = True
  const float sy = p.sh * Y, sx = p.sw * X;
  const int ya = min((int)sy, p.h - 1), xa = min((int)sx, p.w - 1);     // (the min never binds for Y < H, X < W: it keeps a tap in bounds whatever the scale rounds to)
  const int yb = ya + (ya < p.h - 1 ? 1 : 0), xb = xa + (xa < p.w - 1 ? 1 : 0);
  const float h1 = sy - (float)ya, h0 = 1.0f - h1, w1 = sx - (float)xa, w0 = 1.0f - w1;
  return fix_non_finite(p, h0 * (w0 * fetch(ya, xa) + w1 * fetch(ya, xb)) + h1 * (w0 * fetch(yb, xa) + w1 * fetch(yb, xb)));
}

__device__ __forceinline__ unsigned to_u16(const FinArgs& p, float v) { return (unsigned)fminf(fmaxf(rintf(v * p.u16_scale), 0.f), 65535.f); }

__device__ __forceinline__ int cmap_index(const FinArgs& p, float v) { return (int)fminf(fmaxf(floorf((v - p.vmin) * p.cscale), 0.f), 255.f); }

// 8 consecutive pixels at flat offset o (o % 8 == 0, outputs 16-byte aligned): two 16-byte stores of fp32, one of uint16, 24 bytes of
// RGB as three 8-byte stores
__device__ __forceinline__ void store8(const FinArgs& p, long o, const float (&v)[8]) {
  if (p.depth != nullptr) {
    *reinterpret_cast<float4*>(p.depth + o) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(p.depth + o + 4) = make_float4(v[4], v[5], v[6], v[7]);
  }
  if (p.u16 != nullptr) {
    uint4 q;
    q.x = to_u16(p, v[0]) | (to_u16(p, v[1]) << 16);
    q.y = to_u16(p, v[2]) | (to_u16(p, v[3]) << 16);
    q.z = to_u16(p, v[4]) | (to_u16(p, v[5]) << 16);
    q.w = to_u16(p, v[6]) | (to_u16(p, v[7]) << 16);
    *reinterpret_cast<uint4*>(p.u16 + o) = q;
  }
  if (p.rgb != nullptr) {
    unsigned by[24];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint8_t* c = p.cmap + 3 * cmap_index(p, v[i]);
      by[3 * i] = c[0]; by[3 * i + 1] = c[1]; by[3 * i + 2] = c[2];
    }
    uint2* d = reinterpret_cast<uint2*>(p.rgb + 3 * o);          // 24 bytes per thread: 8-byte aligned
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const unsigned* s = by + 8 * j;
      d[j] = make_uint2(s[0] | (s[1] << 8) | (s[2] << 16) | (s[3] << 24), s[4] | (s[5] << 8) | (s[6] << 16) | (s[7] << 24));
    }
  }
}

// The resize proper (W % 8 == 0): a workgroup owns a TILE_H x TILE_W tile of the output and first stages the source pixels the tile's
// taps fall on -- clamped and averaged with the mirrored map ONCE per source pixel, not once per tap -- in LDS; a thread then forms 8
// consecutive pixels of a row from LDS.  At 2x that is ~660 source pixels for 2048 outputs, each read from memory once per tile
// (the direct form issued 64 scattered loads per thread and was bound by the L1 address path: 0.7 - 1.1 TB/s).  A tile whose source
// window does not fit (a strong down-scale) reads its taps from global memory instead; same arithmetic, same values.
constexpr int TILE_H = 16, TILE_W = 128, STAGE_FLOATS = 4096;

__global__ __launch_bounds__(256) void depth_finalize_tile_kernel(FinArgs p, int tiles_x) {
  __shared__ float src[STAGE_FLOATS];
  const int tid = threadIdx.x;
  const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
  const long b = blockIdx.y;
  const float* pb = p.pred + b * (long)p.h * p.w;
  const float* mb = p.mirror != nullptr ? p.mirror + b * (long)p.h * p.w : nullptr;
  const int Y0 = ty * TILE_H, X0 = tx * TILE_W;
  const int Yl = min(Y0 + TILE_H, p.H) - 1, Xl = min(X0 + TILE_W, p.W) - 1;
  // source window of the tile: first tap of its first pixel .. second tap of its last (fp32 products of a positive scale are monotone)
  const int r0 = min((int)(p.sh * Y0), p.h - 1), r1 = min(min((int)(p.sh * Yl), p.h - 1) + 1, p.h - 1);
  const int c0 = min((int)(p.sw * X0), p.w - 1), c1 = min(min((int)(p.sw * Xl), p.w - 1) + 1, p.w - 1);
  const int nr = r1 - r0 + 1, nc = c1 - c0 + 1;
  const bool staged = nr * nc <= STAGE_FLOATS;                   // uniform over the workgroup
  if (staged) {
    for (int i = tid; i < nr * nc; i += 256) {
      const int r = i / nc, c = i - r * nc;
      src[i] = tap(p, pb, mb, r0 + r, c0 + c);
    }
  }
  __syncthreads();
  const int Y = Y0 + (tid >> 4), X = X0 + ((tid & 15) << 3);
  if (Y >= p.H || X >= p.W) return;                             // (W % 8 == 0: a group of 8 is inside the row or outside it)
  float v[8];
  if (staged) {
    auto fetch = [&](int y, int x) { return src[(y - r0) * nc + (x - c0)]; };
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = final_depth(p, fetch, Y, X + i);
  } else {
    auto fetch = [&](int y, int x) { return tap(p, pb, mb, y, x); };
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = final_depth(p, fetch, Y, X + i);
  }
  store8(p, b * (long)p.H * p.W + (long)Y * p.W + X, v);
}

// Without a tile: V = 8, a thread owns 8 consecutive pixels of an image's flat H x W map (H * W % 8 == 0; equal sizes, where there is
// nothing to share between pixels, and widths that are no multiple of 8); V = 1: one pixel, scalar stores (any size).
template <int V>
__global__ __launch_bounds__(256) void depth_finalize_kernel(FinArgs p) {
  const long P = (long)p.H * p.W;
  const long groups = P / V, total = groups * p.B;
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
    const long b = t / groups, pix0 = (t - b * groups) * V;
    const float* pb = p.pred + b * (long)p.h * p.w;
    const float* mb = p.mirror != nullptr ? p.mirror + b * (long)p.h * p.w : nullptr;
    auto fetch = [&](int y, int x) { return tap(p, pb, mb, y, x); };
    int Y = (int)(pix0 / p.W), X = (int)(pix0 - (long)Y * p.W);
    float v[V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
      v[i] = final_depth(p, fetch, Y, X);
      if (++X == p.W) { X = 0; ++Y; }
    }
    const long o = b * P + pix0;
    if constexpr (V == 8) {
      store8(p, o, v);
    } else {
      if (p.depth != nullptr) p.depth[o] = v[0];
      if (p.u16 != nullptr) p.u16[o] = (uint16_t)to_u16(p, v[0]);
      if (p.rgb != nullptr) {
        const uint8_t* c = p.cmap + 3 * cmap_index(p, v[0]);
        p.rgb[3 * o] = c[0]; p.rgb[3 * o + 1] = c[1]; p.rgb[3 * o + 2] = c[2];
      }
    }
  }
}

// ---------------------------------------------------------------------------
// The same resize for the bin head's per-pixel statistics (csrc/bin_head.hip, STATS): the distribution predicted at an output pixel
// is the MIXTURE of its source distributions with the bilinear weights above (halved over the map and the un-mirrored mirror map
// under flip-TTA).  With d_t, var_t, pmax_t the sources' mean (UNCLAMPED), variance and peak probability and w_t their weights:
//   m = sum w_t d_t     var = sum w_t (var_t + (d_t - m)^2)   (law of total variance)     depth_std = sqrt(var)     confidence = sum w_t pmax_t
// nan -> max_depth - min_depth (std), 0 (confidence).  The TTA pair of a source pixel is merged first -- mean (a + b) / 2, variance
// (var_a + var_b) / 2 + (a - b)^2 / 4, the same law applied to the inner mixture: every term stays non-negative -- so a tile stages three
// numbers per source pixel.  The weights are the depth kernel's fp32 weights, statement for statement; the sums over the taps run in
// fp64 (a few operations per pixel under a launch bound by its stores).
// ---------------------------------------------------------------------------
struct FinStatsArgs {
  const float *pred, *mirror, *var, *var_mirror, *pmax, *pmax_mirror;      // var / pmax (and their mirrors) null when their output is
  float* std_out;                     // [B][1][H][W] or null
  float* conf;                        // [B][1][H][W] or null
  int h, w, H, W, B;
  float sh, sw, span;
};

struct Src3 { float mean, var, peak; };

__device__ __forceinline__ Src3 tap3(const FinStatsArgs& p, long base, int y, int x) {
  const long i = base + y * p.w + x, j = base + y * p.w + (p.w - 1 - x);
  Src3 r{0.f, 0.f, 0.f};
  const bool tta = p.mirror != nullptr;
  if (p.std_out != nullptr) {
    const double a = p.pred[i], va = p.var[i];
    if (tta) {
      const double b = p.mirror[j], vb = p.var_mirror[j], df = a - b;
      r.mean = (float)(0.5 * (a + b));
      r.var = (float)(0.5 * (va + vb) + 0.25 * df * df);
    } else {
      r.mean = (float)a;
      r.var = (float)va;
    }
  }
  if (p.conf != nullptr) r.peak = tta ? 0.5f * (p.pmax[i] + p.pmax_mirror[j]) : p.pmax[i];
  return r;
}

struct Fin2 { float sd, cf; };

template <typename Fetch>
__device__ __forceinline__ Fin2 final_stats(const FinStatsArgs& p, Fetch fetch, int Y, int X) {
  double var, cf;
  if (p.h == p.H && p.w == p.W) {
    const Src3 s = fetch(Y, X);
    const double e = (double)s.mean - (double)s.mean;            // 0, or NaN for a non-finite mean: m = d_t here, and (d_t - m)^2 keeps it
    var = s.var + e * e; cf = s.peak;
  } else {
    const float sy = p.sh * Y, sx = p.sw * X;
    const int ya = min((int)sy, p.h - 1), xa = min((int)sx, p.w - 1);
    const int yb = ya + (ya < p.h - 1 ? 1 : 0), xb = xa + (xa < p.w - 1 ? 1 : 0);
    const float h1 = sy - (float)ya, h0 = 1.0f - h1, w1 = sx - (float)xa, w0 = 1.0f - w1;
    const Src3 s[4] = {fetch(ya, xa), fetch(ya, xb), fetch(yb, xa), fetch(yb, xb)};
    const double wt[4] = {(double)h0 * w0, (double)h0 * w1, (double)h1 * w0, (double)h1 * w1};
    double m = 0.0;
    cf = 0.0;
#pragma unroll
    for (int t = 0; t < 4; ++t) { m += wt[t] * s[t].mean; cf += wt[t] * s[t].peak; }      // (all four terms always: 0 * NaN = NaN, as in the depth map)
    var = 0.0;
#pragma unroll
    for (int t = 0; t < 4; ++t) { const double e = s[t].mean - m; var += wt[t] * (s[t].var + e * e); }
  }
  Fin2 r;
  r.sd = (float)__builtin_sqrt(var);
  r.cf = (float)cf;
  if (r.sd != r.sd) r.sd = p.span;
  if (r.cf != r.cf) r.cf = 0.f;
  return r;
}

__device__ __forceinline__ void store8f(float* dst, long o, const float (&v)[8]) {
  *reinterpret_cast<float4*>(dst + o) = make_float4(v[0], v[1], v[2], v[3]);
  *reinterpret_cast<float4*>(dst + o + 4) = make_float4(v[4], v[5], v[6], v[7]);
}

constexpr int STAGE_PIXELS = STAGE_FLOATS;       // the same source window as the depth kernel's tile, three numbers per pixel

__global__ __launch_bounds__(256) void depth_finalize_stats_tile_kernel(FinStatsArgs p, int tiles_x) {
  __shared__ Src3 src[STAGE_PIXELS];
  const int tid = threadIdx.x;
  const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
  const long base = (long)blockIdx.y * p.h * p.w;
  const int Y0 = ty * TILE_H, X0 = tx * TILE_W;
  const int Yl = min(Y0 + TILE_H, p.H) - 1, Xl = min(X0 + TILE_W, p.W) - 1;
  const int r0 = min((int)(p.sh * Y0), p.h - 1), r1 = min(min((int)(p.sh * Yl), p.h - 1) + 1, p.h - 1);
  const int c0 = min((int)(p.sw * X0), p.w - 1), c1 = min(min((int)(p.sw * Xl), p.w - 1) + 1, p.w - 1);
  const int nr = r1 - r0 + 1, nc = c1 - c0 + 1;
  const bool staged = nr * nc <= STAGE_PIXELS;                   // uniform over the workgroup
  if (staged) {
    for (int i = tid; i < nr * nc; i += 256) {
      const int r = i / nc, c = i - r * nc;
      src[i] = tap3(p, base, r0 + r, c0 + c);
    }
  }
  __syncthreads();
  const int Y = Y0 + (tid >> 4), X = X0 + ((tid & 15) << 3);
  if (Y >= p.H || X >= p.W) return;
  float sd[8], cf[8];
  if (staged) {
    auto fetch = [&](int y, int x) { return src[(y - r0) * nc + (x - c0)]; };
#pragma unroll
    for (int i = 0; i < 8; ++i) { const Fin2 f = final_stats(p, fetch, Y, X + i); sd[i] = f.sd; cf[i] = f.cf; }
  } else {
    auto fetch = [&](int y, int x) { return tap3(p, base, y, x); };
#pragma unroll
    for (int i = 0; i < 8; ++i) { const Fin2 f = final_stats(p, fetch, Y, X + i); sd[i] = f.sd; cf[i] = f.cf; }
  }
  const long o = (long)blockIdx.y * p.H * p.W + (long)Y * p.W + X;
  if (p.std_out != nullptr) store8f(p.std_out, o, sd);
  if (p.conf != nullptr) store8f(p.conf, o, cf);
}

template <int V>
__global__ __launch_bounds__(256) void depth_finalize_stats_kernel(FinStatsArgs p) {
  const long P = (long)p.H * p.W;
  const long groups = P / V, total = groups * p.B;
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
    const long b = t / groups, pix0 = (t - b * groups) * V;
    const long base = b * (long)p.h * p.w;
    auto fetch = [&](int y, int x) { return tap3(p, base, y, x); };
    int Y = (int)(pix0 / p.W), X = (int)(pix0 - (long)Y * p.W);
    float sd[V], cf[V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const Fin2 f = final_stats(p, fetch, Y, X);
      sd[i] = f.sd; cf[i] = f.cf;
      if (++X == p.W) { X = 0; ++Y; }
    }
    const long o = b * P + pix0;
    if constexpr (V == 8) {
      if (p.std_out != nullptr) store8f(p.std_out, o, sd);
      if (p.conf != nullptr) store8f(p.conf, o, cf);
    } else {
      if (p.std_out != nullptr) p.std_out[o] = sd[0];
      if (p.conf != nullptr) p.conf[o] = cf[0];
    }
  }
}

}  // namespace

extern "C" int ocv_depth_finalize_fwd(const float* pred, const float* pred_mirror, int h, int w, float min_depth, float max_depth,
                                      int H, int W, float* depth, uint16_t* depth_u16, float u16_scale, uint8_t* rgb8,
                                      const uint8_t* colormap, float vmin, float colormap_scale, int B, ocv_stream_t stream) {
  OCV_CHECK_ARG(pred, "ocv_depth_finalize_fwd: null pointer (pred)");
  OCV_CHECK_ARG(depth || depth_u16 || rgb8, "ocv_depth_finalize_fwd: null pointer (at least one of depth, depth_u16, rgb8 must be given)");
  OCV_CHECK_ARG(!rgb8 || colormap, "ocv_depth_finalize_fwd: null pointer (rgb8 needs the [256][3] colour table)");
  OCV_CHECK_ARG(B >= 1 && h >= 1 && w >= 1 && H >= 1 && W >= 1, "ocv_depth_finalize_fwd: bad sizes (B, h, w, H, W must be >= 1)");
  OCV_CHECK_ARG(min_depth < max_depth, "ocv_depth_finalize_fwd: min_depth must be below max_depth");
  OCV_CHECK_ARG(!depth_u16 || u16_scale > 0.f, "ocv_depth_finalize_fwd: u16_scale must be positive");
  OCV_CHECK_ARG(!rgb8 || (colormap_scale > 0.f && vmin == vmin), "ocv_depth_finalize_fwd: colormap_scale = 256 / (vmax - vmin) must be positive");
  OCV_CHECK_ARG((reinterpret_cast<uintptr_t>(depth) & 3) == 0 && (reinterpret_cast<uintptr_t>(depth_u16) & 1) == 0,
                "ocv_depth_finalize_fwd: misaligned output");
  FinArgs a{pred, pred_mirror, depth, depth_u16, rgb8, colormap, h, w, H, W, B,
            H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.f, W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.f, min_depth, max_depth,
            u16_scale, vmin, colormap_scale};
  const long P = (long)H * W;
  const bool vec = (P & 7) == 0 && (reinterpret_cast<uintptr_t>(depth) & 15) == 0 && (reinterpret_cast<uintptr_t>(depth_u16) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(rgb8) & 7) == 0;
  hipStream_t st = (hipStream_t)stream;
  const int tiles_x = (W + TILE_W - 1) / TILE_W, tiles_y = (H + TILE_H - 1) / TILE_H;
  if (vec && (W & 7) == 0 && !(h == H && w == W) && B <= 65535 && (long)tiles_x * tiles_y <= 0x7fffffffL) {
    hipLaunchKernelGGL(depth_finalize_tile_kernel, dim3(tiles_x * tiles_y, B), dim3(256), 0, st, a, tiles_x);
  } else {
    const long threads = vec ? P / 8 * B : P * B;
    long grid = (threads + 255) / 256;
    if (grid > 8192) grid = 8192;
    if (vec) hipLaunchKernelGGL(depth_finalize_kernel<8>, dim3((int)grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(depth_finalize_kernel<1>, dim3((int)grid), dim3(256), 0, st, a);
  }
  OCV_CHECK_LAUNCH("ocv_depth_finalize_fwd");
  return 0;
}

extern "C" int ocv_depth_finalize_stats_fwd(const float* pred, const float* pred_mirror, const float* var, const float* var_mirror,
                                            const float* pmax, const float* pmax_mirror, int h, int w, float min_depth, float max_depth,
                                            int H, int W, float* depth_std, float* confidence, int B, ocv_stream_t stream) {
  OCV_CHECK_ARG(depth_std || confidence, "ocv_depth_finalize_stats_fwd: null pointer (at least one of depth_std, confidence must be given)");
  OCV_CHECK_ARG(!depth_std || (pred && var), "ocv_depth_finalize_stats_fwd: null pointer (depth_std needs pred and var)");
  OCV_CHECK_ARG(!confidence || pmax, "ocv_depth_finalize_stats_fwd: null pointer (confidence needs pmax)");
  const bool tta = pred_mirror || var_mirror || pmax_mirror;
  OCV_CHECK_ARG(!tta || ((!depth_std || (pred_mirror && var_mirror)) && (!confidence || pmax_mirror)),
                "ocv_depth_finalize_stats_fwd: null pointer (with flip-TTA every map that is read needs its mirror)");
  OCV_CHECK_ARG(B >= 1 && h >= 1 && w >= 1 && H >= 1 && W >= 1, "ocv_depth_finalize_stats_fwd: bad sizes (B, h, w, H, W must be >= 1)");
  OCV_CHECK_ARG(min_depth < max_depth, "ocv_depth_finalize_stats_fwd: min_depth must be below max_depth");
  OCV_CHECK_ARG((reinterpret_cast<uintptr_t>(depth_std) & 3) == 0 && (reinterpret_cast<uintptr_t>(confidence) & 3) == 0,
                "ocv_depth_finalize_stats_fwd: misaligned output");
  // (mirror: the flag of the TTA form for both outputs; a map that is not read may stay null)
  FinStatsArgs a{pred, tta ? (pred_mirror ? pred_mirror : pmax_mirror) : nullptr, var, var_mirror, pmax, pmax_mirror, depth_std, confidence,
                 h, w, H, W, B, H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.f, W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.f,
                 max_depth - min_depth};
  const long P = (long)H * W;
  const bool vec = (P & 7) == 0 && (reinterpret_cast<uintptr_t>(depth_std) & 15) == 0 && (reinterpret_cast<uintptr_t>(confidence) & 15) == 0;
  hipStream_t st = (hipStream_t)stream;
  const int tiles_x = (W + TILE_W - 1) / TILE_W, tiles_y = (H + TILE_H - 1) / TILE_H;
  if (vec && (W & 7) == 0 && !(h == H && w == W) && B <= 65535 && (long)tiles_x * tiles_y <= 0x7fffffffL) {
    hipLaunchKernelGGL(depth_finalize_stats_tile_kernel, dim3(tiles_x * tiles_y, B), dim3(256), 0, st, a, tiles_x);
  } else {
    const long threads = vec ? P / 8 * B : P * B;
    long grid = (threads + 255) / 256;
    if (grid > 8192) grid = 8192;
    if (vec) hipLaunchKernelGGL(depth_finalize_stats_kernel<8>, dim3((int)grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(depth_finalize_stats_kernel<1>, dim3((int)grid), dim3(256), 0, st, a);
  }
  OCV_CHECK_LAUNCH("ocv_depth_finalize_stats_fwd");
  return 0;
}
