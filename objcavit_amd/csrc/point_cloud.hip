// Point-cloud output behind the predict path's final map: depth map -> compacted 3-D points in the camera frame.
//   depth [B][1][H][W] (+ confidence, depth_std), K [B][4] = fx, fy, cx, cy in pixels of the map's grid (+ the uint8 frames the map was
//   made from, for the colour) -> points [B][cap][4] (16-byte records X, Y, Z, RGBA), pixel [B][cap], counts [B], total [B]
// A deterministic, filtered STREAM COMPACTION with a pinhole back-projection (the definition is in include/objcavit_hip.h).  Two launches
// over one grid, one 256-thread workgroup per (image, tile); a tile is 2048 consecutive candidates of the strided pixel grid in row-major
// order, taken as eight rounds of 256 consecutive candidates (coalesced 4-byte loads, eight in flight):
//   count   evaluates the predicate, counts the keepers of a tile (ballot + popcount per wave and round, the waves' sums through LDS)
//           and writes ONE int32 per tile into the workspace [B][T];
//   write   sums the counts of the tiles in front of its own (one load per thread and 256 tiles + a reduction), evaluates the predicate
//           again, ranks the keepers of a round by ballot + mbcnt, and stores every record with ONE 16-byte store at base + rank:
//           consecutive keepers land in consecutive records, a wave's stores are contiguous.  The last tile's workgroup writes total
//           and counts.
// No workgroup waits for another, nothing is read on the host, there is no atomic: integer sums in any order are exact, so two calls
// give identical bytes.  rx = (x - cx) / fx and ry = (y - cy) / fy are evaluated by the thread that keeps a pixel (two IEEE divisions
// per kept point, ~25 VALU instructions against 20 - 40 bytes of memory traffic: the launch is bound by its traffic).
#include "common.hpp"
#include "../../include/objcavit_hip.h"
#include "keep_pixel.hpp"

#include <float.h>

namespace {

constexpr int UP_THREADS = 256, UP_WAVES = UP_THREADS / OCV_WAVE, UP_ROUNDS = 8, UP_TILE = UP_THREADS * UP_ROUNDS;
static_assert(UP_TILE == OCV_UNPROJECT_TILE, "the workspace formula of the header is this kernel's tile");

struct UnprojectArgs {
  const float *depth, *K, *conf, *std;
  const uint8_t* frames;
  long frame_stride, row_stride;      // bytes
  float* points;                      // [B][cap][4]
  int *pixel, *counts, *total, *tiles;
  int H, W, sy, sx, Wc, T, cap, top, left;
  int step_y, step_x;                 // 256 / Wc, 256 % Wc: a thread's candidate moves by these from one round to the next
  unsigned N;                         // candidates per image = ceil(H / sy) * ceil(W / sx)
  float near, far, min_conf, max_std;
};

// The keepers of the calling thread's eight candidates of tile t of image b: bit r of the result = round r; z / cf / off of a keeper are
// its depth, its confidence (1 without a map) and its pixel index y * W + x.  Everything the two kernels must agree on is here.
__device__ __forceinline__ unsigned up_evaluate(const UnprojectArgs& p, int b, int t, int tid, float (&z)[UP_ROUNDS], float (&cf)[UP_ROUNDS],
                                                int (&off)[UP_ROUNDS]) {
  const float4 k = *reinterpret_cast<const float4*>(p.K + 4 * (long)b);
  const bool camera = up_camera_ok(k);                                      // (keep_pixel.hpp: the rule the ground grid shares)
  const long plane = (long)b * p.H * p.W;
  const unsigned c0 = (unsigned)t * UP_TILE + tid;
  int yc = (int)(c0 / (unsigned)p.Wc), xc = (int)(c0 - (unsigned)yc * p.Wc);
  bool in[UP_ROUNDS];
#pragma unroll
  for (int r = 0; r < UP_ROUNDS; ++r) {
    in[r] = camera && c0 + (unsigned)(r * UP_THREADS) < p.N;
    off[r] = in[r] ? yc * p.sy * p.W + xc * p.sx : 0;                        // (H * W < 2^31: the entry point checks it)
    yc += p.step_y;
    xc += p.step_x;
    if (xc >= p.Wc) { xc -= p.Wc; ++yc; }
  }
  const float nan = __uint_as_float(0x7fc00000u);
  float sd[UP_ROUNDS];
#pragma unroll
  for (int r = 0; r < UP_ROUNDS; ++r) z[r] = in[r] ? p.depth[plane + off[r]] : nan;
#pragma unroll
  for (int r = 0; r < UP_ROUNDS; ++r) cf[r] = (in[r] && p.conf != nullptr) ? p.conf[plane + off[r]] : 1.f;
#pragma unroll
  for (int r = 0; r < UP_ROUNDS; ++r) sd[r] = (in[r] && p.std != nullptr) ? p.std[plane + off[r]] : 0.f;
  unsigned keep = 0u;
#pragma unroll
  for (int r = 0; r < UP_ROUNDS; ++r) {
    const bool on = up_keep(in[r], z[r], cf[r], sd[r], p.conf != nullptr, p.std != nullptr, p.near, p.far, p.min_conf, p.max_std);
    keep |= on ? 1u << r : 0u;
  }
  return keep;
}

__global__ __launch_bounds__(UP_THREADS) void unproject_count_kernel(UnprojectArgs p) {
  __shared__ int s_n[UP_WAVES];
  const int tid = threadIdx.x, lane = tid & (OCV_WAVE - 1), wave = tid / OCV_WAVE;
  const int b = blockIdx.x / p.T, t = blockIdx.x - b * p.T;
  float z[UP_ROUNDS], cf[UP_ROUNDS];
  int off[UP_ROUNDS];
  const unsigned keep = up_evaluate(p, b, t, tid, z, cf, off);
  int n = 0;
#pragma unroll
  for (int r = 0; r < UP_ROUNDS; ++r) n += __popcll(__ballot((keep >> r) & 1u));
  if (lane == 0) s_n[wave] = n;
  __syncthreads();
  if (tid == 0) {
    int sum = 0;
#pragma unroll
    for (int w = 0; w < UP_WAVES; ++w) sum += s_n[w];
    p.tiles[blockIdx.x] = sum;
  }
}

__global__ __launch_bounds__(UP_THREADS) void unproject_write_kernel(UnprojectArgs p) {
  __shared__ int s_n[UP_ROUNDS][UP_WAVES];
  __shared__ int s_before[UP_WAVES];
  const int tid = threadIdx.x, lane = tid & (OCV_WAVE - 1), wave = tid / OCV_WAVE;
  const int b = blockIdx.x / p.T, t = blockIdx.x - b * p.T;

  // the keepers of the tiles in front of this one
  int before = 0;
  for (int i = tid; i < t; i += UP_THREADS) before += p.tiles[b * p.T + i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o, OCV_WAVE);
  if (lane == 0) s_before[wave] = before;

  float z[UP_ROUNDS], cf[UP_ROUNDS];
  int off[UP_ROUNDS];
  const unsigned keep = up_evaluate(p, b, t, tid, z, cf, off);
  int rank[UP_ROUNDS];
#pragma unroll
  for (int r = 0; r < UP_ROUNDS; ++r) {
    const unsigned long long m = __ballot((keep >> r) & 1u);
    rank[r] = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));   // keepers in lower lanes
    if (lane == 0) s_n[r][wave] = __popcll(m);
  }
  __syncthreads();

  // record index of this wave's first keeper of every round: rounds in order, within a round the waves in order
  int run = 0;
#pragma unroll
  for (int w = 0; w < UP_WAVES; ++w) run += s_before[w];
#pragma unroll
  for (int r = 0; r < UP_ROUNDS; ++r) {
#pragma unroll
    for (int w = 0; w < UP_WAVES; ++w) {
      if (w == wave) rank[r] += run;                                         // rank -> record index
      run += s_n[r][w];
    }
  }
  if (t == p.T - 1 && tid == 0) {                                            // run = every keeper of the image
    p.total[b] = run;
    p.counts[b] = min(run, p.cap);
  }
  if (keep == 0u) return;

  const float4 k = *reinterpret_cast<const float4*>(p.K + 4 * (long)b);
  const long row0 = (long)b * p.cap;
#pragma unroll
  for (int r = 0; r < UP_ROUNDS; ++r) {
    const int idx = rank[r];
    if (!((keep >> r) & 1u) || idx >= p.cap) continue;
    const int y = off[r] / p.W, x = off[r] - y * p.W;
    // every statement rounded to fp32 on its own (the library is built with contraction on); `/` is the IEEE division
    const float rx = __fsub_rn((float)x, k.z) / k.x;
    const float ry = __fsub_rn((float)y, k.w) / k.y;
    unsigned rgba = 0u;
    if (p.frames != nullptr) {
      const uint8_t* s = p.frames + b * p.frame_stride + (long)(p.top + y) * p.row_stride + (long)(p.left + x) * 3;
      rgba = (unsigned)s[0] | ((unsigned)s[1] << 8) | ((unsigned)s[2] << 16);
    }
    const unsigned alpha = p.conf != nullptr ? (unsigned)rintf(__fmul_rn(255.f, fminf(fmaxf(cf[r], 0.f), 1.f))) : 255u;
    rgba |= alpha << 24;
    *reinterpret_cast<float4*>(p.points + 4 * (row0 + idx)) =
        make_float4(__fmul_rn(rx, z[r]), __fmul_rn(ry, z[r]), z[r], __uint_as_float(rgba));
    if (p.pixel != nullptr) p.pixel[row0 + idx] = off[r];
  }
}

long up_tiles(int H, int W, int sy, int sx) {
  const long n = (long)ocv_cdiv(H, sy) * ocv_cdiv(W, sx);
  return (n + UP_TILE - 1) / UP_TILE;
}

bool up_sizes_ok(int B, int H, int W, int sy, int sx) {
  return B >= 1 && H >= 1 && W >= 1 && sy >= 1 && sx >= 1 && (long)H * W <= 0x7fffffffL && (long)B * up_tiles(H, W, sy, sx) <= 0x7fffffffL;
}

}  // namespace

extern "C" size_t ocv_depth_unproject_workspace_bytes(int B, int H, int W, int sy, int sx) {
  if (!up_sizes_ok(B, H, W, sy, sx)) return 0;
  return (size_t)B * (size_t)up_tiles(H, W, sy, sx) * sizeof(int);
}

extern "C" int ocv_depth_unproject_fwd(const float* depth, const float* K, const float* confidence, const float* depth_std,
                                       const uint8_t* frames, long frame_stride, long row_stride, int Hs, int Ws, int top, int left,
                                       int B, int H, int W, int sy, int sx, float near, float far, float min_confidence, float max_std,
                                       int cap, float* points, int* pixel, int* counts, int* total, void* workspace,
                                       size_t workspace_bytes, ocv_stream_t stream) {
  OCV_CHECK_ARG(depth && K && points && counts && total && workspace,
                "ocv_depth_unproject_fwd: null pointer (depth, K, points, counts, total, workspace)");
  OCV_CHECK_ARG(B >= 1 && H >= 1 && W >= 1, "ocv_depth_unproject_fwd: bad sizes (B, H, W must be >= 1)");
  OCV_CHECK_ARG(sy >= 1 && sx >= 1, "ocv_depth_unproject_fwd: stride (%d, %d) must be >= 1", sy, sx);
  OCV_CHECK_ARG(up_sizes_ok(B, H, W, sy, sx), "ocv_depth_unproject_fwd: bad sizes (H * W and B * tiles below 2^31)");
  OCV_CHECK_ARG(cap >= 1, "ocv_depth_unproject_fwd: capacity = %d must be >= 1", cap);
  OCV_CHECK_ARG((long)B * cap <= 0x7fffffffL, "ocv_depth_unproject_fwd: bad sizes (B * capacity below 2^31)");
  OCV_CHECK_ARG(near <= far, "ocv_depth_unproject_fwd: near = %g must be <= far = %g", (double)near, (double)far);
  if (frames != nullptr) {
    OCV_CHECK_ARG(Hs >= 1 && Ws >= 1 && top >= 0 && left >= 0 && (long)top + H <= Hs && (long)left + W <= Ws,
                  "ocv_depth_unproject_fwd: window %d x %d at (%d, %d) outside the %d x %d frame", H, W, top, left, Hs, Ws);
    OCV_CHECK_ARG(row_stride >= (long)Ws * 3 && (B == 1 || frame_stride >= (long)(Hs - 1) * row_stride + (long)Ws * 3),
                  "ocv_depth_unproject_fwd: strides (bytes) smaller than a row / a frame");
  }
  const size_t need = ocv_depth_unproject_workspace_bytes(B, H, W, sy, sx);
  OCV_CHECK_ARG(workspace_bytes >= need, "ocv_depth_unproject_fwd: workspace too small (%zu bytes, need %zu)", workspace_bytes, need);
  OCV_CHECK_ARG(ocv_aligned16(points) && ocv_aligned16(K), "ocv_depth_unproject_fwd: points / K must be 16-byte aligned");
  OCV_CHECK_ARG(((reinterpret_cast<uintptr_t>(depth) | reinterpret_cast<uintptr_t>(confidence) | reinterpret_cast<uintptr_t>(depth_std) |
                  reinterpret_cast<uintptr_t>(pixel) | reinterpret_cast<uintptr_t>(counts) | reinterpret_cast<uintptr_t>(total) |
                  reinterpret_cast<uintptr_t>(workspace)) & 3) == 0, "ocv_depth_unproject_fwd: misaligned pointer");
  UnprojectArgs a{};
  a.depth = depth; a.K = K; a.conf = confidence; a.std = depth_std;
  a.frames = frames; a.frame_stride = frames ? frame_stride : 0; a.row_stride = frames ? row_stride : 0;
  a.points = points; a.pixel = pixel; a.counts = counts; a.total = total; a.tiles = static_cast<int*>(workspace);
  a.H = H; a.W = W; a.sy = sy; a.sx = sx; a.Wc = ocv_cdiv(W, sx); a.T = (int)up_tiles(H, W, sy, sx); a.cap = cap;
  a.top = frames ? top : 0; a.left = frames ? left : 0;
  a.step_y = UP_THREADS / a.Wc; a.step_x = UP_THREADS % a.Wc;
  a.N = (unsigned)((long)ocv_cdiv(H, sy) * a.Wc);
  a.near = near; a.far = far; a.min_conf = min_confidence; a.max_std = max_std;
  const dim3 grid((unsigned)((long)B * a.T));
  hipLaunchKernelGGL(unproject_count_kernel, grid, dim3(UP_THREADS), 0, (hipStream_t)stream, a);
  OCV_CHECK_LAUNCH("ocv_depth_unproject_fwd (count)");
  hipLaunchKernelGGL(unproject_write_kernel, grid, dim3(UP_THREADS), 0, (hipStream_t)stream, a);
  OCV_CHECK_LAUNCH("ocv_depth_unproject_fwd (write)");
  return 0;
}
