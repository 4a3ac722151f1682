// Bird's-eye occupancy grid behind the predict path's final map (DESIGN.md section 6b "Ground grid", STATEMENT G of include/objcavit_hip.h):
//   depth [B][1][H][W] (+ confidence, depth_std), K [B][4], pose [B][12] = [R | t] camera -> ground frame
//   -> per cell of a GX x GY grid: count, obstacle, h_min, h_max, h_mean, state; per lateral column: first_occupied
// A SCATTER (everything else here gathers or compacts): every kept pixel is a point that lands in one cell.  Three launches:
//   clear       zero fill of the per-cell records in the workspace (ocv_zero_async: a launch, not a memset node).  The records are
//               made so that all-zero means "empty": the minimum is kept as the maximum of the COMPLEMENT of the float's key.
//   accumulate  one 256-thread workgroup per (image, tile); a tile is GG_TILE = 1024 consecutive candidates of the strided pixel grid in
//               row-major order, four rounds of 256 (coalesced 4-byte loads).  1024 because a point's height is at most 2^20 in units
//               of 1 / 1024 m (the band's bound), so a tile's height sum fits an int32 and the on-chip arithmetic is 32-bit.  The
//               tile's points are merged ON CHIP before anything leaves the CU:
//                 1. in a wave, runs of consecutive lanes with the same cell -- neighbouring pixels of a row on near ground or on a
//                    wall -- are combined by a segmented reduction (one ballot of the run heads, six steps of four shuffles);
//                 2. the run leaders insert into an LDS table keyed by cell: GG_SLOTS = 1024 slots (as many as a tile can have
//                    distinct cells; the keys and four 4-byte value arrays, 20 KB, so the eight workgroups a CU's wave slots allow
//                    fit its 160 KB), open addressing with linear probing, at most GG_PROBES = 8 probes, LDS integer atomics
//                    (compare-and-swap on the key; add / max on the values).
//               At the end of the tile every occupied slot issues ONE set of global atomics.  A leader whose probes all hit other
//               cells goes straight to the global records: correctness does not depend on the table's size.
//   finalize    a coalesced pass over the B * GX * GY records into the given outputs, and, in further workgroups of the same launch,
//               the column scan: 16 columns x 16 row phases per workgroup (each thread walks iy = phase, phase + 16, ... with eight
//               independent loads in flight, reads coalesced across ix), the phases' minima joined through LDS.  It reads the
//               records, not the state output, so it needs no launch of its own.
// INTEGER ATOMICS ONLY: counts are integer adds, the extremes unsigned max on the order-preserving integer image of the float, the
// height sum a 64-bit integer add of rint(1024 h) (exact: a power-of-two product).  Integer sums and extremes do not depend on the
// order of arrival, so two calls give identical bytes.  No allocation, no synchronisation, nothing read on the host: capturable.
// The keep rule is the point cloud's (keep_pixel.hpp).  Every per-point operation is fp32 and rounded on its own (__fmul_rn & co., and
// gg_mul of rounded_mul.hpp where a product feeds a sum: the library is built with contraction on); `/` is the IEEE division.
#include "common.hpp"
#include "float_key.hpp"
#include "keep_pixel.hpp"
#include "rounded_mul.hpp"
#include "seg_reduce.hpp"
#include "../../include/objcavit_hip.h"

#include <math.h>

namespace {

constexpr int GG_THREADS = 256, GG_ROUNDS = 4, GG_TILE = GG_THREADS * GG_ROUNDS;
constexpr int GG_LOG_SLOTS = 10, GG_SLOTS = 1 << GG_LOG_SLOTS, GG_PROBES = 8;
constexpr int GG_COLS = 16, GG_PHASES = GG_THREADS / GG_COLS, GG_AHEAD = 8;
constexpr int GG_MAX_SIDE = 1 << 24;                     // GX, GY exact as fp32
static_assert(GG_TILE == OCV_GROUND_GRID_TILE, "the header names this kernel's tile");
static_assert((long)GG_TILE << 20 <= 0x40000000L, "a tile's height sum must fit an int32");
static_assert(GG_TILE < (1 << 16), "count and obstacle of a tile share one 32-bit word");

struct GridRecords {                                     // the workspace: [B * cells] of each, all-zero = empty
  long long* sum;                                        // of rint(1024 h)
  int *count, *obstacle;
  unsigned *nmin, *max;                                  // ~key(h) and key(h): both joined by max
};

struct GridArgs {
  const float *depth, *K, *pose, *conf, *std;
  GridRecords rec;
  int H, W, sy, sx, Wc, T, GX, GY;
  unsigned N;                                            // candidates per image
  int cells;                                             // GX * GY
  float near, far, min_conf, max_std, x0, y0, cell, lo, hi, obstacle_height;
};

struct FinalArgs {
  GridRecords rec;
  int *count, *obstacle;
  float *h_min, *h_max, *h_mean, *first;
  uint8_t* state;
  int B, GX, GY, cells, min_points, min_obstacle, cell_blocks, col_groups;
  long n;                                                // B * cells
  float y0, cell;
};

__device__ __forceinline__ int gg_state(int count, int obstacle, int min_points, int min_obstacle) {
  return count < min_points ? 0 : (obstacle >= min_obstacle ? 2 : 1);
}

// one set of global atomics: `packed` = count | obstacle << 16 of the points joined so far
__device__ __forceinline__ void gg_global(const GridRecords& r, long at, int packed, unsigned nmin, unsigned mx, int sum) {
  atomicAdd(r.count + at, packed & 0xffff);
  if (packed >> 16) atomicAdd(r.obstacle + at, packed >> 16);
  atomicMax(r.nmin + at, nmin);
  atomicMax(r.max + at, mx);
  atomicAdd(reinterpret_cast<unsigned long long*>(r.sum + at), (unsigned long long)(long long)sum);
}

__global__ __launch_bounds__(GG_THREADS) void grid_accumulate_kernel(GridArgs p) {
  __shared__ unsigned s_key[GG_SLOTS], s_nmin[GG_SLOTS], s_max[GG_SLOTS];
  __shared__ int s_packed[GG_SLOTS], s_sum[GG_SLOTS];
  const int tid = threadIdx.x, lane = tid & (OCV_WAVE - 1);
  const int b = blockIdx.x / p.T, t = blockIdx.x - b * p.T;
  const float4 k = *reinterpret_cast<const float4*>(p.K + 4 * (long)b);
  const float4 p0 = *reinterpret_cast<const float4*>(p.pose + 12 * (long)b);
  const float4 p1 = *reinterpret_cast<const float4*>(p.pose + 12 * (long)b + 4);
  const float4 p2 = *reinterpret_cast<const float4*>(p.pose + 12 * (long)b + 8);
  const bool posed = up_finite(p0.x) && up_finite(p0.y) && up_finite(p0.z) && up_finite(p0.w) && up_finite(p1.x) && up_finite(p1.y) &&
                     up_finite(p1.z) && up_finite(p1.w) && up_finite(p2.x) && up_finite(p2.y) && up_finite(p2.z) && up_finite(p2.w);
  if (!(up_camera_ok(k) && posed)) return;               // (the whole workgroup: b is its image) the image keeps nothing
  for (int i = tid; i < GG_SLOTS; i += GG_THREADS) {
    s_key[i] = 0u; s_nmin[i] = 0u; s_max[i] = 0u; s_packed[i] = 0; s_sum[i] = 0;
  }
  __syncthreads();
  const long plane = (long)b * p.H * p.W, base = (long)b * p.cells;
  const float gx = (float)p.GX, gy = (float)p.GY;
#pragma unroll
  for (int r = 0; r < GG_ROUNDS; ++r) {
    const unsigned c = (unsigned)t * GG_TILE + (unsigned)(r * GG_THREADS + tid);
    const bool in = c < p.N;
    const int yc = (int)(c / (unsigned)p.Wc), xc = (int)(c - (unsigned)yc * p.Wc);
    const int y = yc * p.sy, x = xc * p.sx;
    const long off = in ? plane + (long)y * p.W + x : 0;  // (H * W < 2^31: the entry point checks it)
    const float z = in ? p.depth[off] : 0.f;
    const float cf = (in && p.conf != nullptr) ? p.conf[off] : 1.f;
    const float sd = (in && p.std != nullptr) ? p.std[off] : 0.f;
    int cell = -1, packed = 0, sum = 0;
    unsigned nmin = 0u, mx = 0u;
    if (up_keep(in, z, cf, sd, p.conf != nullptr, p.std != nullptr, p.near, p.far, p.min_conf, p.max_std)) {
      const float rx = __fsub_rn((float)x, k.z) / k.x, ry = __fsub_rn((float)y, k.w) / k.y;
      const float X = __fmul_rn(rx, z), Y = __fmul_rn(ry, z);
      const float g0 = __fadd_rn(__fadd_rn(__fadd_rn(gg_mul(p0.x, X), gg_mul(p0.y, Y)), gg_mul(p0.z, z)), p0.w);
      const float g1 = __fadd_rn(__fadd_rn(__fadd_rn(gg_mul(p1.x, X), gg_mul(p1.y, Y)), gg_mul(p1.z, z)), p1.w);
      const float g2 = __fadd_rn(__fadd_rn(__fadd_rn(gg_mul(p2.x, X), gg_mul(p2.y, Y)), gg_mul(p2.z, z)), p2.w);
      const float fxi = floorf(__fsub_rn(g0, p.x0) / p.cell), fyi = floorf(__fsub_rn(g1, p.y0) / p.cell);
      if (fxi >= 0.f && fxi < gx && fyi >= 0.f && fyi < gy && p.lo <= g2 && g2 <= p.hi) {      // (NaN fails every comparison)
        cell = (int)fyi * p.GX + (int)fxi;               // < GX * GY: fxi, fyi are whole numbers below GX, GY <= 2^24
        packed = 1 | (g2 > p.obstacle_height ? 1 << 16 : 0);
        mx = gg_key(g2);
        nmin = ~mx;
        sum = (int)rintf(__fmul_rn(g2, 1024.f));         // |g2| <= 1000: at most 2^20, exact
      }
    }
    if (__ballot(cell >= 0) == 0ull) continue;           // (wave-uniform)
    // 1. runs of consecutive lanes with the same cell: the run's first lane ends up with the run's join
    const SegRuns runs = seg_runs(cell, lane);             // (seg_reduce.hpp, shared with csrc/obstacles.hip)
    seg_reduce(runs, lane, [&](int o, bool take) {
      const int packed_o = __shfl_down(packed, o, OCV_WAVE), sum_o = __shfl_down(sum, o, OCV_WAVE);
      const unsigned nmin_o = __shfl_down(nmin, o, OCV_WAVE), mx_o = __shfl_down(mx, o, OCV_WAVE);
      if (take) {                                          // lane + o is of this lane's run
        packed += packed_o; sum += sum_o;
        nmin = max(nmin, nmin_o); mx = max(mx, mx_o);
      }
    });
    // 2. the leaders insert
    if (runs.head && cell >= 0) {
      unsigned slot = ((unsigned)cell * 2654435761u) >> (32 - GG_LOG_SLOTS);
      bool placed = false;
      for (int probe = 0; probe < GG_PROBES && !placed; ++probe) {
        const unsigned old = atomicCAS(&s_key[slot], 0u, (unsigned)cell + 1u);
        if (old == 0u || old == (unsigned)cell + 1u) {
          atomicAdd(&s_packed[slot], packed);
          atomicAdd(&s_sum[slot], sum);
          atomicMax(&s_nmin[slot], nmin);
          atomicMax(&s_max[slot], mx);
          placed = true;
        } else {
          slot = (slot + 1u) & (GG_SLOTS - 1);
        }
      }
      if (!placed) gg_global(p.rec, base + cell, packed, nmin, mx, sum);
    }
  }
  __syncthreads();
  for (int i = tid; i < GG_SLOTS; i += GG_THREADS) {
    const unsigned key = s_key[i];
    if (key != 0u) gg_global(p.rec, base + (long)(key - 1u), s_packed[i], s_nmin[i], s_max[i], s_sum[i]);
  }
}

__global__ __launch_bounds__(GG_THREADS) void grid_finalize_kernel(FinalArgs p) {
  __shared__ int s_first[GG_PHASES][GG_COLS];
  const int tid = threadIdx.x;
  if ((int)blockIdx.x < p.cell_blocks) {                 // the records -> the per-cell outputs
    const long i = (long)blockIdx.x * GG_THREADS + tid;
    if (i >= p.n) return;
    const int count = p.rec.count[i], obstacle = p.rec.obstacle[i];
    if (p.count != nullptr) p.count[i] = count;
    if (p.obstacle != nullptr) p.obstacle[i] = obstacle;
    if (p.h_min != nullptr) p.h_min[i] = count > 0 ? gg_unkey(~p.rec.nmin[i]) : 0.f;
    if (p.h_max != nullptr) p.h_max[i] = count > 0 ? gg_unkey(p.rec.max[i]) : 0.f;
    if (p.h_mean != nullptr) p.h_mean[i] = count > 0 ? (float)((double)p.rec.sum[i] / (1024.0 * (double)count)) : 0.f;
    if (p.state != nullptr) p.state[i] = (uint8_t)gg_state(count, obstacle, p.min_points, p.min_obstacle);
    return;
  }
  // the column scan: workgroup = (image, 16 columns), thread = (row phase, column)
  const int g = (int)blockIdx.x - p.cell_blocks, b = g / p.col_groups, ix = (g - b * p.col_groups) * GG_COLS + (tid & (GG_COLS - 1));
  const int phase = tid / GG_COLS;
  int first = 0x7fffffff;
  if (ix < p.GX) {
    const long at = (long)b * p.cells + ix;
    for (int iy0 = phase; iy0 < p.GY && first == 0x7fffffff; iy0 += GG_PHASES * GG_AHEAD) {
      int count[GG_AHEAD], obstacle[GG_AHEAD];
#pragma unroll
      for (int j = 0; j < GG_AHEAD; ++j) {
        const int iy = iy0 + j * GG_PHASES;
        count[j] = iy < p.GY ? p.rec.count[at + (long)iy * p.GX] : 0;
        obstacle[j] = iy < p.GY ? p.rec.obstacle[at + (long)iy * p.GX] : 0;
      }
#pragma unroll
      for (int j = GG_AHEAD - 1; j >= 0; --j)
        if (gg_state(count[j], obstacle[j], p.min_points, p.min_obstacle) == 2) first = iy0 + j * GG_PHASES;
    }
  }
  s_first[phase][tid & (GG_COLS - 1)] = first;
  __syncthreads();
  if (tid < GG_COLS && ix < p.GX) {
#pragma unroll
    for (int q = 0; q < GG_PHASES; ++q) first = min(first, s_first[q][tid]);
    p.first[(long)b * p.GX + ix] = first == 0x7fffffff ? __uint_as_float(0x7f800000u) : __fadd_rn(p.y0, gg_mul((float)first, p.cell));
  }
}

long gg_tiles(int H, int W, int sy, int sx) {
  const long n = (long)ocv_cdiv(H, sy) * ocv_cdiv(W, sx);
  return (n + GG_TILE - 1) / GG_TILE;
}

bool gg_grid_ok(int B, int GX, int GY) {
  return B >= 1 && GX >= 1 && GY >= 1 && GX <= GG_MAX_SIDE && GY <= GG_MAX_SIDE && (long)B * GX * GY <= 0x7fffffffL;
}

constexpr size_t GG_RECORD_BYTES = sizeof(long long) + 4 * sizeof(int);

}  // namespace

extern "C" size_t ocv_ground_grid_workspace_bytes(int B, int GX, int GY) {
  if (!gg_grid_ok(B, GX, GY)) return 0;
  return (size_t)B * (size_t)GX * (size_t)GY * GG_RECORD_BYTES;
}

extern "C" int ocv_ground_grid_fwd(const float* depth, const float* K, const float* pose, const float* confidence, const float* depth_std,
                                   int B, int H, int W, int sy, int sx, float near, float far, float min_confidence, float max_std,
                                   float x0, float y0, float cell, int GX, int GY, float lo, float hi, float obstacle_height,
                                   int min_points, int min_obstacle_points, int* count, int* obstacle, float* h_min, float* h_max,
                                   float* h_mean, uint8_t* state, float* first_occupied, void* workspace, size_t workspace_bytes,
                                   ocv_stream_t stream) {
  OCV_CHECK_ARG(depth && K && pose && workspace, "ocv_ground_grid_fwd: null pointer (depth, K, pose, workspace)");
  OCV_CHECK_ARG(count || obstacle || h_min || h_max || h_mean || state || first_occupied, "ocv_ground_grid_fwd: no output given");
  OCV_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && GX >= 1 && GY >= 1, "ocv_ground_grid_fwd: bad sizes (B, H, W, GX, GY must be >= 1)");
  OCV_CHECK_ARG(sy >= 1 && sx >= 1, "ocv_ground_grid_fwd: stride (%d, %d) must be >= 1", sy, sx);
  OCV_CHECK_ARG((long)H * W <= 0x7fffffffL && (long)B * gg_tiles(H, W, sy, sx) <= 0x7fffffffL && gg_grid_ok(B, GX, GY),
                "ocv_ground_grid_fwd: bad sizes (H * W, B * tiles and B * GX * GY below 2^31, GX and GY at most 2^24)");
  OCV_CHECK_ARG(near <= far, "ocv_ground_grid_fwd: near = %g must be <= far = %g", (double)near, (double)far);
  OCV_CHECK_ARG(cell > 0.f && cell <= FLT_MAX, "ocv_ground_grid_fwd: cell = %g must be > 0 and finite", (double)cell);
  OCV_CHECK_ARG(fabsf(x0) <= FLT_MAX && fabsf(y0) <= FLT_MAX, "ocv_ground_grid_fwd: origin (%g, %g) must be finite", (double)x0, (double)y0);
  OCV_CHECK_ARG(lo <= hi && fabsf(lo) <= 1000.f && fabsf(hi) <= 1000.f,
                "ocv_ground_grid_fwd: band [%g, %g] must have lo <= hi, both within +-1000", (double)lo, (double)hi);
  OCV_CHECK_ARG(obstacle_height == obstacle_height, "ocv_ground_grid_fwd: obstacle_height is NaN");
  OCV_CHECK_ARG(min_points >= 1 && min_obstacle_points >= 1, "ocv_ground_grid_fwd: min_points = %d and min_obstacle_points = %d must be >= 1",
                min_points, min_obstacle_points);
  OCV_CHECK_ARG(ocv_aligned16(K) && ocv_aligned16(pose), "ocv_ground_grid_fwd: K / pose must be 16-byte aligned");
  OCV_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "ocv_ground_grid_fwd: misaligned pointer (workspace: 8 bytes)");
  OCV_CHECK_ARG(((reinterpret_cast<uintptr_t>(depth) | reinterpret_cast<uintptr_t>(confidence) | reinterpret_cast<uintptr_t>(depth_std) |
                  reinterpret_cast<uintptr_t>(count) | reinterpret_cast<uintptr_t>(obstacle) | reinterpret_cast<uintptr_t>(h_min) |
                  reinterpret_cast<uintptr_t>(h_max) | reinterpret_cast<uintptr_t>(h_mean) | reinterpret_cast<uintptr_t>(first_occupied)) & 3) == 0,
                "ocv_ground_grid_fwd: misaligned pointer");
  const size_t need = ocv_ground_grid_workspace_bytes(B, GX, GY);
  OCV_CHECK_ARG(workspace_bytes >= need, "ocv_ground_grid_fwd: workspace too small (%zu bytes, need %zu)", workspace_bytes, need);

  const long n = (long)B * GX * GY;
  GridRecords rec{};
  rec.sum = static_cast<long long*>(workspace);
  rec.count = reinterpret_cast<int*>(rec.sum + n);
  rec.obstacle = rec.count + n;
  rec.nmin = reinterpret_cast<unsigned*>(rec.obstacle + n);
  rec.max = rec.nmin + n;

  const int zrc = ocv_zero_async(workspace, need, (hipStream_t)stream);
  if (zrc != 0) return zrc;

  GridArgs a{};
  a.depth = depth; a.K = K; a.pose = pose; a.conf = confidence; a.std = depth_std; a.rec = rec;
  a.H = H; a.W = W; a.sy = sy; a.sx = sx; a.Wc = ocv_cdiv(W, sx); a.T = (int)gg_tiles(H, W, sy, sx); a.GX = GX; a.GY = GY;
  a.N = (unsigned)((long)ocv_cdiv(H, sy) * a.Wc); a.cells = GX * GY;
  a.near = near; a.far = far; a.min_conf = min_confidence; a.max_std = max_std;
  a.x0 = x0; a.y0 = y0; a.cell = cell; a.lo = lo; a.hi = hi; a.obstacle_height = obstacle_height;
  hipLaunchKernelGGL(grid_accumulate_kernel, dim3((unsigned)((long)B * a.T)), dim3(GG_THREADS), 0, (hipStream_t)stream, a);
  OCV_CHECK_LAUNCH("ocv_ground_grid_fwd (accumulate)");

  FinalArgs f{};
  f.rec = rec; f.count = count; f.obstacle = obstacle; f.h_min = h_min; f.h_max = h_max; f.h_mean = h_mean; f.first = first_occupied;
  f.state = state; f.B = B; f.GX = GX; f.GY = GY; f.cells = GX * GY; f.min_points = min_points; f.min_obstacle = min_obstacle_points;
  f.n = n; f.y0 = y0; f.cell = cell;
  const bool cells_wanted = count || obstacle || h_min || h_max || h_mean || state;
  f.cell_blocks = cells_wanted ? (int)((n + GG_THREADS - 1) / GG_THREADS) : 0;
  f.col_groups = ocv_cdiv(GX, GG_COLS);
  const long blocks = (long)f.cell_blocks + (first_occupied ? (long)B * f.col_groups : 0);
  hipLaunchKernelGGL(grid_finalize_kernel, dim3((unsigned)blocks), dim3(GG_THREADS), 0, (hipStream_t)stream, f);
  OCV_CHECK_LAUNCH("ocv_ground_grid_fwd (finalize)");
  return 0;
}
