// Ground memory: the occupancy grid fused over time (DESIGN.md section 6b "Ground memory", STATEMENT F of include/objcavit_hip.h):
//   this step's state / h_max, the previous step's evidence / fused h_max and the vehicle's motion in between
//   -> per cell: evidence int16, fused state, fused h_max; per lateral column: first_occupied of the fused state.
// ONE launch of 256-thread workgroups, no workspace, no atomics:
//   cell blocks    one per (image, FU_TILE x FU_TILE output cells).  A cell's value is a pure function of its own inputs and of ONE cell
//                  of the previous map (nearest neighbour through the motion), so there is nothing to stage or to join: the gather reads
//                  the previous map straight from memory (160 KB of evidence per image: it lives in L2).  The tile is square so that its
//                  source footprint stays compact under ANY rotation (16 x 16 cells turn into at most 24 x 24), where a row-shaped tile
//                  would turn into a column of 64 cache lines at a quarter turn.
//   column blocks  one per (image, FU_COLS lateral columns), thread = (row phase, column).  They do NOT read the fused state the cell
//                  blocks write -- that would take a second launch behind the first, or a grid-wide barrier -- but evaluate the
//                  statement again for the cells of their columns, FU_AHEAD rows at a time, and stop at the first occupied one.  The
//                  statement is a dozen operations and two loads per cell; a launch boundary costs more than the whole map.
// Every fp32 operation is rounded on its own (gg_mul of rounded_mul.hpp where a product feeds a sum: the library is built with
// contraction on), the rest is integer arithmetic: two calls give identical bytes.  No allocation, no synchronisation, nothing read on
// the host: capturable.
#include "common.hpp"
#include "rounded_mul.hpp"
#include "../../include/objcavit_hip.h"

#include <float.h>
#include <math.h>

namespace {

constexpr int FU_THREADS = 256;
constexpr int FU_LOG_TILE = 4, FU_TILE = 1 << FU_LOG_TILE;
constexpr int FU_COLS = 8, FU_PHASES = FU_THREADS / FU_COLS, FU_AHEAD = 8;
constexpr int FU_MAX_SIDE = 1 << 24, FU_MAX_INT = 16383;
static_assert(FU_TILE * FU_TILE == FU_THREADS, "one thread per cell of a tile");
static_assert(FU_TILE == OCV_GROUND_FUSE_TILE, "the header names this kernel's tile");

struct FuArgs {
  const uint8_t* state;
  const float* h_max;
  const int16_t* prev_evidence;
  const float* prev_h;
  const float* motion;
  int16_t* evidence;
  uint8_t* fused_state;
  float* fused_h;
  float* first;
  int B, GX, GY, cells, TX, TY, cell_blocks, col_groups;
  int free, occupied, decay, limit, free_at, occupied_at;
  float x0, y0, cell;
};

struct FuMotion {
  float c, s, tx, ty;
  bool forget;
};

__device__ __forceinline__ FuMotion fu_motion(const FuArgs& p, int b) {
  const float4 m = *reinterpret_cast<const float4*>(p.motion + 4 * (long)b);
  FuMotion r;
  r.c = m.x; r.s = m.y; r.tx = m.z; r.ty = m.w;
  r.forget = !(fabsf(m.x) <= FLT_MAX && fabsf(m.y) <= FLT_MAX && fabsf(m.z) <= FLT_MAX && fabsf(m.w) <= FLT_MAX);    // (NaN fails)
  return r;
}

// the cell of the previous map that output cell (iy, ix) carries, as iy' * GX + ix', or -1 when there is none
__device__ __forceinline__ int fu_source(const FuArgs& p, const FuMotion& m, int iy, int ix) {
  const float xc = __fadd_rn(p.x0, gg_mul(__fadd_rn((float)ix, 0.5f), p.cell));
  const float yc = __fadd_rn(p.y0, gg_mul(__fadd_rn((float)iy, 0.5f), p.cell));
  const float px = __fadd_rn(__fsub_rn(gg_mul(m.c, xc), gg_mul(m.s, yc)), m.tx);
  const float py = __fadd_rn(__fadd_rn(gg_mul(m.s, xc), gg_mul(m.c, yc)), m.ty);
  const float fxi = floorf(__fsub_rn(px, p.x0) / p.cell), fyi = floorf(__fsub_rn(py, p.y0) / p.cell);
  const bool inside = !m.forget && fxi >= 0.f && fxi < (float)p.GX && fyi >= 0.f && fyi < (float)p.GY;      // (NaN fails every comparison)
  return inside ? (int)fyi * p.GX + (int)fxi : -1;       // < GX * GY: fxi, fyi are whole numbers below GX, GY <= 2^24
}

__device__ __forceinline__ int fu_evidence(const FuArgs& p, int carried, int state) {
  const int m = abs(carried) - p.decay;
  const int faded = m > 0 ? (carried > 0 ? m : -m) : 0;
  const int hit = state == 2 ? p.occupied : state == 1 ? -p.free : 0;
  return min(max(faded + hit, -p.limit), p.limit);
}

__device__ __forceinline__ int fu_state(const FuArgs& p, int evidence) {
  return evidence >= p.occupied_at ? 2 : evidence <= -p.free_at ? 1 : 0;
}

__global__ __launch_bounds__(FU_THREADS) void ground_fuse_kernel(FuArgs p) {
  const int tid = threadIdx.x;
  if ((int)blockIdx.x < p.cell_blocks) {
    const int tiles = p.TX * p.TY, b = blockIdx.x / tiles, t = blockIdx.x - b * tiles;
    const int ty = t / p.TX, tx = t - ty * p.TX;
    const int iy = ty * FU_TILE + (tid >> FU_LOG_TILE), ix = tx * FU_TILE + (tid & (FU_TILE - 1));
    if (iy >= p.GY || ix >= p.GX) return;
    const long base = (long)b * p.cells, at = base + (long)iy * p.GX + ix;
    const FuMotion m = fu_motion(p, b);
    const int src = fu_source(p, m, iy, ix);
    const int state = p.state[at];
    const int carried = (src >= 0 && p.prev_evidence != nullptr) ? (int)p.prev_evidence[base + src] : 0;
    const int evidence = fu_evidence(p, carried, state);
    if (p.evidence != nullptr) p.evidence[at] = (int16_t)evidence;
    if (p.fused_state != nullptr) p.fused_state[at] = (uint8_t)fu_state(p, evidence);
    if (p.fused_h != nullptr) {
      const float ninf = __uint_as_float(0xff800000u);
      float h = ninf;
      if (p.h_max != nullptr && state == 2) h = p.h_max[at];
      if (p.prev_h != nullptr && src >= 0 && carried > 0) {
        const float q = p.prev_h[base + src];
        if (q > h) h = q;
      }
      p.fused_h[at] = (evidence > 0 && h > ninf) ? h : 0.f;
    }
    return;
  }
  // the column scan: workgroup = (image, FU_COLS columns), thread = (row phase, column)
  __shared__ int s_first[FU_PHASES][FU_COLS];
  const int g = (int)blockIdx.x - p.cell_blocks, b = g / p.col_groups;
  const int col = tid & (FU_COLS - 1), phase = tid / FU_COLS, ix = (g - b * p.col_groups) * FU_COLS + col;
  int first = 0x7fffffff;
  if (ix < p.GX) {
    const long base = (long)b * p.cells;
    const FuMotion m = fu_motion(p, b);
    for (int iy0 = phase; iy0 < p.GY && first == 0x7fffffff; iy0 += FU_PHASES * FU_AHEAD) {
      int src[FU_AHEAD], state[FU_AHEAD], carried[FU_AHEAD];
#pragma unroll
      for (int j = 0; j < FU_AHEAD; ++j) {
        const int iy = iy0 + j * FU_PHASES;
        src[j] = iy < p.GY ? fu_source(p, m, iy, ix) : -1;
        state[j] = iy < p.GY ? (int)p.state[base + (long)iy * p.GX + ix] : 0;
      }
#pragma unroll
      for (int j = 0; j < FU_AHEAD; ++j)
        carried[j] = (src[j] >= 0 && p.prev_evidence != nullptr) ? (int)p.prev_evidence[base + src[j]] : 0;
#pragma unroll
      for (int j = FU_AHEAD - 1; j >= 0; --j)            // (a row at or beyond GY has carried = state = 0: evidence 0 < occupied_at)
        if (fu_state(p, fu_evidence(p, carried[j], state[j])) == 2) first = iy0 + j * FU_PHASES;
    }
  }
  s_first[phase][col] = first;
  __syncthreads();
  if (tid < FU_COLS && ix < p.GX) {
#pragma unroll
    for (int q = 0; q < FU_PHASES; ++q) first = min(first, s_first[q][tid]);
    p.first[(long)b * p.GX + ix] = first == 0x7fffffff ? __uint_as_float(0x7f800000u) : __fadd_rn(p.y0, gg_mul((float)first, p.cell));
  }
}

bool fu_grid_ok(int B, int GX, int GY) {
  return B >= 1 && GX >= 1 && GY >= 1 && GX <= FU_MAX_SIDE && GY <= FU_MAX_SIDE && (long)B * GX * GY <= 0x7fffffffL;
}

bool fu_overlap(const void* a, size_t na, const void* b, size_t nb) {
  if (a == nullptr || b == nullptr) return false;
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + nb && y < x + na;
}

}  // namespace

extern "C" int ocv_ground_fuse_fwd(const uint8_t* state, const float* h_max, const int16_t* prev_evidence, const float* prev_h,
                                   const float* motion, int B, int GX, int GY, float x0, float y0, float cell, int free, int occupied,
                                   int decay, int limit, int free_at, int occupied_at, int16_t* evidence, uint8_t* fused_state,
                                   float* fused_h_max, float* first_occupied, ocv_stream_t stream) {
  OCV_CHECK_ARG(state && motion, "ocv_ground_fuse_fwd: null pointer (state, motion)");
  OCV_CHECK_ARG(evidence || fused_state || fused_h_max || first_occupied, "ocv_ground_fuse_fwd: no output given");
  OCV_CHECK_ARG(B >= 1 && GX >= 1 && GY >= 1, "ocv_ground_fuse_fwd: bad sizes (B, GX, GY must be >= 1)");
  OCV_CHECK_ARG(fu_grid_ok(B, GX, GY), "ocv_ground_fuse_fwd: bad sizes (B * GX * GY below 2^31, GX and GY at most 2^24)");
  OCV_CHECK_ARG(cell > 0.f && cell <= FLT_MAX, "ocv_ground_fuse_fwd: cell = %g must be > 0 and finite", (double)cell);
  OCV_CHECK_ARG(fabsf(x0) <= FLT_MAX && fabsf(y0) <= FLT_MAX, "ocv_ground_fuse_fwd: origin (%g, %g) must be finite", (double)x0, (double)y0);
  OCV_CHECK_ARG(free >= 0 && free <= FU_MAX_INT, "ocv_ground_fuse_fwd: free = %d must be in 0..%d", free, FU_MAX_INT);
  OCV_CHECK_ARG(occupied >= 0 && occupied <= FU_MAX_INT, "ocv_ground_fuse_fwd: occupied = %d must be in 0..%d", occupied, FU_MAX_INT);
  OCV_CHECK_ARG(decay >= 0 && decay <= FU_MAX_INT, "ocv_ground_fuse_fwd: decay = %d must be in 0..%d", decay, FU_MAX_INT);
  OCV_CHECK_ARG(limit >= 1 && limit <= FU_MAX_INT, "ocv_ground_fuse_fwd: limit = %d must be in 1..%d", limit, FU_MAX_INT);
  OCV_CHECK_ARG(free_at >= 1 && free_at <= FU_MAX_INT, "ocv_ground_fuse_fwd: free_at = %d must be in 1..%d", free_at, FU_MAX_INT);
  OCV_CHECK_ARG(occupied_at >= 1 && occupied_at <= FU_MAX_INT, "ocv_ground_fuse_fwd: occupied_at = %d must be in 1..%d", occupied_at,
                FU_MAX_INT);
  OCV_CHECK_ARG(ocv_aligned16(motion), "ocv_ground_fuse_fwd: misaligned pointer (motion: 16 bytes)");
  OCV_CHECK_ARG(((reinterpret_cast<uintptr_t>(h_max) | reinterpret_cast<uintptr_t>(prev_h) | reinterpret_cast<uintptr_t>(fused_h_max) |
                  reinterpret_cast<uintptr_t>(first_occupied)) & 3) == 0,
                "ocv_ground_fuse_fwd: misaligned pointer (fp32 tensors: 4 bytes)");
  OCV_CHECK_ARG(((reinterpret_cast<uintptr_t>(prev_evidence) | reinterpret_cast<uintptr_t>(evidence)) & 1) == 0,
                "ocv_ground_fuse_fwd: misaligned pointer (int16 tensors: 2 bytes)");
  // the warp is a gather and the column scan reads this step's state again: no output may lie over an input
  const size_t n = (size_t)B * GX * GY;
  const void* ins[5] = {prev_evidence, prev_h, state, h_max, motion};
  const size_t in_bytes[5] = {2 * n, 4 * n, n, 4 * n, 16 * (size_t)B};
  const char* in_names[5] = {"prev_evidence", "prev_h", "state", "h_max", "motion"};
  const void* outs[4] = {evidence, fused_h_max, fused_state, first_occupied};
  const size_t out_bytes[4] = {2 * n, 4 * n, n, 4 * (size_t)B * GX};
  const char* out_names[4] = {"evidence", "fused h_max", "fused state", "first_occupied"};
  for (int o = 0; o < 4; ++o)
    for (int i = 0; i < 5; ++i)
      OCV_CHECK_ARG(!fu_overlap(outs[o], out_bytes[o], ins[i], in_bytes[i]),
                    "ocv_ground_fuse_fwd: the output %s overlaps the input %s (the warp is a gather: it cannot run in place)", out_names[o],
                    in_names[i]);

  FuArgs a{};
  a.state = state; a.h_max = h_max; a.prev_evidence = prev_evidence; a.prev_h = prev_h; a.motion = motion;
  a.evidence = evidence; a.fused_state = fused_state; a.fused_h = fused_h_max; a.first = first_occupied;
  a.B = B; a.GX = GX; a.GY = GY; a.cells = GX * GY; a.TX = ocv_cdiv(GX, FU_TILE); a.TY = ocv_cdiv(GY, FU_TILE);
  a.free = free; a.occupied = occupied; a.decay = decay; a.limit = limit; a.free_at = free_at; a.occupied_at = occupied_at;
  a.x0 = x0; a.y0 = y0; a.cell = cell;
  const bool cells_wanted = evidence || fused_state || fused_h_max;
  const long cell_blocks = cells_wanted ? (long)B * a.TX * a.TY : 0;
  a.col_groups = ocv_cdiv(GX, FU_COLS);
  const long blocks = cell_blocks + (first_occupied ? (long)B * a.col_groups : 0);
  OCV_CHECK_ARG(blocks <= 0x7fffffffL, "ocv_ground_fuse_fwd: bad sizes (B * tiles at or above 2^31)");
  a.cell_blocks = (int)cell_blocks;
  hipLaunchKernelGGL(ground_fuse_kernel, dim3((unsigned)blocks), dim3(FU_THREADS), 0, (hipStream_t)stream, a);
  OCV_CHECK_LAUNCH("ocv_ground_fuse_fwd");
  return 0;
}
