// Obstacle list behind the ground grid (DESIGN.md section 6b "Obstacles", STATEMENT O of include/objcavit_hip.h):
//   state uint8 [B][GY][GX] (+ count, obstacle, h_max of ocv_ground_grid_fwd) -> the connected components of the occupied cells under
//   |dix|, |diy| <= link, each with its extent, cell / point counts, centroid, height and fill; those kept ranked nearest first.
// Connected-component labelling by union-find with union by smaller index (union_find.hpp: a parent only ever decreases, so every loop
// ends by construction and the root of a component is its smallest linear index).  The launches, all 256 threads wide:
//   clear    zero fill of the per-cell records in the workspace (ocv_zero_async: a launch, not a memset node).  All-zero means "nothing
//            joined": the minima are kept as maxima of the complements (GX - 1 - ix, GY - 1 - iy), the height by its key (float_key.hpp).
//   tile     one workgroup per (image, OB_TILE x OB_TILE cells).  The tile's occupancy is staged once into LDS and the union-find runs
//            there on LDS-local indices (row-major in the tile, which orders cells as the image's linear index does, so the local minimum
//            is the global one), each cell joining the occupied cells of the FORWARD half of its (2 link + 1)^2 window (every pair is
//            seen from its smaller index).  No halo is staged: a pair across a tile edge is the seam pass's, and two cells of a tile that
//            are connected only through another tile are joined there as well.  Then every cell's parent goes to the workspace as a linear
//            index of the image, -1 for a cell that is not occupied.
//   seam     one thread per cell; only occupied cells within `link` of their tile's left, right or lower edge have forward neighbours in
//            another tile.  find, then an atomic min on the larger root, again while another caller was faster (uf_union).
//   stats    one workgroup per (image, 256 consecutive cells): every occupied cell walks to its root, stores it as its parent (the
//            flattening) and sends n = 1, its count / obstacle, ix, iy, the extent and the key of its h_max to the record AT ITS ROOT.  A
//            wall puts thousands of cells on one record, so the cells are merged ON CHIP first: runs of lanes with equal root by the
//            segmented reduction csrc/ground_grid.hip uses (seg_reduce.hpp), then an LDS table keyed by root (OB_SLOTS slots, linear
//            probing, at most OB_PROBES probes, LDS integer atomics), one set of global atomics per distinct root of the workgroup.  A
//            leader whose probes all hit other roots goes straight to memory: correctness does not depend on the table.
//   count    one workgroup per (image, OB_CHUNK consecutive cells): the number of KEPT roots (parent == self, n >= min_cells,
//            obstacle_points >= min_obstacle_points) of the chunk.
//   write    same workgroups: the chunks' counts in front give the chunk's first rank (and all of them the total), a scan over the chunk
//            gives every kept root its rank = its position among the kept roots in row-major order; rank < cap writes its two rows; the
//            rank (or -2) is left per cell for the relabel pass; the rows at or beyond counts[b] are zeroed; counts / total.
//   relabel  (only with `labels`) one thread per cell: -1, or the rank found at the cell's root.
// INTEGER ATOMICS ONLY; every statistic is a function of the component as a set, so two calls give identical bytes.  The float outputs
// are formed once per component from the integers, one rounded operation at a time (the library is built with contraction on: gg_mul /
// gg_mul64 of rounded_mul.hpp where a product feeds a sum).  No allocation, no synchronisation, nothing read on the host: capturable.
#include "common.hpp"
#include "float_key.hpp"
#include "rounded_mul.hpp"
#include "seg_reduce.hpp"
#include "union_find.hpp"
#include "../../include/objcavit_hip.h"

#include <float.h>
#include <math.h>

namespace {

constexpr int OB_THREADS = 256, OB_WAVES = OB_THREADS / OCV_WAVE;
constexpr int OB_LOG_TILE = 5, OB_TILE = 1 << OB_LOG_TILE, OB_TILE_CELLS = OB_TILE * OB_TILE, OB_PER = OB_TILE_CELLS / OB_THREADS;
constexpr int OB_CHUNK = 1024, OB_CHUNK_PER = OB_CHUNK / OB_THREADS;
constexpr int OB_LOG_SLOTS = 8, OB_SLOTS = 1 << OB_LOG_SLOTS, OB_PROBES = 8;
constexpr int OB_MAX_SIDE = 1 << 24, OB_MAX_LINK = 3;
constexpr long long OB_CLAMP = 0x7fffffffLL;
static_assert(OB_TILE == OCV_OBSTACLES_TILE && OB_CHUNK == OCV_OBSTACLES_CHUNK, "the header names this kernel's tile and chunk");
static_assert(OB_SLOTS >= OB_THREADS, "a workgroup of the stats pass has at most one root per thread");
static_assert(OB_MAX_LINK < OB_TILE, "a window reaches the neighbouring tile only");

int g_on_chip_merge = 1;                                   // ocv_obstacles_set_dispatch: 0 = every cell goes straight to memory (the A/B)

struct ObRecords {                                         // the workspace's zero-filled part: [B * cells] of each, at the ROOT's cell
  long long *points, *obstacle, *sum_ix, *sum_iy;
  int *n, *nxmin, *xmax, *nymin, *ymax;                    // nxmin = GX - 1 - ix_min, nymin = GY - 1 - iy_min: all four joined by max
  unsigned* hkey;                                          // gg_key(h_max), joined by max; 0 = none
};

struct ObArgs {
  const uint8_t* state;
  const int *count, *obstacle;
  const float* h_max;
  ObRecords rec;
  int *parent, *rank, *chunk_count;                        // [B * cells], [B * cells], [B * chunks]
  int* cells;
  float* metres;
  int *labels, *counts, *total;
  int B, GX, GY, ncell, TX, TY, link, min_cells, min_obstacle, cap, chunks, groups, merge;   // groups: stats workgroups per image
  long n;                                                  // B * cells
  float x0, y0, cell;
};

struct ObValue {                                           // what one cell, or a set of cells of one component, sends to its root's record
  long long points, obstacle, sum_ix, sum_iy;
  int n, nxmin, xmax, nymin, ymax;
  unsigned hkey;
};

__device__ __forceinline__ void ob_global(const ObRecords& r, long at, const ObValue& v) {
  atomicAdd(r.n + at, v.n);
  if (v.points != 0) atomicAdd(reinterpret_cast<unsigned long long*>(r.points + at), (unsigned long long)v.points);
  if (v.obstacle != 0) atomicAdd(reinterpret_cast<unsigned long long*>(r.obstacle + at), (unsigned long long)v.obstacle);
  atomicAdd(reinterpret_cast<unsigned long long*>(r.sum_ix + at), (unsigned long long)v.sum_ix);
  atomicAdd(reinterpret_cast<unsigned long long*>(r.sum_iy + at), (unsigned long long)v.sum_iy);
  atomicMax(r.nxmin + at, v.nxmin);
  atomicMax(r.xmax + at, v.xmax);
  atomicMax(r.nymin + at, v.nymin);
  atomicMax(r.ymax + at, v.ymax);
  if (v.hkey != 0u) atomicMax(r.hkey + at, v.hkey);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// tile: union-find in LDS
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(OB_THREADS) void ob_tile_kernel(ObArgs p) {
  __shared__ int s_parent[OB_TILE_CELLS];
  __shared__ uint8_t s_occ[OB_TILE_CELLS];
  const int tid = threadIdx.x;
  const int tiles = p.TX * p.TY, b = blockIdx.x / tiles, t = blockIdx.x - b * tiles;
  const int ty = t / p.TX, tx = t - ty * p.TX;
  const int gx0 = tx << OB_LOG_TILE, gy0 = ty << OB_LOG_TILE;
  const long base = (long)b * p.ncell;
#pragma unroll
  for (int k = 0; k < OB_PER; ++k) {
    const int l = k * OB_THREADS + tid, lx = l & (OB_TILE - 1), ly = l >> OB_LOG_TILE;
    const int gx = gx0 + lx, gy = gy0 + ly;
    const bool in = gx < p.GX && gy < p.GY;
    s_occ[l] = (in && p.state[base + (long)gy * p.GX + gx] == 2) ? 1 : 0;
    s_parent[l] = l;
  }
  __syncthreads();
  const int L = p.link;
#pragma unroll
  for (int k = 0; k < OB_PER; ++k) {
    const int l = k * OB_THREADS + tid, lx = l & (OB_TILE - 1), ly = l >> OB_LOG_TILE;
    if (!s_occ[l]) continue;
    for (int dy = 0; dy <= L; ++dy) {                      // the forward half of the window: the rest of the row, then the rows below
      const int ny = ly + dy;
      if (ny >= OB_TILE) break;
      for (int dx = dy == 0 ? 1 : -L; dx <= L; ++dx) {
        const int nx = lx + dx;
        if (nx < 0 || nx >= OB_TILE) continue;
        const int m = (ny << OB_LOG_TILE) + nx;
        if (s_occ[m]) uf_union(s_parent, l, m);
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < OB_PER; ++k) {
    const int l = k * OB_THREADS + tid, lx = l & (OB_TILE - 1), ly = l >> OB_LOG_TILE;
    const int gx = gx0 + lx, gy = gy0 + ly;
    if (gx >= p.GX || gy >= p.GY) continue;
    int root = -1;
    if (s_occ[l]) {
      const int r = uf_find(s_parent, l);                  // (nothing stores any more: plain walks)
      root = (gy0 + (r >> OB_LOG_TILE)) * p.GX + gx0 + (r & (OB_TILE - 1));
    }
    p.parent[base + (long)gy * p.GX + gx] = root;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// seam: the pairs across tile edges, in memory
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(OB_THREADS) void ob_seam_kernel(ObArgs p) {
  const long i = (long)blockIdx.x * OB_THREADS + threadIdx.x;
  if (i >= p.n) return;
  const int b = (int)(i / p.ncell), c = (int)(i - (long)b * p.ncell);
  const int gy = c / p.GX, gx = c - gy * p.GX;
  const int lx = gx & (OB_TILE - 1), ly = gy & (OB_TILE - 1), L = p.link;
  if (lx >= L && lx < OB_TILE - L && ly < OB_TILE - L) return;                 // every forward neighbour is of this cell's own tile
  const long base = (long)b * p.ncell;
  if (p.state[base + c] != 2) return;
  int* parent = p.parent + base;
  for (int dy = 0; dy <= L; ++dy) {
    const int ny = gy + dy;
    if (ny >= p.GY) break;
    for (int dx = dy == 0 ? 1 : -L; dx <= L; ++dx) {
      const int nx = gx + dx;
      if (nx < 0 || nx >= p.GX) continue;
      if ((nx >> OB_LOG_TILE) == (gx >> OB_LOG_TILE) && (ny >> OB_LOG_TILE) == (gy >> OB_LOG_TILE)) continue;      // the tile pass's
      const int m = ny * p.GX + nx;
      if (p.state[base + m] == 2) uf_union(parent, c, m);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// stats: flatten, and the records at the roots
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(OB_THREADS) void ob_stats_kernel(ObArgs p) {
  __shared__ unsigned s_key[OB_SLOTS], s_hkey[OB_SLOTS];
  __shared__ unsigned long long s_points[OB_SLOTS], s_obstacle[OB_SLOTS], s_sum_ix[OB_SLOTS], s_sum_iy[OB_SLOTS];
  __shared__ int s_n[OB_SLOTS], s_nxmin[OB_SLOTS], s_xmax[OB_SLOTS], s_nymin[OB_SLOTS], s_ymax[OB_SLOTS];
  const int tid = threadIdx.x, lane = tid & (OCV_WAVE - 1);
  const int b = blockIdx.x / p.groups, c = (blockIdx.x - b * p.groups) * OB_THREADS + tid;
  const long base = (long)b * p.ncell;
  if (p.merge) {
    for (int i = tid; i < OB_SLOTS; i += OB_THREADS) {
      s_key[i] = 0u; s_hkey[i] = 0u; s_points[i] = 0ull; s_obstacle[i] = 0ull; s_sum_ix[i] = 0ull; s_sum_iy[i] = 0ull;
      s_n[i] = 0; s_nxmin[i] = 0; s_xmax[i] = 0; s_nymin[i] = 0; s_ymax[i] = 0;
    }
    __syncthreads();
  }
  int* parent = p.parent + base;
  int root = -1;
  ObValue v{};
  if (c < p.ncell && uf_load(parent, c) >= 0) {
    root = uf_find(parent, c);
    __atomic_store_n(parent + c, root, __ATOMIC_RELAXED);  // flatten: root <= what was there, so a walk that passes here still ends
    const int iy = c / p.GX, ix = c - iy * p.GX;
    v.n = 1;
    v.points = p.count != nullptr ? (long long)p.count[base + c] : 0ll;
    v.obstacle = p.obstacle != nullptr ? (long long)p.obstacle[base + c] : 0ll;
    v.sum_ix = ix; v.sum_iy = iy;
    v.nxmin = p.GX - 1 - ix; v.xmax = ix; v.nymin = p.GY - 1 - iy; v.ymax = iy;
    v.hkey = p.h_max != nullptr ? gg_key(p.h_max[base + c]) : 0u;
  }
  if (!p.merge) {
    if (root >= 0) ob_global(p.rec, base + root, v);
    return;
  }
  if (__ballot(root >= 0) != 0ull) {                       // (wave-uniform)
    // 1. runs of consecutive lanes with the same root: the run's first lane ends up with the run's join
    const SegRuns runs = seg_runs(root, lane);
    seg_reduce(runs, lane, [&](int o, bool take) {
      const long long points_o = __shfl_down(v.points, o, OCV_WAVE), obstacle_o = __shfl_down(v.obstacle, o, OCV_WAVE);
      const long long sum_ix_o = __shfl_down(v.sum_ix, o, OCV_WAVE), sum_iy_o = __shfl_down(v.sum_iy, o, OCV_WAVE);
      const int n_o = __shfl_down(v.n, o, OCV_WAVE), nxmin_o = __shfl_down(v.nxmin, o, OCV_WAVE), xmax_o = __shfl_down(v.xmax, o, OCV_WAVE);
      const int nymin_o = __shfl_down(v.nymin, o, OCV_WAVE), ymax_o = __shfl_down(v.ymax, o, OCV_WAVE);
      const unsigned hkey_o = __shfl_down(v.hkey, o, OCV_WAVE);
      if (take) {
        v.points += points_o; v.obstacle += obstacle_o; v.sum_ix += sum_ix_o; v.sum_iy += sum_iy_o; v.n += n_o;
        v.nxmin = max(v.nxmin, nxmin_o); v.xmax = max(v.xmax, xmax_o); v.nymin = max(v.nymin, nymin_o); v.ymax = max(v.ymax, ymax_o);
        v.hkey = max(v.hkey, hkey_o);
      }
    });
    // 2. the leaders insert
    if (runs.head && root >= 0) {
      unsigned slot = ((unsigned)root * 2654435761u) >> (32 - OB_LOG_SLOTS);
      bool placed = false;
      for (int probe = 0; probe < OB_PROBES && !placed; ++probe) {
        const unsigned old = atomicCAS(&s_key[slot], 0u, (unsigned)root + 1u);
        if (old == 0u || old == (unsigned)root + 1u) {
          atomicAdd(&s_n[slot], v.n);
          if (v.points != 0) atomicAdd(&s_points[slot], (unsigned long long)v.points);
          if (v.obstacle != 0) atomicAdd(&s_obstacle[slot], (unsigned long long)v.obstacle);
          atomicAdd(&s_sum_ix[slot], (unsigned long long)v.sum_ix);
          atomicAdd(&s_sum_iy[slot], (unsigned long long)v.sum_iy);
          atomicMax(&s_nxmin[slot], v.nxmin);
          atomicMax(&s_xmax[slot], v.xmax);
          atomicMax(&s_nymin[slot], v.nymin);
          atomicMax(&s_ymax[slot], v.ymax);
          atomicMax(&s_hkey[slot], v.hkey);
          placed = true;
        } else {
          slot = (slot + 1u) & (OB_SLOTS - 1);
        }
      }
      if (!placed) ob_global(p.rec, base + root, v);
    }
  }
  __syncthreads();
  for (int i = tid; i < OB_SLOTS; i += OB_THREADS) {
    const unsigned key = s_key[i];
    if (key == 0u) continue;
    ObValue w;
    w.points = (long long)s_points[i]; w.obstacle = (long long)s_obstacle[i]; w.sum_ix = (long long)s_sum_ix[i]; w.sum_iy = (long long)s_sum_iy[i];
    w.n = s_n[i]; w.nxmin = s_nxmin[i]; w.xmax = s_xmax[i]; w.nymin = s_nymin[i]; w.ymax = s_ymax[i]; w.hkey = s_hkey[i];
    ob_global(p.rec, base + (long)(key - 1u), w);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// count, write, relabel
// ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool ob_kept(const ObArgs& p, long base, int c) {
  if (c >= p.ncell || p.parent[base + c] != c) return false;
  return p.rec.n[base + c] >= p.min_cells && p.rec.obstacle[base + c] >= (long long)p.min_obstacle;
}

// the sum of v over the workgroup, in every thread (s: OB_WAVES ints of LDS; two barriers)
__device__ __forceinline__ int ob_block_sum(int v, int* s, int tid) {
#pragma unroll
  for (int o = OCV_WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, OCV_WAVE);
  __syncthreads();                                         // (s may still be read from the call before)
  if ((tid & (OCV_WAVE - 1)) == 0) s[tid / OCV_WAVE] = v;
  __syncthreads();
  int sum = 0;
#pragma unroll
  for (int w = 0; w < OB_WAVES; ++w) sum += s[w];
  return sum;
}

__global__ __launch_bounds__(OB_THREADS) void ob_count_kernel(ObArgs p) {
  __shared__ int s_sum[OB_WAVES];
  const int tid = threadIdx.x, b = blockIdx.x / p.chunks, chunk = blockIdx.x - b * p.chunks;
  const long base = (long)b * p.ncell;
  int mine = 0;
#pragma unroll
  for (int j = 0; j < OB_CHUNK_PER; ++j) {
    const long c = (long)chunk * OB_CHUNK + tid * OB_CHUNK_PER + j;
    mine += (c < p.ncell && ob_kept(p, base, (int)c)) ? 1 : 0;
  }
  const int sum = ob_block_sum(mine, s_sum, tid);
  if (tid == 0) p.chunk_count[(long)b * p.chunks + chunk] = sum;
}

__global__ __launch_bounds__(OB_THREADS) void ob_write_kernel(ObArgs p) {
  __shared__ int s_sum[OB_WAVES], s_scan[OB_WAVES];
  const int tid = threadIdx.x, lane = tid & (OCV_WAVE - 1), wave = tid / OCV_WAVE;
  const int b = blockIdx.x / p.chunks, chunk = blockIdx.x - b * p.chunks;
  const long base = (long)b * p.ncell;
  // the kept roots in the chunks in front, and in all of them
  int before = 0, all = 0;
  for (int j = tid; j < p.chunks; j += OB_THREADS) {
    const int n = p.chunk_count[(long)b * p.chunks + j];
    all += n;
    before += j < chunk ? n : 0;
  }
  before = ob_block_sum(before, s_sum, tid);
  const int total = ob_block_sum(all, s_sum, tid);
  // this thread's cells, and the exclusive scan of the threads' counts
  bool kept[OB_CHUNK_PER];
  int mine = 0;
#pragma unroll
  for (int j = 0; j < OB_CHUNK_PER; ++j) {
    const long c = (long)chunk * OB_CHUNK + tid * OB_CHUNK_PER + j;
    kept[j] = c < p.ncell && ob_kept(p, base, (int)c);
    mine += kept[j] ? 1 : 0;
  }
  int incl = mine;
#pragma unroll
  for (int o = 1; o < OCV_WAVE; o <<= 1) {
    const int up = __shfl_up(incl, o, OCV_WAVE);
    if (lane >= o) incl += up;
  }
  if (lane == OCV_WAVE - 1) s_scan[wave] = incl;
  __syncthreads();
  int k = before + incl - mine;
  for (int w = 0; w < wave; ++w) k += s_scan[w];
#pragma unroll
  for (int j = 0; j < OB_CHUNK_PER; ++j) {
    const long cl = (long)chunk * OB_CHUNK + tid * OB_CHUNK_PER + j;
    if (cl >= p.ncell) break;
    const int c = (int)cl;
    int rank = p.parent[base + c] < 0 ? -1 : -2;
    if (kept[j]) {
      if (k < p.cap) {
        rank = k;
        const long row = ((long)b * p.cap + k) * 8;
        const int n = p.rec.n[base + c];
        const int ix_min = p.GX - 1 - p.rec.nxmin[base + c], ix_max = p.rec.xmax[base + c];
        const int iy_min = p.GY - 1 - p.rec.nymin[base + c], iy_max = p.rec.ymax[base + c];
        if (p.cells != nullptr) {
          int* o = p.cells + row;
          o[0] = ix_min; o[1] = ix_max; o[2] = iy_min; o[3] = iy_max; o[4] = n;
          o[5] = (int)min(p.rec.points[base + c], OB_CLAMP);
          o[6] = (int)min(p.rec.obstacle[base + c], OB_CLAMP);
          o[7] = c;
        }
        if (p.metres != nullptr) {
          float* o = p.metres + row;
          const double dn = (double)n, dcell = (double)p.cell;
          o[0] = __fadd_rn(p.x0, gg_mul((float)ix_min, p.cell));
          o[1] = __fadd_rn(p.x0, gg_mul((float)(ix_max + 1), p.cell));
          o[2] = __fadd_rn(p.y0, gg_mul((float)iy_min, p.cell));
          o[3] = __fadd_rn(p.y0, gg_mul((float)(iy_max + 1), p.cell));
          o[4] = (float)__dadd_rn((double)p.x0, gg_mul64(__dadd_rn(__ddiv_rn((double)p.rec.sum_ix[base + c], dn), 0.5), dcell));
          o[5] = (float)__dadd_rn((double)p.y0, gg_mul64(__dadd_rn(__ddiv_rn((double)p.rec.sum_iy[base + c], dn), 0.5), dcell));
          o[6] = p.h_max != nullptr ? gg_unkey(p.rec.hkey[base + c]) : 0.f;
          o[7] = (float)__ddiv_rn(dn, gg_mul64((double)(ix_max - ix_min + 1), (double)(iy_max - iy_min + 1)));
        }
      }
      ++k;
    }
    p.rank[base + c] = rank;
  }
  const int written = min(total, p.cap);
  if (chunk == 0 && tid == 0) {
    if (p.counts != nullptr) p.counts[b] = written;
    if (p.total != nullptr) p.total[b] = total;
  }
  // the rows at or beyond counts[b]: all zero, shared out over the image's workgroups
  for (long r = (long)written + (long)chunk * OB_THREADS + tid; r < p.cap; r += (long)p.chunks * OB_THREADS) {
    const long row = ((long)b * p.cap + r) * 8;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      if (p.cells != nullptr) p.cells[row + q] = 0;
      if (p.metres != nullptr) p.metres[row + q] = 0.f;
    }
  }
}

__global__ __launch_bounds__(OB_THREADS) void ob_relabel_kernel(ObArgs p) {
  const long i = (long)blockIdx.x * OB_THREADS + threadIdx.x;
  if (i >= p.n) return;
  const int root = p.parent[i];
  p.labels[i] = root < 0 ? -1 : p.rank[i - (i % p.ncell) + root];
}

bool ob_grid_ok(int B, int GX, int GY) {
  return B >= 1 && GX >= 1 && GY >= 1 && GX <= OB_MAX_SIDE && GY <= OB_MAX_SIDE && (long)B * GX * GY < 0x80000000L;
}

long ob_chunks(int GX, int GY) { return ((long)GX * GY + OB_CHUNK - 1) / OB_CHUNK; }

constexpr size_t OB_RECORD_BYTES = 4 * sizeof(long long) + 6 * sizeof(int);    // the zero-filled part, per cell
constexpr size_t OB_CELL_BYTES = OB_RECORD_BYTES + 2 * sizeof(int);            // + parent, rank

}  // namespace

extern "C" int ocv_obstacles_set_dispatch(int on_chip_merge) {
  if (on_chip_merge != 0 && on_chip_merge != 1) {
    ocv_set_error("ocv_obstacles_set_dispatch: on_chip_merge must be 0 or 1, got %d", on_chip_merge);
    return -1;
  }
  g_on_chip_merge = on_chip_merge;
  return 0;
}

extern "C" size_t ocv_obstacles_workspace_bytes(int B, int GX, int GY) {
  if (!ob_grid_ok(B, GX, GY)) return 0;
  return (size_t)B * (size_t)GX * (size_t)GY * OB_CELL_BYTES + (size_t)B * (size_t)ob_chunks(GX, GY) * sizeof(int);
}

extern "C" int ocv_obstacles_fwd(const uint8_t* state, const int* count, const int* obstacle, const float* h_max, int B, int GX, int GY,
                                 float x0, float y0, float cell, int link, int min_cells, int min_obstacle_points, int cap, int* cells,
                                 float* metres, int* labels, int* counts, int* total, void* workspace, size_t workspace_bytes,
                                 ocv_stream_t stream) {
  OCV_CHECK_ARG(state && workspace, "ocv_obstacles_fwd: null pointer (state, workspace)");
  OCV_CHECK_ARG(cells || metres || labels || counts || total, "ocv_obstacles_fwd: no output given");
  OCV_CHECK_ARG(link >= 1 && link <= OB_MAX_LINK, "ocv_obstacles_fwd: link = %d must be 1, 2 or 3", link);
  OCV_CHECK_ARG(min_cells >= 1 && min_obstacle_points >= 0 && cap >= 1,
                "ocv_obstacles_fwd: min_cells = %d must be >= 1, min_obstacle_points = %d >= 0 and cap = %d >= 1", min_cells,
                min_obstacle_points, cap);
  OCV_CHECK_ARG(B >= 1 && GX >= 1 && GY >= 1, "ocv_obstacles_fwd: bad sizes (B, GX, GY must be >= 1)");
  OCV_CHECK_ARG(ob_grid_ok(B, GX, GY) && (long)B * cap * 8 < 0x80000000L,
                "ocv_obstacles_fwd: bad sizes (B * GX * GY and B * cap * 8 below 2^31, GX and GY at most 2^24)");
  OCV_CHECK_ARG(cell > 0.f && cell <= FLT_MAX, "ocv_obstacles_fwd: cell = %g must be > 0 and finite", (double)cell);
  OCV_CHECK_ARG(fabsf(x0) <= FLT_MAX && fabsf(y0) <= FLT_MAX, "ocv_obstacles_fwd: origin (%g, %g) must be finite", (double)x0, (double)y0);
  OCV_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "ocv_obstacles_fwd: misaligned pointer (workspace: 8 bytes)");
  OCV_CHECK_ARG(((reinterpret_cast<uintptr_t>(count) | reinterpret_cast<uintptr_t>(obstacle) | reinterpret_cast<uintptr_t>(h_max) |
                  reinterpret_cast<uintptr_t>(cells) | reinterpret_cast<uintptr_t>(metres) | reinterpret_cast<uintptr_t>(labels) |
                  reinterpret_cast<uintptr_t>(counts) | reinterpret_cast<uintptr_t>(total)) & 3) == 0,
                "ocv_obstacles_fwd: misaligned pointer");
  const size_t need = ocv_obstacles_workspace_bytes(B, GX, GY);
  OCV_CHECK_ARG(workspace_bytes >= need, "ocv_obstacles_fwd: workspace too small (%zu bytes, need %zu)", workspace_bytes, need);

  const long n = (long)B * GX * GY;
  ObArgs a{};
  a.rec.points = static_cast<long long*>(workspace);
  a.rec.obstacle = a.rec.points + n;
  a.rec.sum_ix = a.rec.obstacle + n;
  a.rec.sum_iy = a.rec.sum_ix + n;
  a.rec.n = reinterpret_cast<int*>(a.rec.sum_iy + n);
  a.rec.nxmin = a.rec.n + n;
  a.rec.xmax = a.rec.nxmin + n;
  a.rec.nymin = a.rec.xmax + n;
  a.rec.ymax = a.rec.nymin + n;
  a.rec.hkey = reinterpret_cast<unsigned*>(a.rec.ymax + n);
  a.parent = reinterpret_cast<int*>(a.rec.hkey + n);
  a.rank = a.parent + n;
  a.chunk_count = a.rank + n;
  a.state = state; a.count = count; a.obstacle = obstacle; a.h_max = h_max;
  a.cells = cells; a.metres = metres; a.labels = labels; a.counts = counts; a.total = total;
  a.B = B; a.GX = GX; a.GY = GY; a.ncell = GX * GY; a.TX = ocv_cdiv(GX, OB_TILE); a.TY = ocv_cdiv(GY, OB_TILE);
  a.link = link; a.min_cells = min_cells; a.min_obstacle = min_obstacle_points; a.cap = cap; a.chunks = (int)ob_chunks(GX, GY);
  a.groups = ocv_cdiv(a.ncell, OB_THREADS); a.merge = g_on_chip_merge; a.n = n; a.x0 = x0; a.y0 = y0; a.cell = cell;

  const int zrc = ocv_zero_async(workspace, (size_t)n * OB_RECORD_BYTES, (hipStream_t)stream);
  if (zrc != 0) return zrc;
  const hipStream_t st = (hipStream_t)stream;
  const unsigned per_cell = (unsigned)((n + OB_THREADS - 1) / OB_THREADS);
  hipLaunchKernelGGL(ob_tile_kernel, dim3((unsigned)((long)B * a.TX * a.TY)), dim3(OB_THREADS), 0, st, a);
  OCV_CHECK_LAUNCH("ocv_obstacles_fwd (tile)");
  if (a.TX > 1 || a.TY > 1) {
    hipLaunchKernelGGL(ob_seam_kernel, dim3(per_cell), dim3(OB_THREADS), 0, st, a);
    OCV_CHECK_LAUNCH("ocv_obstacles_fwd (seam)");
  }
  hipLaunchKernelGGL(ob_stats_kernel, dim3((unsigned)((long)B * a.groups)), dim3(OB_THREADS), 0, st, a);
  OCV_CHECK_LAUNCH("ocv_obstacles_fwd (stats)");
  hipLaunchKernelGGL(ob_count_kernel, dim3((unsigned)((long)B * a.chunks)), dim3(OB_THREADS), 0, st, a);
  OCV_CHECK_LAUNCH("ocv_obstacles_fwd (count)");
  hipLaunchKernelGGL(ob_write_kernel, dim3((unsigned)((long)B * a.chunks)), dim3(OB_THREADS), 0, st, a);
  OCV_CHECK_LAUNCH("ocv_obstacles_fwd (write)");
  if (labels != nullptr) {
    hipLaunchKernelGGL(ob_relabel_kernel, dim3(per_cell), dim3(OB_THREADS), 0, st, a);
    OCV_CHECK_LAUNCH("ocv_obstacles_fwd (relabel)");
  }
  return 0;
}
