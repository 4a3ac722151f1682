// Ground plane of the predict path's final map (DESIGN.md section 6b "Ground plane", STATEMENT E of include/objcavit_hip.h):
//   depth [B][1][H][W] (+ confidence, depth_std), K [B][4], triples [T][3] (a table of pixel triples made on the host), prior [B][12]
//   -> pose [B][12] = [R | t] camera -> ground frame of the plane the map's points agree on, stats [B][4]
// A consensus over a FIXED table of hypotheses (RANSAC without a random number at run time) and one refit from integer moments.  Four
// launches:
//   hypotheses  one thread per (image, triple): the plane through the triple's three points, (n, h), or "invalid" (h = NaN).  The same
//               launch zeroes the counts and the moments, so the workspace needs no clear of its own.
//   consensus   THE HOT ONE: T x candidates plane tests.  One 256-thread workgroup per (image, tile of GP_TILE = 1024 consecutive
//               candidates of the strided pixel grid, the ground grid's numbering), four candidates per thread, back-projected ONCE into
//               registers (X, Y, Z, thr; thr = -1 for a candidate that is not kept, which no residual is below).  The loop over the
//               hypotheses is wave-uniform: n and h come from uniform loads, eight hypotheses (128 bytes) at a time so that a wave
//               waits for memory once per eight, an invalid hypothesis is skipped by the whole wave, the plane test is packed fp32
//               arithmetic on two candidates at a time, and a hypothesis's inliers in a wave are a compare and the popcount of its
//               ballot -- a scalar, not a per-lane counter.  Lane t % 64 keeps the wave's count of hypothesis t in a register; every 64
//               hypotheses the wave stores them to its own row of an LDS table (GP_WAVES x 1024 int32, 16 KB).  At the end the workgroup
//               adds its four rows and issues ONE global integer add per hypothesis with a non-zero count.
//   moments     the same tiling; every wave finds the best hypothesis (largest count, smallest index) from the T counts itself, the
//               inliers' coordinates become integers q = rint(128 v) and nine int64 sums are reduced in the wave (shuffles), across the
//               waves (LDS) and into memory with one set of nine 64-bit integer adds per workgroup.
//   solve       one wave per image finds the best hypothesis again, its lane 0 solves the 2 x 2 normal equations in float64 and writes
//               the pose (or the prior's bytes) and the stats.
// INTEGER ATOMICS ONLY, so two calls give identical bytes.  No allocation, no synchronisation, nothing read on the host: capturable.
// The keep rule is keep_pixel.hpp's; every fp32 / fp64 operation is rounded on its own (rounded_mul.hpp where a product feeds a sum).
#include "common.hpp"
#include "keep_pixel.hpp"
#include "rounded_mul.hpp"
#include "../../include/objcavit_hip.h"

#include <math.h>

namespace {

constexpr int GP_THREADS = 256, GP_PER = 4, GP_TILE = GP_THREADS * GP_PER, GP_WAVES = GP_THREADS / OCV_WAVE;
constexpr int GP_MAX_T = OCV_GROUND_PLANE_MAX_HYPOTHESES, GP_MOMENTS = 9;
constexpr int GP_BATCH = OCV_GROUND_PLANE_BATCH;          // hypotheses per uniform load of the consensus loop; Tp is a multiple of it
constexpr long GP_MAX_CANDIDATES = 1L << 22;              // every moment stays below 2^53: 2^22 * (2^15)^2 = 2^52
constexpr float GP_MAX_COORD = 256.f, GP_SCALE = 128.f;   // |q| <= 2^15
static_assert(GP_TILE == OCV_GROUND_PLANE_TILE, "the header names this kernel's tile");
static_assert(GP_MAX_T % OCV_WAVE == 0, "a wave stores its counts 64 hypotheses at a time");
static_assert(OCV_WAVE % GP_BATCH == 0 && GP_PER % 2 == 0, "batches do not straddle a store; candidates are tested in pairs");

struct PlaneSpace {                                       // the workspace (the header documents the layout)
  float* hyp;                                             // [B][Tp][4] = n0, n1, n2, h; h = NaN: invalid.  Tp = T rounded up to GP_BATCH
  long long* mom;                                         // [B][9]
  int* count;                                             // [B][T]
};

struct PlaneArgs {
  const float *depth, *K, *prior, *conf, *std;
  const int* triples;
  PlaneSpace ws;
  float* pose;
  int* stats;
  int B, H, W, sy, sx, Wc, tiles, T, Tp, min_inliers;
  unsigned N;                                             // candidates per image
  float near, far, min_conf, max_std, tol, rel_tol, h_lo, h_hi, cos_tilt, min_cross;
};

// candidate r of thread tid of a tile: X, Y, Z and its threshold, or thr = -1 where the keep rule drops it
__device__ __forceinline__ void gp_candidate(const PlaneArgs& p, const float4 k, long plane, int tile, int r, int tid, float& X, float& Y,
                                             float& Z, float& thr) {
  const unsigned c = (unsigned)tile * GP_TILE + (unsigned)(r * GP_THREADS + tid);
  const bool in = c < p.N;
  const int yc = (int)(c / (unsigned)p.Wc), xc = (int)(c - (unsigned)yc * p.Wc);
  const int y = yc * p.sy, x = xc * p.sx;
  const long off = in ? plane + (long)y * p.W + x : 0;    // (H * W < 2^31: the entry point checks it)
  const float z = in ? p.depth[off] : 0.f;
  const float cf = (in && p.conf != nullptr) ? p.conf[off] : 1.f;
  const float sd = (in && p.std != nullptr) ? p.std[off] : 0.f;
  const bool kept = up_keep(in, z, cf, sd, p.conf != nullptr, p.std != nullptr, p.near, p.far, p.min_conf, p.max_std);
  const float rx = __fsub_rn((float)x, k.z) / k.x, ry = __fsub_rn((float)y, k.w) / k.y;
  X = kept ? gg_mul(rx, z) : 0.f;
  Y = kept ? gg_mul(ry, z) : 0.f;
  Z = kept ? z : 0.f;
  thr = kept ? __fadd_rn(p.tol, gg_mul(p.rel_tol, z)) : -1.f;
}

__device__ __forceinline__ bool gp_inlier(float n0, float n1, float n2, float h, float X, float Y, float Z, float thr) {
  const float d = __fadd_rn(__fadd_rn(__fadd_rn(gg_mul(n0, X), gg_mul(n1, Y)), gg_mul(n2, Z)), h);
  return fabsf(d) <= thr;                                 // (NaN fails; thr = -1 fails)
}

// the selection, by a whole wave: the smallest t with the largest count (every lane returns the same pair)
__device__ __forceinline__ int gp_best(const int* count, int T, int lane, int& best_count) {
  int bc = -1, bt = 0x7fffffff;
  for (int t = lane; t < T; t += OCV_WAVE) {
    const int c = count[t];
    if (c > bc) { bc = c; bt = t; }
  }
#pragma unroll
  for (int o = OCV_WAVE / 2; o > 0; o >>= 1) {
    const int oc = __shfl_xor(bc, o, OCV_WAVE), ot = __shfl_xor(bt, o, OCV_WAVE);
    if (oc > bc || (oc == bc && ot < bt)) { bc = oc; bt = ot; }
  }
  best_count = bc;
  return bt;
}

__device__ __forceinline__ bool gp_prior_finite(const float* q) {
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 12; ++i) ok = ok && up_finite(q[i]);
  return ok;
}

__global__ __launch_bounds__(GP_THREADS) void plane_hypotheses_kernel(PlaneArgs p) {
  const long i = (long)blockIdx.x * GP_THREADS + threadIdx.x;
  if (i < (long)p.B * GP_MOMENTS) p.ws.mom[i] = 0;
  if (i >= (long)p.B * p.Tp) return;
  const int b = (int)(i / p.Tp), t = (int)(i - (long)b * p.Tp);
  float n0 = 0.f, n1 = 0.f, n2 = 0.f, h = __uint_as_float(0x7fc00000u);
  if (t < p.T) {
    p.ws.count[(long)b * p.T + t] = 0;
    const float4 k = *reinterpret_cast<const float4*>(p.K + 4 * (long)b);
    const float* q = p.prior + 12 * (long)b;
    const long hw = (long)p.H * p.W, plane = (long)b * hw;
    bool ok = up_camera_ok(k) && gp_prior_finite(q);
    float P[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int idx = p.triples[3 * t + j];
      const bool in = idx >= 0 && (long)idx < hw;
      const long off = in ? plane + idx : 0;              // (nothing is read through an index outside the map)
      const float z = in ? p.depth[off] : 0.f;
      const float cf = (in && p.conf != nullptr) ? p.conf[off] : 1.f;
      const float sd = (in && p.std != nullptr) ? p.std[off] : 0.f;
      ok = ok && up_keep(in, z, cf, sd, p.conf != nullptr, p.std != nullptr, p.near, p.far, p.min_conf, p.max_std);
      const int y = in ? idx / p.W : 0, x = in ? idx - y * p.W : 0;
      const float rx = __fsub_rn((float)x, k.z) / k.x, ry = __fsub_rn((float)y, k.w) / k.y;
      P[j][0] = gg_mul(rx, z); P[j][1] = gg_mul(ry, z); P[j][2] = z;
    }
    const float a0 = __fsub_rn(P[1][0], P[0][0]), a1 = __fsub_rn(P[1][1], P[0][1]), a2 = __fsub_rn(P[1][2], P[0][2]);
    const float b0 = __fsub_rn(P[2][0], P[0][0]), b1 = __fsub_rn(P[2][1], P[0][1]), b2 = __fsub_rn(P[2][2], P[0][2]);
    const float m0 = __fsub_rn(gg_mul(a1, b2), gg_mul(a2, b1)), m1 = __fsub_rn(gg_mul(a2, b0), gg_mul(a0, b2)),
                m2 = __fsub_rn(gg_mul(a0, b1), gg_mul(a1, b0));
    const float l = __fsqrt_rn(__fadd_rn(__fadd_rn(gg_mul(m0, m0), gg_mul(m1, m1)), gg_mul(m2, m2)));
    float c0 = __fdiv_rn(m0, l), c1 = __fdiv_rn(m1, l), c2 = __fdiv_rn(m2, l);
    if (c1 > 0.f) { c0 = -c0; c1 = -c1; c2 = -c2; }       // the camera's y points down: up has n1 < 0
    const float hh = -__fadd_rn(__fadd_rn(gg_mul(c0, P[0][0]), gg_mul(c1, P[0][1])), gg_mul(c2, P[0][2]));
    const float dot = __fadd_rn(__fadd_rn(gg_mul(c0, q[8]), gg_mul(c1, q[9])), gg_mul(c2, q[10]));
    if (ok && l >= p.min_cross && dot >= p.cos_tilt && p.h_lo <= hh && hh <= p.h_hi) {      // (NaN fails each)
      n0 = c0; n1 = c1; n2 = c2; h = hh;
    }
  }
  reinterpret_cast<float4*>(p.ws.hyp)[i] = make_float4(n0, n1, n2, h);
}

__global__ __launch_bounds__(GP_THREADS) void plane_consensus_kernel(PlaneArgs p) {
  __shared__ int s_count[GP_WAVES][GP_MAX_T];
  const int tid = threadIdx.x, lane = tid & (OCV_WAVE - 1), wave = tid / OCV_WAVE;
  const int b = blockIdx.x / p.tiles, tile = blockIdx.x - b * p.tiles;
  const float4 k = *reinterpret_cast<const float4*>(p.K + 4 * (long)b);
  if (!up_camera_ok(k)) return;                           // (the whole workgroup: b is its image) no candidates, the counts stay 0
  const long plane = (long)b * p.H * p.W;
  gg_float2 X[GP_PER / 2], Y[GP_PER / 2], Z[GP_PER / 2], thr[GP_PER / 2];      // pairs: the tests below are packed fp32 operations
#pragma unroll
  for (int r = 0; r < GP_PER / 2; ++r) {
    float x0, y0, z0, t0, x1, y1, z1, t1;
    gp_candidate(p, k, plane, tile, 2 * r, tid, x0, y0, z0, t0);
    gp_candidate(p, k, plane, tile, 2 * r + 1, tid, x1, y1, z1, t1);
    X[r] = gg_float2{x0, x1}; Y[r] = gg_float2{y0, y1}; Z[r] = gg_float2{z0, z1}; thr[r] = gg_float2{t0, t1};
  }
  const float4* hyp = reinterpret_cast<const float4*>(p.ws.hyp) + (long)b * p.Tp;
  int mine = 0;
  for (int t0 = 0; t0 < p.Tp; t0 += GP_BATCH) {           // wave-uniform: GP_BATCH hypotheses per uniform 128-byte load, a uniform skip
    float4 q[GP_BATCH];
#pragma unroll
    for (int j = 0; j < GP_BATCH; ++j) q[j] = hyp[t0 + j];
#pragma unroll
    for (int j = 0; j < GP_BATCH; ++j) {
      const int t = t0 + j;
      int c = 0;
      if (q[j].w == q[j].w) {
#pragma unroll
        for (int r = 0; r < GP_PER / 2; ++r) {              // gp_inlier, two candidates at a time (the same operations, each rounded on its own)
          const gg_float2 d = ((gg_mul2(q[j].x, X[r]) + gg_mul2(q[j].y, Y[r])) + gg_mul2(q[j].z, Z[r])) + q[j].w;
          c += __popcll(__ballot(fabsf(d.x) <= thr[r].x)) + __popcll(__ballot(fabsf(d.y) <= thr[r].y));
        }
      }
      if (lane == (t & (OCV_WAVE - 1))) mine = c;
      if ((t & (OCV_WAVE - 1)) == OCV_WAVE - 1 || t == p.Tp - 1) {
        s_count[wave][(t & ~(OCV_WAVE - 1)) + lane] = mine; // (t < Tp <= 1024 = GP_MAX_T, a multiple of 64: the index stays below it)
        mine = 0;
      }
    }
  }
  __syncthreads();
  int* count = p.ws.count + (long)b * p.T;
  for (int t = tid; t < p.T; t += GP_THREADS) {
    int c = 0;
#pragma unroll
    for (int w = 0; w < GP_WAVES; ++w) c += s_count[w][t];
    if (c != 0) atomicAdd(count + t, c);
  }
}

__global__ __launch_bounds__(GP_THREADS) void plane_moments_kernel(PlaneArgs p) {
  __shared__ long long s_mom[GP_WAVES][GP_MOMENTS];
  const int tid = threadIdx.x, lane = tid & (OCV_WAVE - 1), wave = tid / OCV_WAVE;
  const int b = blockIdx.x / p.tiles, tile = blockIdx.x - b * p.tiles;
  const float4 k = *reinterpret_cast<const float4*>(p.K + 4 * (long)b);
  if (!up_camera_ok(k)) return;
  int best_count;
  const int best = gp_best(p.ws.count + (long)b * p.T, p.T, lane, best_count);
  if (best_count < p.min_inliers) return;                 // (the whole workgroup) no plane: the moments stay 0
  const float4 hyp = reinterpret_cast<const float4*>(p.ws.hyp)[(long)b * p.Tp + best];
  const float n0 = hyp.x, n1 = hyp.y, n2 = hyp.z, h = hyp.w;
  const long plane = (long)b * p.H * p.W;
  long long s[GP_MOMENTS];
#pragma unroll
  for (int i = 0; i < GP_MOMENTS; ++i) s[i] = 0;
#pragma unroll
  for (int r = 0; r < GP_PER; ++r) {
    float X, Y, Z, thr;
    gp_candidate(p, k, plane, tile, r, tid, X, Y, Z, thr);
    if (gp_inlier(n0, n1, n2, h, X, Y, Z, thr) && fabsf(X) <= GP_MAX_COORD && fabsf(Y) <= GP_MAX_COORD && fabsf(Z) <= GP_MAX_COORD) {
      const int qx = (int)rintf(__fmul_rn(X, GP_SCALE)), qy = (int)rintf(__fmul_rn(Y, GP_SCALE)), qz = (int)rintf(__fmul_rn(Z, GP_SCALE));
      s[0] += 1; s[1] += qx; s[2] += qy; s[3] += qz;      // |q| <= 2^15: the products fit an int32
      s[4] += qx * qx; s[5] += qx * qz; s[6] += qz * qz; s[7] += qx * qy; s[8] += qz * qy;
    }
  }
#pragma unroll
  for (int i = 0; i < GP_MOMENTS; ++i) {
#pragma unroll
    for (int o = OCV_WAVE / 2; o > 0; o >>= 1) s[i] += __shfl_down(s[i], o, OCV_WAVE);
    if (lane == 0) s_mom[wave][i] = s[i];
  }
  __syncthreads();
  if (tid < GP_MOMENTS) {
    long long v = 0;
#pragma unroll
    for (int w = 0; w < GP_WAVES; ++w) v += s_mom[w][tid];
    if (v != 0) atomicAdd(reinterpret_cast<unsigned long long*>(p.ws.mom + (long)b * GP_MOMENTS + tid), (unsigned long long)v);
  }
}

__device__ __forceinline__ double gp_sub_products(double a, double b, double c, double d) {   // a * b - c * d, three roundings
  return __dsub_rn(gg_mul64(a, b), gg_mul64(c, d));
}

__global__ __launch_bounds__(OCV_WAVE) void plane_solve_kernel(PlaneArgs p) {
  const int b = blockIdx.x, lane = threadIdx.x;
  int best_count;
  int best = gp_best(p.ws.count + (long)b * p.T, p.T, lane, best_count);
  if (best_count < p.min_inliers) { best = -1; best_count = 0; }
  if (lane != 0) return;
  const long long* m = p.ws.mom + (long)b * GP_MOMENTS;
  const float* q = p.prior + 12 * (long)b;
  float out[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) out[i] = q[i];
  const long long n = m[0];
  int ok = 0;
  if (best >= 0 && n >= (long long)p.min_inliers) {
    const double N = (double)n;
    const double mx = __ddiv_rn((double)m[1], N), my = __ddiv_rn((double)m[2], N), mz = __ddiv_rn((double)m[3], N);
    const double cxx = __dsub_rn(__ddiv_rn((double)m[4], N), gg_mul64(mx, mx)), cxz = __dsub_rn(__ddiv_rn((double)m[5], N), gg_mul64(mx, mz));
    const double czz = __dsub_rn(__ddiv_rn((double)m[6], N), gg_mul64(mz, mz)), cxy = __dsub_rn(__ddiv_rn((double)m[7], N), gg_mul64(mx, my));
    const double czy = __dsub_rn(__ddiv_rn((double)m[8], N), gg_mul64(mz, my));
    const double det = gp_sub_products(cxx, czz, cxz, cxz);
    const double A = __ddiv_rn(gp_sub_products(cxy, czz, czy, cxz), det), Bc = __ddiv_rn(gp_sub_products(czy, cxx, cxy, cxz), det);
    const double C = __ddiv_rn(__dsub_rn(__dsub_rn(my, gg_mul64(A, mx)), gg_mul64(Bc, mz)), 128.0);
    const double s = __dsqrt_rn(__dadd_rn(__dadd_rn(gg_mul64(A, A), 1.0), gg_mul64(Bc, Bc)));
    const double u0 = __ddiv_rn(A, s), u1 = __ddiv_rn(-1.0, s), u2 = __ddiv_rn(Bc, s), hgt = __ddiv_rn(C, s);
    const double g0 = -gg_mul64(u2, u0), g1 = -gg_mul64(u2, u1), g2 = __dsub_rn(1.0, gg_mul64(u2, u2));
    const double lf = __dsqrt_rn(__dadd_rn(__dadd_rn(gg_mul64(g0, g0), gg_mul64(g1, g1)), gg_mul64(g2, g2)));
    const double f0 = __ddiv_rn(g0, lf), f1 = __ddiv_rn(g1, lf), f2 = __ddiv_rn(g2, lf);
    const double r0 = gp_sub_products(f1, u2, f2, u1), r1 = gp_sub_products(f2, u0, f0, u2), r2 = gp_sub_products(f0, u1, f1, u0);
    const double dot = __dadd_rn(__dadd_rn(gg_mul64(u0, (double)q[8]), gg_mul64(u1, (double)q[9])), gg_mul64(u2, (double)q[10]));
    const float made[12] = {(float)r0, (float)r1, (float)r2, 0.f, (float)f0, (float)f1, (float)f2, 0.f, (float)u0, (float)u1, (float)u2, (float)hgt};
    bool fine = det > 0.0 && (double)p.h_lo <= hgt && hgt <= (double)p.h_hi && dot >= (double)p.cos_tilt && lf > 0.0;
#pragma unroll
    for (int i = 0; i < 12; ++i) fine = fine && up_finite(made[i]);
    if (fine) {
      ok = 1;
#pragma unroll
      for (int i = 0; i < 12; ++i) out[i] = made[i];
    }
  }
  float* pose = p.pose + 12 * (long)b;
#pragma unroll
  for (int i = 0; i < 12; ++i) pose[i] = out[i];
  int* st = p.stats + 4 * (long)b;
  st[0] = best; st[1] = best_count; st[2] = (int)n; st[3] = ok;
}

long gp_candidates(int H, int W, int sy, int sx) { return (long)ocv_cdiv(H, sy) * ocv_cdiv(W, sx); }

bool gp_sizes_ok(int B, int T) { return B >= 1 && T >= 1 && T <= GP_MAX_T && (long)B * GP_MAX_T * 4 <= 0x7fffffffL; }

}  // namespace

extern "C" size_t ocv_ground_plane_workspace_bytes(int B, int T) {
  if (!gp_sizes_ok(B, T)) return 0;
  const size_t Tp = (size_t)((T + GP_BATCH - 1) & ~(GP_BATCH - 1));
  return (size_t)B * (Tp * 4 * sizeof(float) + GP_MOMENTS * sizeof(long long) + (size_t)T * sizeof(int));
}

extern "C" int ocv_ground_plane_fwd(const float* depth, const float* K, const int* triples, const float* prior, const float* confidence,
                                    const float* depth_std, int B, int H, int W, int T, int sy, int sx, float near, float far,
                                    float min_confidence, float max_std, float tol, float rel_tol, float h_lo, float h_hi, float cos_tilt,
                                    float min_cross, int min_inliers, float* pose, int* stats, void* workspace, size_t workspace_bytes,
                                    ocv_stream_t stream) {
  OCV_CHECK_ARG(depth && K && triples && prior && pose && stats && workspace,
                "ocv_ground_plane_fwd: null pointer (depth, K, triples, prior, pose, stats, workspace)");
  OCV_CHECK_ARG(B >= 1 && H >= 1 && W >= 1, "ocv_ground_plane_fwd: bad sizes (B, H, W must be >= 1)");
  OCV_CHECK_ARG(T >= 1 && T <= GP_MAX_T, "ocv_ground_plane_fwd: T = %d hypotheses, must be in 1..%d", T, GP_MAX_T);
  OCV_CHECK_ARG(sy >= 1 && sx >= 1, "ocv_ground_plane_fwd: stride (%d, %d) must be >= 1", sy, sx);
  OCV_CHECK_ARG((long)H * W <= 0x7fffffffL && gp_sizes_ok(B, T), "ocv_ground_plane_fwd: bad sizes (H * W and B * 4096 below 2^31)");
  const long cand = gp_candidates(H, W, sy, sx), tiles = (cand + GP_TILE - 1) / GP_TILE;
  OCV_CHECK_ARG(cand <= GP_MAX_CANDIDATES, "ocv_ground_plane_fwd: %ld candidates per image, at most 2^22 (raise the stride)", cand);
  OCV_CHECK_ARG((long)B * tiles <= 0x7fffffffL, "ocv_ground_plane_fwd: bad sizes (B * tiles below 2^31)");
  OCV_CHECK_ARG(near <= far, "ocv_ground_plane_fwd: near = %g must be <= far = %g", (double)near, (double)far);
  OCV_CHECK_ARG(tol >= 0.f && tol <= FLT_MAX && rel_tol >= 0.f && rel_tol <= FLT_MAX,
                "ocv_ground_plane_fwd: tol = %g and rel_tol = %g must be >= 0 and finite", (double)tol, (double)rel_tol);
  OCV_CHECK_ARG(h_lo <= h_hi, "ocv_ground_plane_fwd: height range [%g, %g] must have h_lo <= h_hi", (double)h_lo, (double)h_hi);
  OCV_CHECK_ARG(cos_tilt > 0.f && cos_tilt <= 1.f, "ocv_ground_plane_fwd: cos_tilt = %g must be in (0, 1]", (double)cos_tilt);
  OCV_CHECK_ARG(min_cross > 0.f, "ocv_ground_plane_fwd: min_cross = %g must be > 0", (double)min_cross);
  OCV_CHECK_ARG(min_inliers >= 3, "ocv_ground_plane_fwd: min_inliers = %d must be >= 3", min_inliers);
  OCV_CHECK_ARG(ocv_aligned16(K) && ocv_aligned16(prior), "ocv_ground_plane_fwd: K / prior must be 16-byte aligned");
  OCV_CHECK_ARG(ocv_aligned16(workspace), "ocv_ground_plane_fwd: misaligned pointer (workspace: 16 bytes)");
  OCV_CHECK_ARG(((reinterpret_cast<uintptr_t>(depth) | reinterpret_cast<uintptr_t>(confidence) | reinterpret_cast<uintptr_t>(depth_std) |
                  reinterpret_cast<uintptr_t>(triples) | reinterpret_cast<uintptr_t>(pose) | reinterpret_cast<uintptr_t>(stats)) & 3) == 0,
                "ocv_ground_plane_fwd: misaligned pointer");
  const size_t need = ocv_ground_plane_workspace_bytes(B, T);
  OCV_CHECK_ARG(workspace_bytes >= need, "ocv_ground_plane_fwd: workspace too small (%zu bytes, need %zu)", workspace_bytes, need);

  PlaneArgs a{};
  a.depth = depth; a.K = K; a.prior = prior; a.conf = confidence; a.std = depth_std; a.triples = triples; a.pose = pose; a.stats = stats;
  a.B = B; a.H = H; a.W = W; a.sy = sy; a.sx = sx; a.Wc = ocv_cdiv(W, sx); a.tiles = (int)tiles; a.T = T; a.Tp = (T + GP_BATCH - 1) & ~(GP_BATCH - 1);
  a.min_inliers = min_inliers; a.N = (unsigned)cand;
  a.near = near; a.far = far; a.min_conf = min_confidence; a.max_std = max_std; a.tol = tol; a.rel_tol = rel_tol; a.h_lo = h_lo;
  a.h_hi = h_hi; a.cos_tilt = cos_tilt; a.min_cross = min_cross;
  a.ws.hyp = static_cast<float*>(workspace);
  a.ws.mom = reinterpret_cast<long long*>(a.ws.hyp + (size_t)B * a.Tp * 4);     // (a multiple of 16 bytes in)
  a.ws.count = reinterpret_cast<int*>(a.ws.mom + (size_t)B * GP_MOMENTS);

  const long firsts = (long)B * (a.Tp > GP_MOMENTS ? a.Tp : GP_MOMENTS);
  hipLaunchKernelGGL(plane_hypotheses_kernel, dim3((unsigned)((firsts + GP_THREADS - 1) / GP_THREADS)), dim3(GP_THREADS), 0,
                     (hipStream_t)stream, a);
  OCV_CHECK_LAUNCH("ocv_ground_plane_fwd (hypotheses)");
  hipLaunchKernelGGL(plane_consensus_kernel, dim3((unsigned)((long)B * tiles)), dim3(GP_THREADS), 0, (hipStream_t)stream, a);
  OCV_CHECK_LAUNCH("ocv_ground_plane_fwd (consensus)");
  hipLaunchKernelGGL(plane_moments_kernel, dim3((unsigned)((long)B * tiles)), dim3(GP_THREADS), 0, (hipStream_t)stream, a);
  OCV_CHECK_LAUNCH("ocv_ground_plane_fwd (moments)");
  hipLaunchKernelGGL(plane_solve_kernel, dim3((unsigned)B), dim3(OCV_WAVE), 0, (hipStream_t)stream, a);
  OCV_CHECK_LAUNCH("ocv_ground_plane_fwd (solve)");
  return 0;
}
