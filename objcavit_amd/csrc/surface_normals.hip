// Surface normals of the predict path's final map (Statement N of include/objcavit_hip.h): the least-squares
// plane slope of z over a (2r + 1)^2 window, turned into the unit normal of the back-projected surface, with a validity mask that
// refuses windows that leave the map, hold a non-finite or out-of-range depth, or straddle a depth discontinuity.
//   depth [B][1][H][W], K [B][4] = fx, fy, cx, cy -> normals [B][3][H][W] fp32, normals_rgb8 [B][H][W][3], valid [B][H][W]
// The dense launch, one 256-thread workgroup (4 waves, one per SIMD) per 64 x 16 output tile, r a template parameter (1..4):
//   stage   the (64 + 2r) x (16 + 2r) tile + halo ONCE into LDS with coalesced 4-byte loads, all of a thread's loads (at most 7) in
//           flight before the first LDS write; a cell outside the map is NaN, so it fails the finite test like any bad depth and the
//           "window inside the map" rule needs no test of its own;
//   pass 1  per (row, column) of the 16 + 2r staged rows: ramp sum_i i (z(x + i) - z(x - i)), box sum, min and max of the 2r + 1
//           horizontal neighbours, back to LDS.  The finite flag rides in the min: NaN iff a neighbour is not finite (a min of finite
//           values is never NaN), which saves a fifth array;
//   pass 2  per output pixel, a thread owning 4 consecutive columns of one row (ds_read_b128 of the pass-1 rows): zu = sum of the
//           2r + 1 ramps / D, zv = sum_j j (box(y + j) - box(y - j)) / D, the window's min / max, the predicate, one v_rsq_f32 per
//           pixel, the stores.
// LDS per workgroup = 4 (16 + 2r) (64 + 2r) + 4 * 4 (16 + 2r) 64 bytes:
//   r = 1: 23 184 B -> 7 workgroups / CU = 7 waves / SIMD      r = 2: 25 920 B -> 6      r = 3: 28 688 B -> 5      r = 4: 31 488 B -> 5
// (160 KiB per CU).  VGPRs: 56 / 81 / 59 / 59, so registers allow 8 / 5 / 8 / 8 and the kernels run at 7 / 5 / 5 / 5 waves per SIMD
// (r = 2 is bounded by the 16 ds_read_b128 its unrolled pass 2 keeps in flight, the others by LDS).  The halo makes a workgroup read
// (64 + 2r)(16 + 2r) / 1024 = 1.29 (r = 2) to 1.69 (r = 4) times its tile, the excess out of L2 (neighbouring tiles).
// Stores.  With W % 4 == 0 (and aligned bases; every dataset size) a thread's 4 pixels are ONE global_store_dwordx4 per plane of
// normals (16 lanes = 256 contiguous bytes per tile row), ONE global_store_dwordx3 of normals_rgb8 -- 4 pixels are 12 consecutive bytes at
// a 4-byte aligned offset, so the picture is packed in registers and written PER THREAD, not through LDS: the ISA shows one 12-byte
// store per thread whose lanes are contiguous (192 bytes per 16 lanes), which an LDS transpose could only widen to 16 bytes at the cost
// of a barrier -- and ONE global_store_dword of valid.  Any other W takes the scalar stores (4 / 1-byte) of the same values.
// The gather launch writes a normal per point of the cloud: out[b][i] = (nx, ny, nz, 0) as one 16-byte store for i < counts[b].
// No atomics, no workspace, nothing read on the host; every value is a function of the inputs in a fixed order: two calls, same bytes.
#include "common.hpp"
#include "../../include/objcavit_hip.h"

#include <float.h>

namespace {

constexpr int SN_TW = 64, SN_TH = 16, SN_THREADS = 256, SN_PX = 4;           // tile, threads, consecutive pixels per thread in pass 2
static_assert(SN_TW / SN_PX * SN_TH == SN_THREADS, "pass 2: one thread per 4 x 1 pixels of the tile");

struct NormalsArgs {
  const float *depth, *K;
  float* normals;
  uint8_t *rgb8, *valid;
  int H, W, tx, ty;                   // tiles along x / y
  float near, far, edge;
  int vec;                            // W % 4 == 0 and the given outputs aligned for the wide stores
};

__device__ __forceinline__ bool sn_finite(float v) { return fabsf(v) <= FLT_MAX; }

__device__ __forceinline__ unsigned sn_byte(float n) { return (unsigned)fminf(fmaxf(rintf(fmaf(127.5f, n, 127.5f)), 0.f), 255.f); }

template <int R>
__global__ __launch_bounds__(SN_THREADS) void depth_normals_kernel(NormalsArgs p) {
  constexpr int SW = SN_TW + 2 * R, SH = SN_TH + 2 * R, CELLS = SH * SW, NS = (CELLS + SN_THREADS - 1) / SN_THREADS;
  constexpr int ITEMS = SH * SN_TW, NP = ITEMS / SN_THREADS;                 // pass 1: NP whole rounds of 256 items, and for an odd r half
  static_assert(ITEMS % 128 == 0, "pass 1 ends on a wave pair's boundary");  // a round more (18 / 22 staged rows): whole waves sit it out
  constexpr int UNROLL_V = R <= 2 ? R : 1;
  constexpr float INV_D =1.0f / (float)((2 * R + 1) * 2 * (R * (R + 1) * (2 * R + 1) / 6));
  __shared__ float s_z[SH][SW];
  __shared__ __attribute__((aligned(16))) float s_ramp[SH][SN_TW], s_box[SH][SN_TW], s_min[SH][SN_TW], s_max[SH][SN_TW];

  const int tid = threadIdx.x;
  const int tile_x = blockIdx.x % p.tx, rest = blockIdx.x / p.tx, tile_y = rest % p.ty, b = rest / p.ty;
  const long HW = (long)p.H * p.W;
  const float nan = __uint_as_float(0x7fc00000u);

  // stage: tile + halo, out-of-map cells NaN
  {
    const float* src = p.depth + b * HW;
    const int gx0 = tile_x * SN_TW - R, gy0 = tile_y * SN_TH - R;
    float v[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const int i = tid + k * SN_THREADS, row = i / SW, col = i - row * SW, y = gy0 + row, x = gx0 + col;
      v[k] = (i < CELLS && (unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W) ? src[(long)y * p.W + x] : nan;
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const int i = tid + k * SN_THREADS;
      if (i < CELLS) (&s_z[0][0])[i] = v[k];
    }
  }
  __syncthreads();

  // pass 1: the 2r + 1 horizontal neighbours of every staged row
#pragma unroll
  for (int k = 0; k <= NP; ++k) {
    const int i = tid + k * SN_THREADS;
    if (k == NP && i >= ITEMS) break;
    const int row = i / SN_TW, col = i % SN_TW;
    const float zc = s_z[row][col + R];
    float ramp = 0.f, box = zc, mn = zc, mx = zc;
    bool fin = sn_finite(zc);
#pragma unroll
    for (int d = 1; d <= R; ++d) {
      const float a = s_z[row][col + R + d], c = s_z[row][col + R - d];
      ramp = fmaf((float)d, a - c, ramp);                                    // the difference first: it is small and nearly exact
      box += a + c;
      mn = fminf(mn, fminf(a, c));
      mx = fmaxf(mx, fmaxf(a, c));
      fin = fin && sn_finite(a) && sn_finite(c);
    }
    s_ramp[row][col] = ramp;
    s_box[row][col] = box;
    s_min[row][col] = fin ? mn : nan;
    s_max[row][col] = mx;
  }
  __syncthreads();

  // pass 2: 4 consecutive pixels of one row per thread
  const int ly = tid / (SN_TW / SN_PX), lx = (tid % (SN_TW / SN_PX)) * SN_PX;
  const int y = tile_y * SN_TH + ly, x0 = tile_x * SN_TW + lx;
  if (y >= p.H || x0 >= p.W) return;

  float su[SN_PX], sv[SN_PX], wmin[SN_PX], wmax[SN_PX];
  bool ok[SN_PX];
  {
    const float4 r0 = *reinterpret_cast<const float4*>(&s_ramp[ly + R][lx]);
    const float4 m0 = *reinterpret_cast<const float4*>(&s_min[ly + R][lx]);
    const float4 M0 = *reinterpret_cast<const float4*>(&s_max[ly + R][lx]);
    const float r_[SN_PX] = {r0.x, r0.y, r0.z, r0.w}, m_[SN_PX] = {m0.x, m0.y, m0.z, m0.w}, M_[SN_PX] = {M0.x, M0.y, M0.z, M0.w};
#pragma unroll
    for (int c = 0; c < SN_PX; ++c) {
      su[c] = r_[c]; sv[c] = 0.f; wmin[c] = m_[c]; wmax[c] = M_[c];
      ok[c] = m_[c] == m_[c];
    }
  }
  // (r >= 3 keeps this loop rolled: unrolled, the scheduler hoists all 8 r ds_read_b128 and r = 4 takes 145 VGPRs = 3 waves per SIMD)
#pragma unroll UNROLL_V
  for (int d = 1; d <= R; ++d) {
    const float4 ra = *reinterpret_cast<const float4*>(&s_ramp[ly + R + d][lx]), rc = *reinterpret_cast<const float4*>(&s_ramp[ly + R - d][lx]);
    const float4 ba = *reinterpret_cast<const float4*>(&s_box[ly + R + d][lx]), bc = *reinterpret_cast<const float4*>(&s_box[ly + R - d][lx]);
    const float4 ma = *reinterpret_cast<const float4*>(&s_min[ly + R + d][lx]), mc = *reinterpret_cast<const float4*>(&s_min[ly + R - d][lx]);
    const float4 Ma = *reinterpret_cast<const float4*>(&s_max[ly + R + d][lx]), Mc = *reinterpret_cast<const float4*>(&s_max[ly + R - d][lx]);
    const float ra_[SN_PX] = {ra.x, ra.y, ra.z, ra.w}, rc_[SN_PX] = {rc.x, rc.y, rc.z, rc.w};
    const float ba_[SN_PX] = {ba.x, ba.y, ba.z, ba.w}, bc_[SN_PX] = {bc.x, bc.y, bc.z, bc.w};
    const float ma_[SN_PX] = {ma.x, ma.y, ma.z, ma.w}, mc_[SN_PX] = {mc.x, mc.y, mc.z, mc.w};
    const float Ma_[SN_PX] = {Ma.x, Ma.y, Ma.z, Ma.w}, Mc_[SN_PX] = {Mc.x, Mc.y, Mc.z, Mc.w};
#pragma unroll
    for (int c = 0; c < SN_PX; ++c) {
      su[c] += ra_[c] + rc_[c];
      sv[c] = fmaf((float)d, ba_[c] - bc_[c], sv[c]);
      ok[c] = ok[c] && ma_[c] == ma_[c] && mc_[c] == mc_[c];
      wmin[c] = fminf(wmin[c], fminf(ma_[c], mc_[c]));
      wmax[c] = fmaxf(wmax[c], fmaxf(Ma_[c], Mc_[c]));
    }
  }

  const float4 k = *reinterpret_cast<const float4*>(p.K + 4 * (long)b);
  const bool camera = sn_finite(k.x) && k.x > 0.f && sn_finite(k.y) && k.y > 0.f && sn_finite(k.z) && sn_finite(k.w);
  const float dy = (float)y - k.w;
  float n[3][SN_PX];
  unsigned vbits = 0u;
#pragma unroll
  for (int c = 0; c < SN_PX; ++c) {
    const float zc = s_z[ly + R][lx + R + c];
    // the predicate: every statement rounded to fp32 on its own (the library is built with contraction on)
    const float t = __fmul_rn(p.edge, zc);
    const bool on = camera && ok[c] && p.near <= wmin[c] && wmax[c] <= p.far && __fsub_rn(wmax[c], zc) <= t && __fsub_rn(zc, wmin[c]) <= t;
    const float zu = su[c] * INV_D, zv = sv[c] * INV_D;
    const float dx = (float)(x0 + c) - k.z;
    float m0 = k.x * zu, m1 = k.y * zv, m2 = -(zc + dx * zu + dy * zv);
    const float s = m0 * m0 + m1 * m1 + m2 * m2;
    const float inv = __builtin_amdgcn_rsqf(s);
    if (s == 0.f) { m0 = 0.f; m1 = 0.f; m2 = -1.f; } else { m0 *= inv; m1 *= inv; m2 *= inv; }
    n[0][c] = on ? m0 : 0.f;
    n[1][c] = on ? m1 : 0.f;
    n[2][c] = on ? m2 : 0.f;
    vbits |= on ? 1u << c : 0u;
  }

  const long at = b * HW + (long)y * p.W + x0;                               // pixel index within the batch
  if (p.vec) {                                                               // W % 4 == 0: the 4 pixels are inside the map
    if (p.normals != nullptr) {
      float* o = p.normals + 2 * b * HW + at;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) *reinterpret_cast<float4*>(o + ch * HW) = make_float4(n[ch][0], n[ch][1], n[ch][2], n[ch][3]);
    }
    if (p.rgb8 != nullptr) {
      unsigned by[3 * SN_PX];
#pragma unroll
      for (int c = 0; c < SN_PX; ++c)
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) by[3 * c + ch] = ((vbits >> c) & 1u) ? sn_byte(n[ch][c]) : 0u;
      unsigned* o = reinterpret_cast<unsigned*>(p.rgb8 + 3 * at);
#pragma unroll
      for (int w = 0; w < 3; ++w) o[w] = by[4 * w] | (by[4 * w + 1] << 8) | (by[4 * w + 2] << 16) | (by[4 * w + 3] << 24);
    }
    if (p.valid != nullptr)
      *reinterpret_cast<unsigned*>(p.valid + at) = (vbits & 1u) | ((vbits & 2u) << 7) | ((vbits & 4u) << 14) | ((vbits & 8u) << 21);
    return;
  }
#pragma unroll
  for (int c = 0; c < SN_PX; ++c) {
    if (x0 + c >= p.W) break;
    const bool on = (vbits >> c) & 1u;
    if (p.normals != nullptr) {
      float* o = p.normals + 2 * b * HW + at + c;
      o[0] = n[0][c]; o[HW] = n[1][c]; o[2 * HW] = n[2][c];
    }
    if (p.rgb8 != nullptr) {
      uint8_t* o = p.rgb8 + 3 * (at + c);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) o[ch] = on ? (uint8_t)sn_byte(n[ch][c]) : (uint8_t)0;
    }
    if (p.valid != nullptr) p.valid[at + c] = on ? 1 : 0;
  }
}

struct GatherArgs {
  const float* normals;
  const int *pixel, *counts;
  float* out;
  int HW, cap, chunks;                // chunks of 256 rows per image
};

__global__ __launch_bounds__(SN_THREADS) void normals_gather_kernel(GatherArgs p) {
  const int b = blockIdx.x / p.chunks, i = (blockIdx.x - b * p.chunks) * SN_THREADS + threadIdx.x;
  const int n = min(p.counts[b], p.cap);
  if (i >= n) return;
  const long row = (long)b * p.cap + i;
  const int pix = p.pixel[row];
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if ((unsigned)pix < (unsigned)p.HW) {
    const float* s = p.normals + 3 * (long)b * p.HW + pix;
    v = make_float4(s[0], s[p.HW], s[2 * (long)p.HW], 0.f);
  }
  *reinterpret_cast<float4*>(p.out + 4 * row) = v;
}

}  // namespace

extern "C" int ocv_depth_normals_fwd(const float* depth, const float* K, int H, int W, int r, float near, float far, float edge_ratio,
                                     float* normals, uint8_t* normals_rgb8, uint8_t* valid, int B, ocv_stream_t stream) {
  OCV_CHECK_ARG(depth && K, "ocv_depth_normals_fwd: null pointer (depth, K)");
  OCV_CHECK_ARG(normals || normals_rgb8 || valid, "ocv_depth_normals_fwd: no output (normals, normals_rgb8, valid are all null)");
  OCV_CHECK_ARG(r >= 1 && r <= 4, "ocv_depth_normals_fwd: radius = %d must be in 1..4", r);
  OCV_CHECK_ARG(B >= 1 && H >= 1 && W >= 1, "ocv_depth_normals_fwd: bad sizes (B, H, W must be >= 1)");
  const long tx = ocv_cdiv(W, SN_TW), ty = ocv_cdiv(H, SN_TH);
  OCV_CHECK_ARG((long)H * W <= 0x7fffffffL && (long)B * tx * ty <= 0x7fffffffL,
                "ocv_depth_normals_fwd: bad sizes (H * W and B * tiles below 2^31)");
  OCV_CHECK_ARG(near <= far, "ocv_depth_normals_fwd: near = %g must be <= far = %g", (double)near, (double)far);
  OCV_CHECK_ARG(edge_ratio > 0.f, "ocv_depth_normals_fwd: edge_ratio = %g must be > 0", (double)edge_ratio);
  OCV_CHECK_ARG(ocv_aligned16(K), "ocv_depth_normals_fwd: K must be 16-byte aligned");
  OCV_CHECK_ARG(((reinterpret_cast<uintptr_t>(depth) | reinterpret_cast<uintptr_t>(normals)) & 3) == 0,
                "ocv_depth_normals_fwd: misaligned pointer (depth, normals)");
  NormalsArgs a{};
  a.depth = depth; a.K = K; a.normals = normals; a.rgb8 = normals_rgb8; a.valid = valid;
  a.H = H; a.W = W; a.tx = (int)tx; a.ty = (int)ty;
  a.near = near; a.far = far; a.edge = edge_ratio;
  a.vec = W % 4 == 0 && ocv_aligned16(normals) && ((reinterpret_cast<uintptr_t>(normals_rgb8) | reinterpret_cast<uintptr_t>(valid)) & 3) == 0;
  const dim3 grid((unsigned)((long)B * tx * ty)), block(SN_THREADS);
  switch (r) {
    case 1: hipLaunchKernelGGL(depth_normals_kernel<1>, grid, block, 0, (hipStream_t)stream, a); break;
    case 2: hipLaunchKernelGGL(depth_normals_kernel<2>, grid, block, 0, (hipStream_t)stream, a); break;
    case 3: hipLaunchKernelGGL(depth_normals_kernel<3>, grid, block, 0, (hipStream_t)stream, a); break;
    default: hipLaunchKernelGGL(depth_normals_kernel<4>, grid, block, 0, (hipStream_t)stream, a); break;
  }
  OCV_CHECK_LAUNCH("ocv_depth_normals_fwd");
  return 0;
}

extern "C" int ocv_normals_gather_fwd(const float* normals, const int* pixel, const int* counts, int H, int W, int cap, float* out, int B,
                                      ocv_stream_t stream) {
  OCV_CHECK_ARG(normals && pixel && counts && out, "ocv_normals_gather_fwd: null pointer (normals, pixel, counts, out)");
  OCV_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && cap >= 1, "ocv_normals_gather_fwd: bad sizes (B, H, W, cap must be >= 1)");
  const long chunks = ocv_cdiv(cap, SN_THREADS);
  OCV_CHECK_ARG((long)H * W <= 0x7fffffffL && (long)B * cap <= 0x7fffffffL && (long)B * chunks <= 0x7fffffffL,
                "ocv_normals_gather_fwd: bad sizes (H * W and B * cap below 2^31)");
  OCV_CHECK_ARG(ocv_aligned16(out), "ocv_normals_gather_fwd: out must be 16-byte aligned");
  OCV_CHECK_ARG(((reinterpret_cast<uintptr_t>(normals) | reinterpret_cast<uintptr_t>(pixel) | reinterpret_cast<uintptr_t>(counts)) & 3) == 0,
                "ocv_normals_gather_fwd: misaligned pointer (normals, pixel, counts)");
  GatherArgs a{};
  a.normals = normals; a.pixel = pixel; a.counts = counts; a.out = out;
  a.HW = H * W; a.cap = cap; a.chunks = (int)chunks;
  hipLaunchKernelGGL(normals_gather_kernel, dim3((unsigned)((long)B * chunks)), dim3(SN_THREADS), 0, (hipStream_t)stream, a);
  OCV_CHECK_LAUNCH("ocv_normals_gather_fwd");
  return 0;
}
