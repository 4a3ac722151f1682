// What the MBConv path of the encoders shares (the sibling of conv_tile.hpp and token_tile.hpp):
//   pointwise_split.hip  1 x 1 convolution, fp32 rows split on the fly (pw_rows / pw_stream / pw_tile kernels)
//   pointwise_hl.hip     1 x 1 convolution on rows that arrive split ("hl32", LDS-DMA), gate folded into per-image weights
//   mbconv_fused.hip     expand 1 x 1 + depthwise in one kernel
//   depthwise_se.hip     depthwise + squeeze-excite pooling partials (register window / LDS rows)
//   se_gate.hip          everything squeeze-excite: pooling, hidden layer, gate, gate folded into packed weights
//   encoder_nhwc.hip     exact-fp32 1 x 1, plain depthwise
// Here: the vector types, the two-term bf16 split (8-wide into MFMA operands, 4-wide into the hl32 layout), the three-MFMA product,
// the address of a packed weight fragment -- ONE copy each, so that the kernels' bit-identical results (the split depthwise output
// against the fp32 one, the packed per-image weights against hip_ops.SplitWeight) do not rest on copies kept in step by hand -- and the
// host-side pieces the launchers share.  A site that is still written out in a kernel is one where the helper changed that kernel's
// instruction stream in every form tried: profiles/mbconv_tile_refactor.txt lists them.
#pragma once
#include "common.hpp"
#include "lds_dma.hpp"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bf16x8 ldb8(const __bf16* p) { return *reinterpret_cast<const bf16x8*>(p); }

__device__ __forceinline__ float4 mul4(float4 a, const float4 g) {
  a.x *= g.x; a.y *= g.y; a.z *= g.z; a.w *= g.w;
  return a;
}
__device__ __forceinline__ float4 fma4(const float4 w, const float4 v, float4 a) {
  a.x = fmaf(w.x, v.x, a.x); a.y = fmaf(w.y, v.y, a.y); a.z = fmaf(w.z, v.z, a.z); a.w = fmaf(w.w, v.w, a.w);
  return a;
}
__device__ __forceinline__ float4 silu4(float4 r) {
  r.x = fast_silu(r.x); r.y = fast_silu(r.y); r.z = fast_silu(r.z); r.w = fast_silu(r.w);
  return r;
}

// 8 consecutive floats (two 16-byte vectors) -> bf16 hi / lo octets: hi = bf16(v), lo = bf16(v - hi)
__device__ __forceinline__ void split8(const float4 u, const float4 v, bf16x8& hi, bf16x8& lo) {
  const float f[8] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const __bf16 h = (__bf16)f[i];
    hi[i] = h;
    lo[i] = (__bf16)(f[i] - (float)h);
  }
}

// The same split of 4 consecutive channels: what the hl32 layout (hl_at, common.hpp) holds as a hi quad at its place and a
// lo quad 32 elements on.  (The two 8-byte stores stay at the call sites: behind a helper that takes the address, the address is
// formed before the conversions and three of the pointwise kernels' streams change.)
__device__ __forceinline__ void split4(const float4 v, bf16x4& hi, bf16x4& lo) {
  const float f[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const __bf16 h = (__bf16)f[e];
    hi[e] = h;
    lo[e] = (__bf16)(f[e] - (float)h);
  }
}

// One split product into a 32 x 32 accumulator: hi hi + hi lo + lo hi on v_mfma_f32_32x32x16_bf16, in THIS order (the order is
// part of the result's bits); the dropped lo lo term is 2^-18 relative.
__device__ __forceinline__ f32x16 mfma3(const bf16x8 ah, const bf16x8 al, const bf16x8 bh, const bf16x8 bl, f32x16 acc) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
  return acc;
}

// Packed weights (hip_ops.SplitWeight on the host, se_gate_weights_kernel per image on the device): the B operand of
// v_mfma_f32_32x32x16_bf16 for channel tile jt (32 channels) and K step s (16 inputs) of nsteps = Kp / 16 is ONE contiguous 1 KB
// fragment -- lane l = 32 hh + l31 holds W[32 jt + l31][16 s + 8 hh .. + 7] -- hi fragment first, lo fragment right behind it:
//   wp[((jt * nsteps + s) * 2 + part) * 512 + lane * 8 + e]
// so a wavefront's weight load touches 8 consecutive cache lines instead of 32 scattered ones (with row-major [N][K] weights the
// per-line tag work of those loads, not bandwidth, was the largest single cost of the tile kernel).  This is the address
// of lane ``lane``'s hi octet in the matrix at ``wp``; + 512: its lo octet, + 1024: the next K step.  The readers and the
// device-side writer both use it (T = const __bf16 / __bf16).  (It takes Kp and shifts inside: with nsteps formed at the call
// site the K-group instances of pw_tile_kernel come out in another instruction order.)
template <class T>
__device__ __forceinline__ T* w_frag(T* wp, int jt, int Kp, int s, int lane) {
  return wp + (((long)jt * (Kp >> 4) + s) * 2) * 512 + lane * 8;
}

// Transpose scratch of the pointwise epilogues (store_tile_lds, ph_store_tile): a 32 x 32 accumulator tile goes through 4 KB of
// LDS owned by the wavefront and leaves as 16-byte stores of 8 rows x 128 B.  Rows are UNPADDED (32 floats): the ds_write_b32 of
// a 32-lane half covers one row = 32 consecutive banks, and each 16-lane group of the ds_read_b128 ({0-3, 12-15, 20-27}, ...)
// covers whole 256-byte bank rows -- one LDS cycle per group; padded rows of 40 floats cost three (MI355X_MICROARCH.md, LDS table).
constexpr int TS = 32;                          // floats per LDS row of the transpose scratch
constexpr int TSCRATCH = 32 * TS;               // floats per wavefront

// XCD-aware, bijective workgroup -> (tile, chunk, image) map of the depthwise kernels: consecutive workgroup ids go round-robin
// to the 8 XCDs, and neighbouring work items share halo rows / columns through their XCD's own L2.  Every XCD gets a contiguous
// run of tiles (whole images at bs = 16); tile fastest, then the channel chunk, then the image.
__device__ __forceinline__ void dw_xcd_decode(int tiles, int chunks, int& tile, int& chunk, long& b) {
  const int wg = ocv_xcd_remap(blockIdx.x, gridDim.x);
  tile = wg % tiles;
  const int rest = wg / tiles;
  chunk = rest % chunks;
  b = rest / chunks;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// Lets ``Kernel`` be launched with up to ``bytes`` of dynamic LDS; set once per kernel and process.
template <auto Kernel>
inline void ocv_allow_dynamic_lds(int bytes = 160 * 1024) {
  static const hipError_t once = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  (void)once;
}

// What every NHWC depthwise entry point asks of its geometry, with ``name`` (the entry point) in front of each message:
// sizes, kernel / stride, padding, an output no larger than the padded input allows, 16-byte alignment (``aligned``: of the
// entry point's own operands).  ``quad_channels``: the kernel walks C channels in quads, so C is a multiple of 4 (false: the entry
// point checks its channel counts itself -- the fused kernel -- and C is not looked at).  0, or -1 with ocv_last_error set.
inline int ocv_check_dw_geometry(const char* name, bool quad_channels, int B, int C, int H, int W, int k, int stride, int pad_t,
                                 int pad_l, int Ho, int Wo, bool aligned) {
  const bool sizes = B >= 1 && H >= 1 && W >= 1 && Ho >= 1 && Wo >= 1;
  if (quad_channels)
    OCV_CHECK_ARG(sizes && C >= 4 && C % 4 == 0, "%s: bad sizes (C must be a multiple of 4)", name);
  else
    OCV_CHECK_ARG(sizes, "%s: bad sizes", name);
  OCV_CHECK_ARG((k == 3 || k == 5) && (stride == 1 || stride == 2), "%s: k must be 3 or 5 and stride 1 or 2 (got k=%d s=%d)", name, k, stride);
  OCV_CHECK_ARG(pad_t >= 0 && pad_l >= 0 && pad_t < k && pad_l < k, "%s: bad padding", name);
  OCV_CHECK_ARG((Ho - 1) * stride - pad_t < H && (Wo - 1) * stride - pad_l < W, "%s: output larger than the padded input allows", name);
  OCV_CHECK_ARG(aligned, "%s: operands must be 16-byte aligned", name);
  return 0;
}
