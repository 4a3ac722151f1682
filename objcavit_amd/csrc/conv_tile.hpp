// What the split-operand convolution family shares (the arithmetic is described at the head of conv_igemm.hip):
//   conv_igemm.hip     fp32 input, split in registers on its way to LDS (conv_igemm_kernel)
//   conv_dma.hip       pre-split "hl32" input moved by LDS-DMA: the tap ring (conv_split_dma_kernel), the halo-staged 3 x 3
//                      (conv_halo_dma_kernel), the split-K finish pass, their dispatch and ocv_conv_launch
//   conv_winograd.hip  F(4x4, 3x3): transforms around a batch of 36 GEMMs on the tap ring
//   patch_embed.hip    the split patch embedding: 16 GEMMs of the tap ring over one K axis
// Here: the tile sizes, the launch arguments, the (hi, lo) split (the hl32 layout itself: hl_index, common.hpp), and the pieces of a 256 x 128 tile's K
// step and epilogue that the two LDS-DMA kernels have in common -- ONE copy of the MFMA triple, the activation, both
// store passes and the weight-row DMA, so that the kernels' bit-identical results do not rest on copies kept in step by hand.
#pragma once
#include "common.hpp"
#include "lds_dma.hpp"
#include "../../include/objcavit_hip.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 cv_h16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 cv_h16x4 __attribute__((ext_vector_type(4)));

constexpr int CBM = 256, CBN = 128, CBK = 32;             // tile: pixels x output channels per workgroup, channels per K step

struct ConvArgs {
  const float* x1; const float* x2;     // NHWC fp32; x2 (nullable) is concatenated after x1's channels
  const __bf16* xhl;                    // OR the input already split, "hl32" layout (see hl_index)   (DMA kernel)
  __bf16* yhl;                          // optional split copy of the output in the same layout (for the next convolution)
  int Cpo;                              // Cout rounded up to 32 (channel blocks of the split output)
  const __bf16* whi; const __bf16* wlo; // [taps][Cout][Cp]
  const float* bias; const float* res; float* y;
  int C1, C2, Cin, Cp, Cout, H, W, ks, act;
  int Ho, Wo, pad_t, pad_l;             // conv_igemm_kernel: output size, zero padding on top / left (its stride is a template parameter)
  long M;
  int mtiles, ntiles;
  int ksplit;                           // conv_split_dma_kernel: 1, or 2 = the channel chunks are halved between two workgroups
                                        // per tile, each writing raw fp32 partial sums to y + khalf * M * Cout (bias / act /
                                        // residual / split output then belong to conv_splitk_finish_kernel)
  int zbatch;                           // conv_split_dma_kernel: > 1 = that many independent GEMMs in one launch (the 16
  long xz_bytes, wz_bytes;              // Winograd positions): operand z at xhl + z xz_bytes / whi, wlo + z wz_bytes, raw fp32
                                        // result at y + (z ksplit + khalf) * M * Cout
  int zflat;                            // conv_split_dma_kernel, 1 x 1 only: > 0 = the zbatch GEMMs are the consecutive pieces of ONE
                                        // K axis (the patch embedding's 16 patch rows): its zbatch * Cp / 32 steps are cut in zflat
                                        // equal parts, one workgroup per (tile, part), raw fp32 result of part k at y + k * M * Cout
  int f16;                              // conv_split_dma_kernel: != 0 = the operands are fp16 (hi, lo) pairs (conv_split_dma_kernel<true>)
                                        // and so is the split copy of the output (yhl)
  const float* oscale;                  // nullable [Cout]: raw accumulators are multiplied by it before bias / activation (the
                                        // per-output-channel power of two the fp16 weights were scaled by, inverted)
  unsigned* range_flag;                 // nullable: the armed range-guard word (common.hpp ocv_range_note); read only where yhl holds fp16 pairs
  unsigned rowpitch;                    // conv_split_dma_kernel: bytes between consecutive rows of the (B H) x W pixel grid of the
                                        // split input when they are not dense (0 = dense, W * 4 Cp); the patch embedding reads
                                        // every 16th image row of the feature map as one GEMM row grid this way
  int gpt, gpt_inv;                     // conv_split_dma_kernel, 3 x 3 only: > 0 = PACKED TAPS (round 6).  The K axis is the nine taps'
  int Kp;                               // REAL channel granules (8 channels = 16 bytes of hi, 16 of lo) laid end to end, gpt = ceil(Cin / 8)
                                        // per tap, instead of nine chunks of Cp channels: a 32-channel K step holds four granules that may
                                        // belong to two taps (two pixels).  24 input channels: 27 granules = 7 steps instead of 9; 40: 45
                                        // granules = 12 steps instead of 18 (their Cp = 32 / 64 multiply 25 % / 37 % zeros).  The weights
                                        // are ONE [Cout][Kp] matrix in the same granule order, Kp = steps x 32; gpt_inv = a 16.16
                                        // reciprocal of gpt, exact for every granule index of the launch (checked on the host).
  int halo;                             // ocv_conv_launch: != 0 = conv_halo_dma_kernel (3 x 3, H % 8 == 0, W % 32 == 0; mtiles counts its patches)
};

// 16-byte global load (compiler-visible: hipcc tracks it and inserts the s_waitcnt before the first use).
// An earlier version issued these from inline asm with hand-counted waits to keep two register stages in flight;
// the register allocator is free to COPY such a destination register before the load has landed (it did, at the loop
// back-edge), which reads stale data -- a silent, history-dependent corruption.  Never hide an in-flight load.
__device__ __forceinline__ f32x4 gload16(const void* p) { return *reinterpret_cast<const f32x4*>(p); }

__device__ __forceinline__ void split4(const f32x4 v, __bf16* hi, __bf16* lo) {
  const float f[4] = {v[0], v[1], v[2], v[3]};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const __bf16 h = (__bf16)f[i];
    hi[i] = h;
    lo[i] = (__bf16)(f[i] - (float)h);
  }
}

// The same split with FP16 terms (round 4: the decoder's convolutions as two-term fp16 products, 2^-22 instead of 2^-17): hi =
// fp16(v), lo = fp16(v - hi), UNSCALED low term (one accumulator in the GEMM kernel): for |v| below ~0.1 the low term is an fp16
// subnormal (honoured by the MFMA), i.e. the pair's ABSOLUTE error has a floor of 2^-25 ~ 3e-8 -- harmless next to O(1)
// activations, and the reason the weights are scaled per output channel (oscale) while activations are range-checked, not scaled.
// Values beyond +-65504 become inf (loud), never clipped.
__device__ __forceinline__ void split4h(const f32x4 v, _Float16* hi, _Float16* lo) {
  const float f[4] = {v[0], v[1], v[2], v[3]};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const _Float16 h = (_Float16)f[i];
    hi[i] = h;
    lo[i] = (_Float16)(f[i] - (float)h);
  }
}
// two-byte (hi, lo) parts of four values as raw bits, either element type
template <bool F16>
__device__ __forceinline__ void split4_bits(const f32x4 v, unsigned short* hi, unsigned short* lo) {
  if constexpr (F16) split4h(v, reinterpret_cast<_Float16*>(hi), reinterpret_cast<_Float16*>(lo));
  else split4(v, reinterpret_cast<__bf16*>(hi), reinterpret_cast<__bf16*>(lo));
}
__device__ __forceinline__ void split4_bits(const f32x4 v, unsigned short* hi, unsigned short* lo, bool f16) {
  if (f16) split4_bits<true>(v, hi, lo);
  else split4_bits<false>(v, hi, lo);
}
// hi + lo of four consecutive (hi at p, lo at p + lo_off) two-byte pairs, either element type.  The two 8-byte loads are issued
// UNCONDITIONALLY and only the conversion depends on the type: a branch around a load makes hipcc wait for every load on its own
// (the first version of this function did, and the Winograd input transform went from 95 to 120 us per launch).
__device__ __forceinline__ f32x4 join4_bits(const void* p, int lo_off, bool f16) {
  const uint2 hb = *reinterpret_cast<const uint2*>(p);
  const uint2 lb = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned short*>(p) + lo_off);
  f32x4 r;
  if (f16) {
    const cv_h16x4 h = __builtin_bit_cast(cv_h16x4, hb), l = __builtin_bit_cast(cv_h16x4, lb);
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = (float)h[e] + (float)l[e];
  } else {
    r[0] = __uint_as_float(hb.x << 16) + __uint_as_float(lb.x << 16);
    r[1] = __uint_as_float(hb.x & 0xffff0000u) + __uint_as_float(lb.x & 0xffff0000u);
    r[2] = __uint_as_float(hb.y << 16) + __uint_as_float(lb.y << 16);
    r[3] = __uint_as_float(hb.y & 0xffff0000u) + __uint_as_float(lb.y & 0xffff0000u);
  }
  return r;
}

__device__ __forceinline__ float conv_act(float v, int act) {
  if (act == OCV_ACT_LEAKY_RELU) return v > 0.f ? v : 0.01f * v;
  if (act == OCV_ACT_SILU) return fast_silu(v);
  if (act == OCV_ACT_RELU) return fmaxf(v, 0.f);
  return v;
}

// ---------------------------------------------------------------------------
// The LDS-DMA kernels' tile (conv_dma.hip): unpadded 64-byte LDS rows, 16 x 16 x 32 MFMAs, accumulators parked in LDS
// ---------------------------------------------------------------------------
constexpr int DROW = 64;                                        // bytes per LDS row (32 bf16), unpadded
constexpr int DA = CBM * DROW, DB = CBN * DROW;                 // 16384, 8192
constexpr int DBUF = 2 * DA + 2 * DB;                           // 49152 per buffer
constexpr int DNBUF = 3;                                         // 3 x 48 KiB: the DMA runs two K steps ahead

// One split product into one 16 x 16 accumulator: hi hi, hi lo, lo hi, in THIS order (the order is part of the result's bits;
// both LDS-DMA kernels issue it per (i, j) of their 8 x 4 fragments).  F16: the MFMA of the other 2-byte type on the same bytes.
template <bool F16>
__device__ __forceinline__ void mma3(const bf16x8 ah, const bf16x8 al, const bf16x8 bh, const bf16x8 bl, f32x4& acc) {
  if constexpr (F16) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(cv_h16x8, ah), __builtin_bit_cast(cv_h16x8, bh), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(cv_h16x8, ah), __builtin_bit_cast(cv_h16x8, bl), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(cv_h16x8, al), __builtin_bit_cast(cv_h16x8, bh), acc, 0, 0, 0);
  } else {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, acc, 0, 0, 0);
  }
}

// The four B pieces of one K step, issued by producer wavefront pw: weight rows [32 pw, +32), hi at ``slot``, lo at slot + DB.
// rbB[i]: this lane's byte offset (row 32 pw + 16 i + (lane >> 2), its swizzled 16-byte chunk) inside the weight matrix,
// woff: the step's (tap, channel chunk) offset.
__device__ __forceinline__ void conv_issue_weights(const char* whi, const char* wlo, unsigned woff, const unsigned (&rbB)[2],
                                                   unsigned char* slot, int pw) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    unsigned char* dst = slot + (32 * pw + 16 * i) * DROW;
    __builtin_amdgcn_global_load_lds((gptr_t)(whi + woff + rbB[i]), (lptr_t)dst, 16, 0, 0);
    __builtin_amdgcn_global_load_lds((gptr_t)(wlo + woff + rbB[i]), (lptr_t)(dst + DB), 16, 0, 0);
  }
}

// ---- epilogue.  accumulator (i, j): register r of lane l is output row 16 i + 4 (l >> 4) + r, column 16 j + (l & 15)
// Storing straight from that layout costs 384 two- and four-byte store instructions per wavefront in 32- / 64-byte
// runs; it was store-ISSUE-bound and, with one workgroup per CU, fully exposed: 23 % of the 128 -> 128 launches
// (ablation: 1.63 -> 1.26 ms without the stores).  Instead the raw tile goes through the consumer wavefront's own 34 KB of
// the (now idle) LDS (the parking loop in each kernel) and leaves, from all eight wavefronts (conv_store_rows), as 16-byte-per-lane stores.
constexpr int ERS = 68;                                       // floats per LDS row: 64 + 4 -> conflict-free writes

// Second half of the epilogue of conv_split_dma_kernel, run by ALL EIGHT wavefronts: the four consumers have parked
// their raw accumulators in LDS (one 128 x 64 fp32 image of ERS-float rows each); wavefront w turns rows
// [64 (w >> 2), +64) of consumer (w & 3)'s image into bias + activation (+ residual) and 16-byte stores, lane = (row
// it * 8 + (lane >> 3), channel octet lane & 7).  Stamps (tools/run_conv_split.py, -DOCV_STAMPS) had put the epilogue
// at 20 K cycles per tile when the four consumer wavefronts did all of it while the producers idled -- instruction
// issue on one wavefront per SIMD, not memory: 19 % of a 128 -> 128 tile at 240 x 320.
// ``rowm(R)``: the output pixel (row of the M x Cout result) of tile row R in [0, 256), >= p.M where the tile has none.
template <bool F16, class RowMap>
__device__ __forceinline__ void conv_store_rows(const ConvArgs& p, const unsigned char* lds, int wave, int lane, RowMap rowm, int n0,
                                                long yoff) {
  const int cw = wave & 3, half = wave >> 2;
  const int wm = cw >> 1, wn = cw & 1;
  const float* tile = reinterpret_cast<const float*>(lds) + cw * (128 * ERS);
  const int oct = lane & 7, rsub = lane >> 3;
  const int ncol = n0 + wn * 64 + oct * 8;
  if (ncol >= p.Cout) return;
  float bv[8], sv[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    bv[e] = p.bias != nullptr ? p.bias[ncol + e] : 0.f;
    sv[e] = p.oscale != nullptr ? p.oscale[ncol + e] : 1.f;
  }
  float amax = 0.f;                               // largest magnitude written as an fp16 pair (range guard, common.hpp)
#pragma unroll 4
  for (int it = 0; it < 8; ++it) {
    const int row = half * 64 + it * 8 + rsub;
    const long m = rowm(wm * 128 + row);
    if (m >= p.M) continue;
    f32x4 a = *reinterpret_cast<const f32x4*>(tile + row * ERS + oct * 8);
    f32x4 c = *reinterpret_cast<const f32x4*>(tile + row * ERS + oct * 8 + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      a[e] = conv_act(fmaf(a[e], sv[e], bv[e]), p.act);            // (sv = 1: exact, the product of round 3)
      c[e] = conv_act(fmaf(c[e], sv[4 + e], bv[4 + e]), p.act);
    }
    const long o = m * p.Cout + ncol;
    if (p.res != nullptr) {
      a += *reinterpret_cast<const f32x4*>(p.res + o);
      c += *reinterpret_cast<const f32x4*>(p.res + o + 4);
    }
    if (p.y != nullptr) {
      *reinterpret_cast<f32x4*>(p.y + yoff + o) = a;
      *reinterpret_cast<f32x4*>(p.y + yoff + o + 4) = c;
    }
    if (p.yhl != nullptr) {
      __attribute__((aligned(16))) unsigned short hi[8], lo[8];
      split4_bits<F16>(a, hi, lo);
      split4_bits<F16>(c, hi + 4, lo + 4);
      if constexpr (F16) amax = ocv_amax4(ocv_amax4(amax, a), c);
      const long oh = hl_index(m, ncol, p.Cpo);          // ncol % 8 == 0: the octet stays inside one 32-block
      *reinterpret_cast<bf16x8*>(p.yhl + oh) = *reinterpret_cast<bf16x8*>(hi);
      *reinterpret_cast<bf16x8*>(p.yhl + oh + 32) = *reinterpret_cast<bf16x8*>(lo);
    }
  }
  if constexpr (F16) ocv_range_note(p.range_flag, amax);
}

// Cout not a multiple of 8: the consumers store element-wise, straight from the accumulator layout (wm, wn: the consumer's
// place in the 2 x 2 over the tile; rowm as for conv_store_rows; ``rows``: tile rows [0, rows) have a pixel).  Register
// allocation of the 128 accumulators plus this body sits at the 256-VGPR limit, and two details keep the fp16 instances out
// of scratch: ``p`` BY VALUE (through a reference every store may alias the arguments, which are then re-read: 356 bytes per
// lane), and the ragged last tile tested on the 32-bit tile row, which folds away where ``rows`` is the constant 256 (a 64-bit
// m < p.M per element cost the halo kernel 116 bytes per lane).
template <bool F16, class RowMap>
__device__ __forceinline__ void conv_store_elems(const ConvArgs p, const f32x4 (&acc)[8][4], RowMap rowm, int rows, int wm, int wn,
                                                 int lane, int n0, long yoff) {
  const int l15 = lane & 15, q4 = lane >> 4;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = n0 + wn * 64 + j * 16 + l15;
    const bool nok = n < p.Cout;
    const float bv = (p.bias != nullptr && nok) ? p.bias[n] : 0.f;
    const float sv = (p.oscale != nullptr && nok) ? p.oscale[n] : 1.f;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int R = wm * 128 + i * 16 + 4 * q4 + r;
        const long m = rowm(R);
        if (nok && R < rows) {
          float v = conv_act(fmaf(acc[i][j][r], sv, bv), p.act);
          if (p.res != nullptr) v += p.res[m * p.Cout + n];
          if (p.y != nullptr) p.y[yoff + m * p.Cout + n] = v;
          if (p.yhl != nullptr) {
            if constexpr (F16) ocv_range_note(p.range_flag, fabsf(v));
            unsigned short* yh = reinterpret_cast<unsigned short*>(p.yhl) + hl_index(m, n, p.Cpo);
            ocv_split1<F16>(v, yh[0], yh[32]);
          }
        }
      }
  }
}

// Launch of conv_split_dma_kernel, or of conv_halo_dma_kernel where ConvArgs::halo is set (conv_dma.hip): fills Cp, M and the
// tile counts from the sizes; the pixel grid is B x a.H x a.W.  0 / hipError_t.
int ocv_conv_launch(ConvArgs& a, int B, hipStream_t st);
