// 3x3 implicit-GEMM convolution with STRIDE 1 or 2 and explicit (pad_t, pad_l) on NHWC fp32 activations, gfx950:
// the dense 3x3 of EfficientNetV2's Fused-MBConv blocks (torchvision's symmetric padding; stride 2 in the first block
// of stages 2 and 3: 24 -> 96 at 240 x 320 -> 120 x 160, 48 -> 192 at 120 x 160 -> 60 x 80).
//
// Same arithmetic and the same workgroup structure as conv_igemm_kernel (conv_igemm.hip, whose kernels stay stride 1 /
// "same" and unchanged): split-bf16 operands, three v_mfma_f32_32x32x16_bf16 per 32x32x16 block (a_hi b_hi + a_hi b_lo +
// a_lo b_hi), fp32 accumulation; 256 pixels x 128 channels per workgroup, K = (32-channel chunk outer, tap inner)
// through a double-buffered LDS image; waves 0-3 consumers (MFMAs only), waves 4-7 two alternating producer groups
// (gather, fp32 -> hi/lo split, LDS writes).  What changes is the gather only: output pixel (b, oy, ox) reads input
// pixel (b, S oy - pad_t + ky, S ox - pad_l + kx), so the per-row base is that of the window's top-left corner (a
// 32-bit byte offset that may wrap below zero: it is only ever used with an in-image tap, whose sum is in range) and the
// per-tap offset (ky W + kx) Cin 4 is non-negative.  The per-row 9-bit mask of in-image taps makes every padded tap
// read a zero page.
// The schedule is a copy of conv_igemm_kernel's (conv_igemm.hip points back here): a fix to one belongs in both.
// Epilogue: + bias (folded BN), activation, + optional residual [B, Ho, Wo, Cout], fp32 NHWC store.
// Weights: the [9][Cout][Cp] bf16 (hi, lo) pair of hip_ops.prep_conv_weight, Cp = Cin rounded up to 32.
#include <stdlib.h>

#include "common.hpp"
#include "../../include/objcavit_hip.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int CBM = 256, CBN = 128, CBK = 32;
constexpr int ROWB = 80;                                  // bytes per LDS row (64 data + 16 pad)
constexpr int A_BYTES = CBM * ROWB, B_BYTES = CBN * ROWB;
constexpr int BUF_BYTES = 2 * A_BYTES + 2 * B_BYTES;      // 61440

struct StridedArgs {
  const float* x;                       // [B][H][W][Cin] fp32
  const __bf16* whi; const __bf16* wlo; // [9][Cout][Cp]
  const float* bias; const float* res; float* y;
  int Cin, Cp, Cout, H, W, Ho, Wo, stride, pad_t, pad_l, act;
  long M;                               // B Ho Wo
  int mtiles, ntiles;
};

__device__ __attribute__((aligned(256))) float cs_zero_page[64];      // zero-initialised: source of padded taps

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

template <int S>
__global__ __launch_bounds__(512) void conv3x3_strided_kernel(StridedArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, hh = lane >> 5;

  // ---- XCD-aware, bijective workgroup -> tile map: consecutive tiles (N fastest) share an XCD
  const int nwg = p.mtiles * p.ntiles;
  int wg = blockIdx.x;
  {
    const int q = nwg >> 3, r = nwg & 7, xcd = wg & 7, idx = wg >> 3;
    wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  const int mt = wg / p.ntiles, nt = wg - mt * p.ntiles;
  const long m0 = (long)mt * CBM;
  const int n0 = nt * CBN;
  constexpr int taps = 9;
  const int nsteps = taps * (p.Cp / CBK);

  if (wave < 4) {
    // =========================== CONSUMERS ===========================
    const int wm = wave >> 1, wn = wave & 1;
    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = f32x16{0};

    __syncthreads();                                   // buffer 0 written by the producers' prologue
    for (int step = 0; step < nsteps; ++step) {
      const unsigned char* base = lds + (step & 1) * BUF_BYTES;
      const unsigned char* pa = base + (wm * 128 + l31) * ROWB + hh * 16;
      const unsigned char* pb = base + 2 * A_BYTES + (wn * 64 + l31) * ROWB + hh * 16;
      bf16x8 ah[2][4], al[2][4], bh[2][2], bl[2][2];
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          bh[kk][j] = *reinterpret_cast<const bf16x8*>(pb + j * 32 * ROWB + kk * 32);
          bl[kk][j] = *reinterpret_cast<const bf16x8*>(pb + B_BYTES + j * 32 * ROWB + kk * 32);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          ah[kk][i] = *reinterpret_cast<const bf16x8*>(pa + i * 32 * ROWB + kk * 32);
          al[kk][i] = *reinterpret_cast<const bf16x8*>(pa + A_BYTES + i * 32 * ROWB + kk * 32);
        }
      }
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[kk][i], bh[kk][j], acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[kk][i], bl[kk][j], acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[kk][i], bh[kk][j], acc[i][j], 0, 0, 0);
          }
      __syncthreads();
    }

    // ---- epilogue: bias, activation, optional residual, NHWC store
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = n0 + wn * 64 + j * 32 + l31;
      const bool nok = n < p.Cout;
      const float bv = (p.bias != nullptr && nok) ? p.bias[n] : 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const long m = m0 + wm * 128 + i * 32 + acc_row(r, hh);
          if (nok && m < p.M) {
            float v = acc[i][j][r] + bv;
            if (p.act == OCV_ACT_LEAKY_RELU) v = v > 0.f ? v : 0.01f * v;
            else if (p.act == OCV_ACT_SILU) v = fast_silu(v);
            else if (p.act == OCV_ACT_RELU) v = fmaxf(v, 0.f);
            if (p.res != nullptr) v += p.res[m * p.Cout + n];
            p.y[m * p.Cout + n] = v;
          }
        }
    }
    return;
  }

  // =========================== PRODUCERS ===========================
  // Two producer groups alternate over the K steps (conv_igemm_kernel's schedule: issue two intervals ahead, convert,
  // write).  Per row: the byte offset of its window's top-left input pixel and the mask of in-image taps, hoisted out of
  // the K loop; per step one scalar byte offset for (tap, channel chunk).
  const int g = (wave - 4) >> 1;                       // producer group
  const int gt = tid - 256 - 128 * g;                  // 0..127 inside the group
  const int apart = (gt & 3) * 8;                      // A role: 4 lanes per row (8 channels each); rows (gt >> 2) + 32 i
  unsigned rb[8], tapmask[8];
  {
    const long hw = (long)p.Ho * p.Wo;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const long am = m0 + (gt >> 2) + 32 * i;
      const bool valid = am < p.M;
      const long pix = valid ? am : 0;
      const long b = pix / hw, rem = pix - b * hw;
      const int oy = (int)(rem / p.Wo), ox = (int)(rem - (long)oy * p.Wo);
      const int iy0 = oy * S - p.pad_t, ix0 = ox * S - p.pad_l;
      unsigned mask = 0;
#pragma unroll
      for (int t = 0; t < taps; ++t) {
        const int iy = iy0 + t / 3, ix = ix0 + t % 3;
        if (valid && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W) mask |= 1u << t;
      }
      tapmask[i] = mask;
      rb[i] = (unsigned)((((b * p.H + iy0) * p.W + ix0) * p.Cin + apart) * 4);   // mod 2^32; see the header
    }
  }
  // B role: one weight row per lane (32 channels: 64 B of hi, 64 B of lo)
  const int bn = min(n0 + gt, p.Cout - 1);
  const unsigned wrow = (unsigned)((long)bn * p.Cp * 2);
  const unsigned wtap = (unsigned)((long)p.Cout * p.Cp * 2);

  struct Raw { f32x4 a[16]; f32x4 bh[4], bl[4]; };
  struct Cvt { bf16x8 ahi[8], alo[8]; };

  int nx_tap = g % taps, nx_c0 = (g / taps) * CBK;
  auto advance = [&]() {
#pragma unroll
    for (int r = 0; r < 2; ++r)
      if (++nx_tap == taps) { nx_tap = 0; nx_c0 += CBK; }
  };
  auto issue_loads = [&](Raw& st) {
    const int tap = nx_tap, c0 = nx_c0;
    advance();
    const int ky = tap / 3, kx = tap - ky * 3;
    const unsigned soff = (unsigned)(((ky * p.W + kx) * p.Cin + c0) * 4);
    const bool cok0 = c0 + apart + 4 <= p.Cin, cok1 = c0 + apart + 8 <= p.Cin;   // channel tail of a partial chunk
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const bool inb = (tapmask[i] >> tap) & 1u;
      const char* src = (const char*)p.x + (rb[i] + soff);
      st.a[2 * i + 0] = gload16((inb && cok0) ? (const void*)src : (const void*)cs_zero_page);
      st.a[2 * i + 1] = gload16((inb && cok1) ? (const void*)(src + 16) : (const void*)cs_zero_page);
    }
    const unsigned woff = (unsigned)tap * wtap + wrow + (unsigned)c0 * 2;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      st.bh[e] = gload16((const char*)p.whi + woff + 16 * e);
      st.bl[e] = gload16((const char*)p.wlo + woff + 16 * e);
    }
  };
  auto convert = [&](const Raw& st, Cvt& cv) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      __bf16 hi[8], lo[8];
      split4(st.a[2 * i + 0], hi, lo);
      split4(st.a[2 * i + 1], hi + 4, lo + 4);
      cv.ahi[i] = *reinterpret_cast<bf16x8*>(hi);
      cv.alo[i] = *reinterpret_cast<bf16x8*>(lo);
    }
  };
  auto write_lds = [&](int buf, const Raw& st, const Cvt& cv) {
    unsigned char* base = lds + buf * BUF_BYTES;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      unsigned char* ah = base + ((gt >> 2) + 32 * i) * ROWB + apart * 2;
      *reinterpret_cast<bf16x8*>(ah) = cv.ahi[i];
      *reinterpret_cast<bf16x8*>(ah + A_BYTES) = cv.alo[i];
    }
    unsigned char* bh = base + 2 * A_BYTES + gt * ROWB;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      *reinterpret_cast<f32x4*>(bh + 16 * e) = st.bh[e];
      *reinterpret_cast<f32x4*>(bh + B_BYTES + 16 * e) = st.bl[e];
    }
  };

  Raw raw;
  Cvt cvt;
  if (g < nsteps) {
    issue_loads(raw);
    convert(raw, cvt);
    write_lds(g, raw, cvt);
  }
  if (g == 0 && 2 < nsteps) issue_loads(raw);
  __syncthreads();
  for (int t = 0; t < nsteps; ++t) {
    if ((t & 1) == g) {
      if (t + 2 < nsteps) convert(raw, cvt);
      __syncthreads();
    } else {
      if (t + 1 >= 2 && t + 1 < nsteps) write_lds((t + 1) & 1, raw, cvt);
      if (t + 3 < nsteps) issue_loads(raw);
      __syncthreads();
    }
  }
}

}  // namespace

extern "C" int ocv_conv3x3_nhwc_strided_fwd(const float* x, int Cin, const void* w_hi, const void* w_lo, const float* bias,
                                            const float* residual, float* y, int B, int H, int W, int Cout, int stride,
                                            int pad_t, int pad_l, int Ho, int Wo, int act, ocv_stream_t stream) {
  OCV_CHECK_ARG(x && w_hi && w_lo && y, "ocv_conv3x3_nhwc_strided_fwd: null pointer");
  OCV_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && Ho >= 1 && Wo >= 1 && Cout >= 1 && Cin >= 4 && Cin % 4 == 0,
                "ocv_conv3x3_nhwc_strided_fwd: bad sizes (Cin must be a positive multiple of 4)");
  OCV_CHECK_ARG(stride == 1 || stride == 2, "ocv_conv3x3_nhwc_strided_fwd: stride must be 1 or 2 (got %d)", stride);
  OCV_CHECK_ARG(pad_t >= 0 && pad_l >= 0 && pad_t < 3 && pad_l < 3, "ocv_conv3x3_nhwc_strided_fwd: bad padding (%d, %d)", pad_t, pad_l);
  OCV_CHECK_ARG((Ho - 1) * stride - pad_t < H && (Wo - 1) * stride - pad_l < W,
                "ocv_conv3x3_nhwc_strided_fwd: output larger than the padded input allows");
  OCV_CHECK_ARG(act >= 0 && act <= 3, "ocv_conv3x3_nhwc_strided_fwd: unknown activation %d", act);
  OCV_CHECK_ARG(ocv_aligned16(x) && ocv_aligned16(w_hi) && ocv_aligned16(w_lo),
                "ocv_conv3x3_nhwc_strided_fwd: operands must be 16-byte aligned");
  OCV_CHECK_ARG((long)B * H * W * Cin * 4 < (1L << 31) && 9L * Cout * (Cin + 32) * 2 < (1L << 31),
                "ocv_conv3x3_nhwc_strided_fwd: each operand must be smaller than 2 GiB (32-bit byte offsets inside the kernel)");
  StridedArgs a{};
  a.x = x; a.whi = (const __bf16*)w_hi; a.wlo = (const __bf16*)w_lo;
  a.bias = bias; a.res = residual; a.y = y;
  a.Cin = Cin; a.Cp = (Cin + CBK - 1) / CBK * CBK; a.Cout = Cout;
  a.H = H; a.W = W; a.Ho = Ho; a.Wo = Wo; a.stride = stride; a.pad_t = pad_t; a.pad_l = pad_l; a.act = act;
  a.M = (long)B * Ho * Wo;
  a.mtiles = ocv_cdiv(a.M, CBM); a.ntiles = ocv_cdiv(Cout, CBN);
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)conv3x3_strided_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute((const void*)conv3x3_strided_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr = true;
  }
  const dim3 grid((unsigned)(a.mtiles * a.ntiles));
  if (stride == 1)
    hipLaunchKernelGGL(conv3x3_strided_kernel<1>, grid, dim3(512), 2 * BUF_BYTES, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(conv3x3_strided_kernel<2>, grid, dim3(512), 2 * BUF_BYTES, (hipStream_t)stream, a);
  OCV_CHECK_LAUNCH("ocv_conv3x3_nhwc_strided_fwd");
  return 0;
}
