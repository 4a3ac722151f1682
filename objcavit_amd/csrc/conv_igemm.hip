// Implicit-GEMM convolution (k = 1 or 3, stride 1 or 2, zero padding) on
// NHWC fp32 activations for gfx950, computed on the bf16 matrix cores with
// SPLIT-bf16 operands and fp32 accumulation:
//
//     a = a_hi + a_lo,  b = b_hi + b_lo   (each part bf16, a_lo = bf16(a - a_hi))
//     a * b  ~=  a_hi b_hi + a_hi b_lo + a_lo b_hi            (3 MFMAs, fp32 accumulate)
//
// hi + lo carries 16 significant bits, the dropped a_lo b_lo term is 2^-18
// relative, so a product is good to ~1e-5 relative and a K-long sum to ~1e-6 of
// its magnitude -- two orders inside the 1e-3 depth tolerance of the path and
// measured end to end in the parity tests -- while the three
// v_mfma_f32_32x32x16_bf16 issues cost 96 cycles per 32x32x16 block against
// 512 cycles for the eight exact v_mfma_f32_32x32x2_f32 issues: 5.3x the fp32
// matrix rate (gfx950 has no xf32/TF32 path).  This is row N1 of SURVEY.md section 8:
// the UNet decoder's 3x3 convolutions are 83 % of the forward's FLOPs
// (modules/DenseFeatureExtractor.py:37-42,97,104-116) and MIOpen's fp32
// implicit GEMM already sits at 85 % of the fp32 matrix peak there.
//
// GEMM view: M = B*Ho*Wo output pixels, N = Cout, K = taps x Cin.  Output
// pixel (b, oy, ox) reads input pixel (b, S oy - pad_t + ky, S ox - pad_l + kx)
// at tap (ky, kx), zero outside the image: stride 1 with pad = k / 2 and
// Ho, Wo = H, W is the decoder's "same" convolution (ocv_conv_nhwc_fwd); stride
// 1 or 2 with explicit top / left padding and output size is EfficientNetV2's
// Fused-MBConv 3x3 (ocv_conv3x3_nhwc_strided_fwd).  The A operand is gathered
// on the fly from one or two NHWC tensors -- a second tensor acts as a virtual
// channel concat, which is how UpSampleWithSkip feeds [upsampled, skip] without
// materialising the cat -- and split into hi/lo in registers on its way to LDS.
// Weights are split once on the host into two bf16 arrays laid out
// [tap][Cout][Cin rounded up to 32].
//
// Tile: 256 pixels x 128 channels per workgroup; K advances 32 channels of one tap per step (channel chunk outer,
// tap inner: the nine taps of a chunk re-read the same L2-resident lines) through a double-buffered LDS image
// (A_hi, A_lo, B_hi, B_lo; rows padded to 80 bytes so the 16-byte fragment reads of 16 consecutive rows land in
// 16 different bank slots).
//
// The 8 wavefronts are SPECIALISED (first version: every wavefront did everything; PMC: 8.5 VALU instructions per
// MFMA, matrix pipe 32 % busy -- the address / bounds / fp32->hi,lo conversion work of a step ran in lock-step on
// all waves between two barriers and could not overlap the MFMAs):
//   waves 0-3  CONSUMERS: 2 x 2 over the tile, 128 x 64 outputs each (8 accumulators); per step 24 ds_read_b128 and
//              48 MFMAs, nothing else.
//   waves 4-7  PRODUCERS: gather the next A chunk (4 rows x 32 B per lane, out-of-image taps read a zero page, no
//              selects), split it into hi/lo, fetch the pre-split weight chunk, write the other LDS buffer.
// One consumer and one producer wave share each SIMD: matrix pipe and VALU run side by side; one barrier per step.
// Workgroup ids are remapped so that the N-tiles of one pixel tile run on the same XCD and share its L2.
// Kernel size, stride and the second source are template parameters (conv_igemm_kernel<KS, S, CAT>): the tap loop, the
// tap -> (ky, kx) split and the source select are resolved at compile time.
//
// This file: the fp32-input kernel and its two entry points.  The family's shared pieces are in conv_tile.hpp, the kernels
// on a pre-split input in conv_dma.hip, Winograd F(4x4, 3x3) in conv_winograd.hip.
#include "conv_tile.hpp"

namespace {

constexpr int ROWB = 80;                                  // bytes per LDS row (64 data + 16 pad)
constexpr int A_BYTES = CBM * ROWB, B_BYTES = CBN * ROWB;
constexpr int BUF_BYTES = 2 * A_BYTES + 2 * B_BYTES;      // 61440

// KS: kernel size (1 or 3); S: stride (1 or 2); CAT: x2 is concatenated after x1's channels
template <int KS, int S, bool CAT>
__global__ __launch_bounds__(512) void conv_igemm_kernel(ConvArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, hh = lane >> 5;

  // ---- XCD-aware, bijective workgroup -> tile map: consecutive tiles (N fastest) share an XCD
  const int wg = ocv_xcd_remap(blockIdx.x, p.mtiles * p.ntiles);
  const int mt = wg / p.ntiles, nt = wg - mt * p.ntiles;
  const long m0 = (long)mt * CBM;
  const int n0 = nt * CBN;
  constexpr int taps = KS * KS;
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
      // all 24 fragment reads of the step are issued up front: the second k-slice's reads return while the first
      // slice's 24 MFMAs run (the only matrix-pipe wave of this SIMD would otherwise sit through their latency)
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

    // ---- epilogue: bias, activation, optional residual, NHWC store (128-byte runs per half-wave)
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
            float v = conv_act(acc[i][j][r] + bv, p.act);
            if (p.res != nullptr) v += p.res[m * p.Cout + n];
            p.y[m * p.Cout + n] = v;
          }
        }
    }
    return;
  }

  // =========================== PRODUCERS ===========================
  // Two producer groups (waves 4-5 and 6-7) ALTERNATE: group g owns the K steps t = g, g+2, g+4, ...  A step's data
  // may only be written to LDS during the interval before it is consumed (its buffer is being read in the one before
  // that), so with a single group the global-load latency sat on the critical path of every step (1.8 us per step
  // against 0.8 us of MFMAs).  Each group now has TWO intervals per step it owns:
  //     interval t-1 (after writing step t):  issue the loads of step t+2          (>= one interval to land)
  //     interval t   ("convert" interval)   :  wait, split fp32 -> bf16 hi/lo into registers
  //     interval t+1 ("write" interval)     :  ds_write step t+2, then issue step t+4 ...
  // while the other group does the same shifted by one interval.  Every wave has at most one stage of loads in
  // flight and all loads are ordinary, compiler-visible loads (see gload16): exact s_waitcnt, no stale registers.
  //
  // All per-lane address work is hoisted out of the K loop (s_memtime stamps showed 2200 of 3600 producer cycles per
  // step in 64-bit index arithmetic, divisions and bounds tests): per row the byte offsets of its window's top-left
  // input pixel in both source tensors and a 9-bit mask of in-image taps; per step one scalar, non-negative byte offset
  // for (tap, channel chunk); tap / chunk counters advance incrementally.  The row offsets are 32-bit and may wrap below
  // zero when the corner lies in the padding: they are only ever added to the offset of an in-image tap, and that sum
  // lies inside the operand (< 4 GiB, checked on the host).
  const int g = (wave - 4) >> 1;                       // producer group
  const int gt = tid - 256 - 128 * g;                  // 0..127 inside the group
  // A role: 4 lanes per row (32 B = 8 channels each); rows (gt >> 2) + 32 i, i = 0..7
  const int apart = (gt & 3) * 8;
  unsigned rb1[8], rb2[8], tapmask[8];                  // rb2: only with CAT
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
        const int iy = iy0 + t / KS, ix = ix0 + t % KS;
        if (valid && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W) mask |= 1u << t;
      }
      tapmask[i] = mask;
      const long corner = (b * p.H + iy0) * p.W + ix0;
      rb1[i] = (unsigned)((corner * p.C1 + apart) * 4);
      if (CAT) rb2[i] = (unsigned)((corner * p.C2 + apart) * 4);
    }
  }
  // B role: one weight row per lane (32 channels: 64 B of hi, 64 B of lo)
  const int bn = min(n0 + gt, p.Cout - 1);
  const unsigned wrow = (unsigned)((long)bn * p.Cp * 2);                 // byte offset inside one tap's [Cout][Cp] slab
  const unsigned wtap = (unsigned)((long)p.Cout * p.Cp * 2);             // bytes per tap slab

  struct Raw { f32x4 a[16]; f32x4 bh[4], bl[4]; };                       // one step as loaded
  struct Cvt { bf16x8 ahi[8], alo[8]; };                                 // its A part, split

  int nx_tap = g % taps, nx_c0 = (g / taps) * CBK;                       // (tap, chunk) of this group's next step
  auto advance = [&]() {                                                 // += 2 steps
#pragma unroll
    for (int r = 0; r < 2; ++r)
      if (++nx_tap == taps) { nx_tap = 0; nx_c0 += CBK; }
  };
  auto issue_loads = [&](Raw& st) {
    const int tap = nx_tap, c0 = nx_c0;
    advance();
    const int ky = tap / KS, kx = tap - ky * KS;
    const bool first = !CAT || c0 < p.C1;
    const char* tbase = (const char*)(first ? p.x1 : p.x2);
    const int tc = first ? p.C1 : p.C2;
    const int cin = first ? c0 : c0 - p.C1;                              // chunk start inside the source tensor
    const unsigned soff = (unsigned)(((ky * p.W + kx) * tc + cin) * 4);  // scalar byte offset of (tap, chunk)
    const bool cok0 = cin + apart + 4 <= tc, cok1 = cin + apart + 8 <= tc;   // channel tail of a partial chunk
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const bool inb = (tapmask[i] >> tap) & 1u;
      const char* src = tbase + ((first ? rb1[i] : rb2[i]) + soff);
      st.a[2 * i + 0] = gload16((inb && cok0) ? (const void*)src : (const void*)ocv_zero_page);
      st.a[2 * i + 1] = gload16((inb && cok1) ? (const void*)(src + 16) : (const void*)ocv_zero_page);
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
  // prologue: group g fills buffer g with step g (nobody reads yet); group 0 also starts the loads of step 2
  if (g < nsteps) {
    issue_loads(raw);
    convert(raw, cvt);
    write_lds(g, raw, cvt);
  }
  if (g == 0 && 2 < nsteps) issue_loads(raw);
  __syncthreads();
  for (int t = 0; t < nsteps; ++t) {                   // interval t: the consumers multiply buffer t & 1
    if ((t & 1) == g) {
      // convert interval: the loads of step t+2 (issued one interval ago) land and are split; B stays as loaded
      if (t + 2 < nsteps) convert(raw, cvt);
      __syncthreads();
    } else {
      // write interval: step t+1 goes to buffer (t+1) & 1 (free since the last barrier), then fetch step t+3
      if (t + 1 >= 2 && t + 1 < nsteps) write_lds((t + 1) & 1, raw, cvt);
      if (t + 3 < nsteps) issue_loads(raw);
      __syncthreads();
    }
  }
}

// conv_igemm_kernel (fp32 input) over the output grid B x Ho x Wo
template <int KS, int S, bool CAT>
int launch_igemm(ConvArgs& a, int B, hipStream_t st, const char* name) {
  a.Cp = (a.Cin + CBK - 1) / CBK * CBK;
  a.M = (long)B * a.Ho * a.Wo;
  a.mtiles = ocv_cdiv(a.M, CBM); a.ntiles = ocv_cdiv(a.Cout, CBN);
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)conv_igemm_kernel<KS, S, CAT>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr = true;
  }
  hipLaunchKernelGGL((conv_igemm_kernel<KS, S, CAT>), dim3(a.mtiles * a.ntiles), dim3(512), 2 * BUF_BYTES, st, a);
  OCV_CHECK_LAUNCH(name);
  return 0;
}
}  // namespace

extern "C" int ocv_conv_nhwc_fwd(const float* x1, int C1, const float* x2, int C2, const void* w_hi, const void* w_lo,
                                 const float* bias, const float* residual, float* y, int B, int H, int W, int Cout,
                                 int ksize, int act, ocv_stream_t stream) {
  OCV_CHECK_ARG(x1 && w_hi && w_lo && y, "ocv_conv_nhwc_fwd: null pointer");
  OCV_CHECK_ARG(ksize == 1 || ksize == 3, "ocv_conv_nhwc_fwd: kernel size must be 1 or 3 (got %d)", ksize);
  OCV_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && Cout >= 1 && C1 >= 4, "ocv_conv_nhwc_fwd: bad sizes");
  OCV_CHECK_ARG(C1 % 4 == 0 && (x2 == nullptr || (C2 >= 4 && C2 % 4 == 0 && C1 % CBK == 0)),
                "ocv_conv_nhwc_fwd: channel counts must be multiples of 4 (and C1 a multiple of %d when a second tensor is concatenated)", CBK);
  OCV_CHECK_ARG(act >= 0 && act <= 3, "ocv_conv_nhwc_fwd: unknown activation %d", act);
  OCV_CHECK_ARG(ocv_aligned16(x1) && ocv_aligned16(x2) && ocv_aligned16(w_hi) && ocv_aligned16(w_lo),
                "ocv_conv_nhwc_fwd: operands must be 16-byte aligned");
  OCV_CHECK_ARG((long)B * H * W * C1 * 4 < (1L << 32) && (long)B * H * W * (x2 ? C2 : 0) * 4 < (1L << 32) &&
                    9L * Cout * (C1 + C2 + 32) * 2 < (1L << 32),
                "ocv_conv_nhwc_fwd: each operand must be smaller than 4 GiB (32-bit byte offsets inside the kernel)");
  ConvArgs a{};
  a.x1 = x1; a.x2 = x2; a.whi = (const __bf16*)w_hi; a.wlo = (const __bf16*)w_lo;
  a.bias = bias; a.res = residual; a.y = y;
  a.C1 = C1; a.C2 = x2 ? C2 : 0; a.Cin = a.C1 + a.C2;
  a.Cout = Cout; a.H = H; a.W = W; a.act = act;
  a.Ho = H; a.Wo = W; a.pad_t = a.pad_l = ksize / 2;                  // stride 1, "same"
  const hipStream_t st = (hipStream_t)stream;
  if (ksize == 1) return x2 ? launch_igemm<1, 1, true>(a, B, st, "ocv_conv_nhwc") : launch_igemm<1, 1, false>(a, B, st, "ocv_conv_nhwc");
  return x2 ? launch_igemm<3, 1, true>(a, B, st, "ocv_conv_nhwc") : launch_igemm<3, 1, false>(a, B, st, "ocv_conv_nhwc");
}

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
  ConvArgs a{};
  a.x1 = x; a.whi = (const __bf16*)w_hi; a.wlo = (const __bf16*)w_lo;
  a.bias = bias; a.res = residual; a.y = y;
  a.C1 = Cin; a.Cin = Cin; a.Cout = Cout;
  a.H = H; a.W = W; a.Ho = Ho; a.Wo = Wo; a.pad_t = pad_t; a.pad_l = pad_l; a.act = act;
  const hipStream_t st = (hipStream_t)stream;
  if (stride == 1) return launch_igemm<3, 1, false>(a, B, st, "ocv_conv3x3_nhwc_strided_fwd");
  return launch_igemm<3, 2, false>(a, B, st, "ocv_conv3x3_nhwc_strided_fwd");
}
