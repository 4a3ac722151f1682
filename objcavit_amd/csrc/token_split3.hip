// Token-path linear layers on the bf16 matrix cores at fp32 accuracy: THREE-term split operands.
//
//   v = h + m + l,  h = bf16(v), m = bf16(v - h), l = bf16(v - h - m)      (24 significant bits; both subtractions exact)
//   a b ~= ah bh + ah bm + am bh + am bm + ah bl + al bh                     (dropped terms <= 2^-24 of the product)
//
// Six v_mfma_f32_32x32x16_bf16 (192 matrix-pipe cycles per 32 x 32 x 16 block) against eight v_mfma_f32_32x32x2_f32
// (512): the same results to fp32 rounding at 2.7x the matrix rate and ~1/2.7 of the matrix-core energy -- the forward
// runs at the package power cap once batches are pipelined, so joules per image are what is left
// to save.  The two-term split of the convolutions (2^-17 per product) is NOT used here: the token path feeds the
// queries of a near-one-hot bin softmax.
//
// Operands: activation rows are split once per workgroup while they are staged into LDS (three bf16 planes, rows padded
// to 272 bytes: conflict-free ds_read_b128 of 16 rows x one K octet); the static weights are split and packed ONCE on the
// device by ocv_pack_split3_fwd (csrc/token_pack.hip) into MFMA B-operand fragments,
//   Wp[((jt * (K/16) + s) * 3 + part) * 512 + lane * 8 + e] = part of W[32 jt + (lane & 31)][16 s + 8 (lane >> 5) + e],
// so a wavefront's weight load is one contiguous 1 KB run per (channel tile, K step, part), straight from L2 into VGPRs
// (every weight element is used by exactly one wavefront of a workgroup).
//   lin3_kernel<NT, EPI>   out = epi(A W^T + b): 32 rows x (128 NT) columns per workgroup; epi = none | residual + LayerNorm
//   ffn3_kernel            out = LayerNorm(x + W2 relu(W1 x + b1) + b2), hidden units 128 at a time through LDS
//   layer_tail3_kernel     everything of a layer that is local to a token, in one launch (below)
// The splits, the staging, the resident fragments and the LayerNorms are csrc/token_tile.hpp; the few-key cross-attention on the
// same operands is csrc/xattn_split3.hip; the second pass of a split FFN is ffn_finish_kernel of csrc/linear.hip.
// Replace nn.Linear / nn.MultiheadAttention projections / linear1 + linear2 of nn.TransformerEncoderLayer at
// modules/ObjCAViT.py:155-161,169,188 and modules/layers.py:8-9,23 (same lines as the fp32 kernels of csrc/linear.hip).
#include <math.h>
#include <stdlib.h>

#include "token_tile.hpp"
#include "../../include/objcavit_hip.h"

namespace {

enum { L3_NONE = 0, L3_RELU = 1, L3_LEAKY = 2, L3_RES_LN = 3 };

struct L3Args {
  const float* A; int lda;
  const __bf16* Wp;
  const float* bias;
  float* out; int ldo;
  int M, N, K;
  const float* res; int ldres;
  const float *gamma, *beta; float eps;
  const uint8_t* zero_mask;
};

template <int NT, int EPI>
__global__ __launch_bounds__(256) void lin3_kernel(L3Args p) {
  __shared__ __attribute__((aligned(16))) __bf16 planes[3 * PLANE];
  __shared__ float Cs[EPI == L3_RES_LN ? TM : 1][E128 + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, hh = lane >> 5;
  const int m0 = blockIdx.x * TM;
  const int nsteps_all = (p.K + 15) >> 4, ntl = (p.N + 31) >> 5;
  int jt[NT];
  const __bf16* wp[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    jt[t] = (blockIdx.y * 4 + wave) * NT + t;
    wp[t] = p.Wp + ((long)min(jt[t], ntl - 1) * nsteps_all * 3) * 512 + lane * 8;
  }
  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x16{0};
  WFrag3 fa, fb;                                           // ping-pong: tile t multiplies from one while t + 1 loads into the other
  for (int k0 = 0; k0 < p.K; k0 += KC) {
    const int kc = min(KC, p.K - k0), ns = (kc + 15) >> 4;
    load_w3(fa, wp[0] + (long)(k0 >> 4) * 1536, ns);
    __syncthreads();
    stage_rows3(planes, p.A, p.lda, m0, p.M, k0, kc, tid);
    __syncthreads();
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      WFrag3& cur = (t & 1) ? fb : fa;
      WFrag3& nxt = (t & 1) ? fa : fb;
      if (t + 1 < NT) load_w3(nxt, wp[t + 1] + (long)(k0 >> 4) * 1536, ns);
      acc[t] = chunk_mfma3(acc[t], planes, cur, ns, l31, hh);
    }
  }
  if (EPI != L3_RES_LN) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int n = jt[t] * 32 + l31;
      if (n >= p.N) continue;
      const float bn = p.bias != nullptr ? p.bias[n] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + acc_row(r, hh);
        float v = acc[t][r] + bn;
        if (EPI == L3_RELU) v = fmaxf(v, 0.f);
        if (EPI == L3_LEAKY) v = v > 0.f ? v : 0.01f * v;
        if (m < p.M) p.out[(long)m * p.ldo + n] = v;
      }
    }
  } else {
    const int n = wave * 32 + l31;                       // N == 128, NT == 1, gridDim.y == 1
    const float bn = p.bias != nullptr ? p.bias[n] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = acc_row(r, hh), m = m0 + row;
      float v = acc[0][r] + bn;
      if (m < p.M) v += p.res[(long)m * p.ldres + n];
      Cs[row][n] = v;
    }
    __syncthreads();
    ln_rows(Cs, p.gamma, p.beta, p.eps, p.zero_mask, p.out, p.ldo, m0, p.M, lane, wave);
  }
}

struct F3Args {
  const float* x;
  const __bf16 *w1p, *w2p;
  const float *b1, *b2, *gamma, *beta;
  float eps;
  const uint8_t* zero_mask;
  float* out;
  int M, FF;
  float* part;           // nsplit > 1: raw partial outputs [nsplit][M][128]
  int nsplit;
};

__global__ __launch_bounds__(256) void ffn3_kernel(F3Args p) {
  __shared__ __attribute__((aligned(16))) __bf16 xp[3 * PLANE];
  __shared__ __attribute__((aligned(16))) __bf16 hp[3 * PLANE];
  __shared__ float Cs[TM][E128 + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, hh = lane >> 5;
  const int m0 = blockIdx.x * TM;
  const int col = wave * 32 + l31;
  const int nchunk_all = p.FF / KC;
  const int cbeg = nchunk_all * (int)blockIdx.y / p.nsplit, cend = nchunk_all * ((int)blockIdx.y + 1) / p.nsplit;
  const int ksteps2 = p.FF >> 4;                         // K steps of W2 (K = FF)
  auto w1_at = [&](int c) { return p.w1p + ((long)(c * 4 + wave) * (E128 / 16) * 3) * 512 + lane * 8; };
  auto w2_at = [&](int c) { return p.w2p + (((long)wave * ksteps2 + c * (KC / 16)) * 3) * 512 + lane * 8; };

  stage_rows3(xp, p.x, E128, m0, p.M, 0, E128, tid);
  f32x16 acc = {0};
  WFrag3 f1, f2;
  load_w3(f1, w1_at(cbeg), E128 / 16);
  __syncthreads();
  for (int c = cbeg; c < cend; ++c) {
    load_w3(f2, w2_at(c), KC / 16);                      // this chunk's W2 fragments: in flight during phase 1
    // phase 1: hidden units [128 c + 32 wave, + 32) of the tile's rows
    f32x16 h = {0};
    h = chunk_mfma3(h, xp, f1, E128 / 16, l31, hh);
    const float b1 = p.b1[c * KC + col];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      __bf16* d = hp + acc_row(r, hh) * PROW + col;
      split1x3(fmaxf(h[r] + b1, 0.f), d[0], d[PLANE], d[2 * PLANE]);
    }
    if (c + 1 < cend) load_w3(f1, w1_at(c + 1), E128 / 16);      // the next chunk's W1 fragments: in flight during phase 2
    __syncthreads();
    // phase 2: out[:, 32 wave ..] += H_chunk . W2[:, 128 c ..]^T
    acc = chunk_mfma3(acc, hp, f2, KC / 16, l31, hh);
    __syncthreads();
  }
  if (p.nsplit > 1) {
    float* dst = p.part + ((long)blockIdx.y * p.M + m0) * E128 + col;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = acc_row(r, hh);
      if (m0 + row < p.M) dst[(long)row * E128] = acc[r];
    }
    return;
  }
  const float b2 = p.b2[col];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = acc_row(r, hh), m = m0 + row;
    Cs[row][col] = acc[r] + b2 + (m < p.M ? p.x[(long)m * E128 + col] : 0.f);
  }
  __syncthreads();
  ln_rows(Cs, p.gamma, p.beta, p.eps, p.zero_mask, p.out, E128, m0, p.M, lane, wave);
}

// ---------------------------------------------------------------------------
// Everything of a post-norm transformer layer that is LOCAL to a token, in one launch per 32-token tile:
//   x1 = LayerNorm1(x + ctx Wo^T + bo)            (ctx = the attention kernel's output for these tokens)
//   x2 = LayerNorm2(x1 + W2 relu(W1 x1 + b1) + b2)          -> out
//   qkv_next = x2 Wqkv'^T + bqkv'                           -> the NEXT layer's packed q | k | v rows (if there is one)
// so a layer is two launches -- attention, this -- instead of four, and the next layer's projection rides along.  The
// four separate launches cost 13 - 17 us each for ~5 us of arithmetic (a cold start per launch: row staging, first
// weight fragments, tail), 112 us per layer.  x1 and x2 never leave the workgroup between the phases (fp32 copy in LDS
// for the residuals, three-term planes for the next contraction).  Same arithmetic, same order as lin3 + ffn3 + lin3.
// ---------------------------------------------------------------------------
struct TailArgs {
  const float *ctx, *x;                 // [M][128]
  const __bf16 *wo_p, *w1_p, *w2_p, *wqkv_p;     // wqkv_p: the next layer's packed in_proj (nullable)
  const float *bo, *g1, *be1, *b1, *b2, *g2, *be2, *bqkv;
  float eps;
  const uint8_t* zero_mask;             // rows written as 0 in `out` (last layer of a masked stack), nullable
  float* out;                           // [M][128]
  float* qkv;                           // [M][384] (nullable with wqkv_p)
  int M, FF;
};

// One 32-token tile per workgroup.  Two row tiles per workgroup (every streamed fragment serving two MFMA tiles) were measured
// SLOWER, 92 us against 60 us per launch: the launch is bound by the chain of phases, each waiting for its fragments, not by L2.
// The record is profiles/r06_tail_forms.txt and tools/diag/layer_tail_row_tiles.patch.txt.
__global__ __launch_bounds__(256) void layer_tail3_kernel(TailArgs p) {
  __shared__ __attribute__((aligned(16))) __bf16 xp[3 * PLANE];      // ctx, then x1, then x2
  __shared__ __attribute__((aligned(16))) __bf16 hp[3 * PLANE];      // hidden chunk
  __shared__ float Cs[TM][E128 + 1];                                  // fp32: sums, x1, x2
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, hh = lane >> 5;
  const int m0 = blockIdx.x * TM;
  const int col = wave * 32 + l31;
  const int ksteps2 = p.FF >> 4, nchunk = p.FF / KC;
  auto w1_at = [&](int c) { return p.w1_p + ((long)(c * 4 + wave) * (E128 / 16) * 3) * 512 + lane * 8; };
  auto w2_at = [&](int c) { return p.w2_p + (((long)wave * ksteps2 + c * (KC / 16)) * 3) * 512 + lane * 8; };

  // ---- x1 = LN1(x + ctx Wo^T + bo)
  WFrag3 f1, f2;
  load_w3(f1, p.wo_p + ((long)wave * (E128 / 16) * 3) * 512 + lane * 8, E128 / 16);
  stage_rows3(xp, p.ctx, E128, m0, p.M, 0, E128, tid);
  __syncthreads();
  {
    const f32x16 a = chunk_mfma3(f32x16{0}, xp, f1, E128 / 16, l31, hh);
    load_w3(f1, w1_at(0), E128 / 16);                  // W1, first chunk: under LN1
    const float bo = p.bo[col];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = acc_row(r, hh), m = m0 + row;
      Cs[row][col] = a[r] + bo + (m < p.M ? p.x[(long)m * E128 + col] : 0.f);
    }
  }
  __syncthreads();
  ln_tile_inplace(Cs, p.g1, p.be1, p.eps, lane, wave);
  __syncthreads();
  tile_to_planes3(xp, Cs, tid);                       // every wavefront is past its reads of the ctx planes
  __syncthreads();

  // ---- x2 = LN2(x1 + W2 relu(W1 x1 + b1) + b2)
  f32x16 acc = {0};
  // (ffn3_kernel's chunk body; as one device function for both, ffn3_kernel gained or lost an s_waitcnt whichever way its arguments went)
  for (int c = 0; c < nchunk; ++c) {
    load_w3(f2, w2_at(c), KC / 16);
    const float b1 = p.b1[c * KC + col];
    const f32x16 h = chunk_mfma3(f32x16{0}, xp, f1, E128 / 16, l31, hh);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      __bf16* d = hp + acc_row(r, hh) * PROW + col;
      split1x3(fmaxf(h[r] + b1, 0.f), d[0], d[PLANE], d[2 * PLANE]);
    }
    if (c + 1 < nchunk) load_w3(f1, w1_at(c + 1), E128 / 16);
    __syncthreads();
    acc = chunk_mfma3(acc, hp, f2, KC / 16, l31, hh);
    __syncthreads();
  }
  const bool next = p.wqkv_p != nullptr;
  if (next) load_w3(f1, p.wqkv_p + ((long)(wave * 3) * (E128 / 16) * 3) * 512 + lane * 8, E128 / 16);     // under LN2
  {
    const float b2 = p.b2[col];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = acc_row(r, hh);
      Cs[row][col] = acc[r] + b2 + Cs[row][col];       // residual = x1 (each element read and written by one lane)
    }
  }
  __syncthreads();
  ln_tile_inplace(Cs, p.g2, p.be2, p.eps, lane, wave);
  __syncthreads();
  for (int i = tid; i < TM * (E128 / 4); i += 256) {     // x2 -> out, 16-byte stores
    const int row = i / (E128 / 4), c4 = (i % (E128 / 4)) * 4, m = m0 + row;
    if (m < p.M) {
      const bool z = p.zero_mask != nullptr && p.zero_mask[m] != 0;
      const float4 v = z ? make_float4(0.f, 0.f, 0.f, 0.f) : make_float4(Cs[row][c4], Cs[row][c4 + 1], Cs[row][c4 + 2], Cs[row][c4 + 3]);
      *reinterpret_cast<float4*>(p.out + (long)m * E128 + c4) = v;
    }
  }
  if (!next) return;

  // ---- the next layer's packed projection: wavefront w -> channel tiles 3 w .. 3 w + 2 of the 12
  tile_to_planes3(xp, Cs, tid);
  __syncthreads();
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    WFrag3& cur = (t & 1) ? f2 : f1;
    WFrag3& nxt = (t & 1) ? f1 : f2;
    if (t + 1 < 3) load_w3(nxt, p.wqkv_p + ((long)(wave * 3 + t + 1) * (E128 / 16) * 3) * 512 + lane * 8, E128 / 16);
    const int n = (wave * 3 + t) * 32 + l31;
    const float bn = p.bqkv[n];
    const f32x16 q = chunk_mfma3(f32x16{0}, xp, cur, E128 / 16, l31, hh);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + acc_row(r, hh);
      if (m < p.M) p.qkv[(long)m * 3 * E128 + n] = q[r] + bn;
    }
  }
}

template <int NT>
int launch_lin3(const L3Args& a, int act, hipStream_t st) {
  dim3 grid(ocv_cdiv(a.M, TM), ocv_cdiv(a.N, 128 * NT)), block(256);
  switch (act) {
    case OCV_ACT_RELU: hipLaunchKernelGGL((lin3_kernel<NT, L3_RELU>), grid, block, 0, st, a); break;
    case OCV_ACT_LEAKY_RELU: hipLaunchKernelGGL((lin3_kernel<NT, L3_LEAKY>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL((lin3_kernel<NT, L3_NONE>), grid, block, 0, st, a); break;
  }
  OCV_CHECK_LAUNCH("ocv_linear_split3_fwd");
  return 0;
}

}  // namespace

extern "C" int ocv_linear_split3_fwd(const float* A, int lda, const void* w_packed, const float* bias, float* out, int ldo,
                                     int M, int N, int K, int act, ocv_stream_t stream) {
  OCV_CHECK_ARG(A && w_packed && out, "ocv_linear_split3_fwd: null pointer");
  OCV_CHECK_ARG(M >= 0 && N >= 1 && K >= 8 && K % 8 == 0 && lda >= K && ldo >= N && lda % 4 == 0,
                "ocv_linear_split3_fwd: bad sizes (K and lda must be multiples of 8 / 4; M=%d N=%d K=%d)", M, N, K);
  OCV_CHECK_ARG(act >= 0 && act <= 2, "ocv_linear_split3_fwd: unknown activation %d", act);
  OCV_CHECK_ARG(ocv_aligned16(A) && ocv_aligned16(w_packed), "ocv_linear_split3_fwd: A / w_packed must be 16-byte aligned");
  if (M == 0) return 0;
  L3Args a{A, lda, (const __bf16*)w_packed, bias, out, ldo, M, N, K, nullptr, 0, nullptr, nullptr, 0.f, nullptr};
  hipStream_t st = (hipStream_t)stream;
  const int ntl = (N + 31) / 32;
  if (ntl % 12 == 0 || ntl > 8) return launch_lin3<3>(a, act, st);       // 384 columns per workgroup (packed QKV)
  if (ntl > 4) return launch_lin3<2>(a, act, st);
  return launch_lin3<1>(a, act, st);
}

extern "C" int ocv_linear_residual_layernorm_split3_fwd(const float* A, int lda, const void* w_packed, const float* bias,
                                                        const float* residual, int ldres, const float* gamma,
                                                        const float* beta, float eps, const uint8_t* zero_row_mask,
                                                        float* out, int ldo, int M, int N, int K, ocv_stream_t stream) {
  OCV_CHECK_ARG(A && w_packed && residual && gamma && beta && out, "ocv_linear_residual_layernorm_split3_fwd: null pointer");
  OCV_CHECK_ARG(N == E128, "ocv_linear_residual_layernorm_split3_fwd: N must be %d (got %d)", E128, N);
  OCV_CHECK_ARG(M >= 0 && K >= 8 && K % 8 == 0 && lda >= K && lda % 4 == 0 && ldo >= N && ldres >= N,
                "ocv_linear_residual_layernorm_split3_fwd: bad sizes");
  OCV_CHECK_ARG(ocv_aligned16(A) && ocv_aligned16(w_packed), "ocv_linear_residual_layernorm_split3_fwd: A / w_packed must be 16-byte aligned");
  if (M == 0) return 0;
  L3Args a{A, lda, (const __bf16*)w_packed, bias, out, ldo, M, N, K, residual, ldres, gamma, beta, eps, zero_row_mask};
  hipLaunchKernelGGL((lin3_kernel<1, L3_RES_LN>), dim3(ocv_cdiv(M, TM), 1), dim3(256), 0, (hipStream_t)stream, a);
  OCV_CHECK_LAUNCH("ocv_linear_residual_layernorm_split3_fwd");
  return 0;
}

extern "C" int ocv_layer_tail_split3_fwd(const float* ctx, const float* x, const ocv_encoder_layer_params* p_caller,
                                         const void* next_in_proj_p3, const float* next_in_proj_b, float eps,
                                         const uint8_t* zero_row_mask, float* out, float* qkv_next, int M, int E, int FF,
                                         ocv_stream_t stream) {
  ocv_encoder_layer_params pv;
  if (ocv_layer_tail_check("ocv_layer_tail_split3_fwd", "p3", ctx, x, p_caller,
                           [](const ocv_encoder_layer_params& v) { return v.out_proj_p3 && v.linear1_p3 && v.linear2_p3; },
                           "needs the packed split3 weights", next_in_proj_p3, next_in_proj_b, zero_row_mask, out, qkv_next, E, FF, &pv) != 0)
    return -1;
  const ocv_encoder_layer_params* p = &pv;
  OCV_CHECK_ARG(M >= 0 && ocv_aligned16(ctx) && ocv_aligned16(x) && ocv_aligned16(out) && ocv_aligned16(qkv_next),
                "ocv_layer_tail_split3_fwd: bad M / alignment");
  if (M == 0) return 0;
  TailArgs a{ctx, x, (const __bf16*)p->out_proj_p3, (const __bf16*)p->linear1_p3, (const __bf16*)p->linear2_p3,
             (const __bf16*)next_in_proj_p3, p->out_proj_b, p->norm1_w, p->norm1_b, p->linear1_b, p->linear2_b, p->norm2_w,
             p->norm2_b, next_in_proj_b, eps, zero_row_mask, out, qkv_next, M, FF};
  hipLaunchKernelGGL(layer_tail3_kernel, dim3(ocv_cdiv(M, TM)), dim3(256), 0, (hipStream_t)stream, a);
  OCV_CHECK_LAUNCH("ocv_layer_tail_split3_fwd");
  return 0;
}

extern "C" size_t ocv_ffn_split3_workspace_bytes(int M, int FF) {
  if (M < 1 || FF < KC || FF % KC != 0) return 0;
  return (size_t)ocv_ffn_split_count(M, FF) * M * E128 * sizeof(float);
}

extern "C" int ocv_ffn_residual_layernorm_split3_fwd(const float* x, const void* w1_packed, const float* b1,
                                                     const void* w2_packed, const float* b2, const float* gamma,
                                                     const float* beta, float eps, const uint8_t* zero_row_mask, float* out,
                                                     int M, int E, int FF, void* workspace, size_t workspace_bytes,
                                                     ocv_stream_t stream) {
  OCV_CHECK_ARG(x && w1_packed && b1 && w2_packed && b2 && gamma && beta && out, "ocv_ffn_residual_layernorm_split3_fwd: null pointer");
  OCV_CHECK_ARG(E == E128 && FF >= KC && FF % KC == 0, "ocv_ffn_residual_layernorm_split3_fwd: needs E = %d and FF a multiple of %d (got %d, %d)", E128, KC, E, FF);
  OCV_CHECK_ARG(M >= 0 && ocv_aligned16(x) && ocv_aligned16(w1_packed) && ocv_aligned16(w2_packed), "ocv_ffn_residual_layernorm_split3_fwd: bad M / alignment");
  if (M == 0) return 0;
  int ns = ocv_ffn_split_count(M, FF);
  if (ns > 1 && (workspace == nullptr || workspace_bytes < (size_t)ns * M * E128 * sizeof(float))) ns = 1;
  F3Args a{x, (const __bf16*)w1_packed, (const __bf16*)w2_packed, b1, b2, gamma, beta, eps, zero_row_mask, out, M, FF,
           (float*)workspace, ns};
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ffn3_kernel, dim3(ocv_cdiv(M, TM), ns), dim3(256), 0, st, a);
  OCV_CHECK_LAUNCH("ocv_ffn_residual_layernorm_split3_fwd");
  if (ns > 1) return ocv_ffn_finish_launch("ocv_ffn_residual_layernorm_split3_fwd(finish)", x, b2, gamma, beta, eps, zero_row_mask, out, M, (const float*)workspace, ns, st);
  return 0;
}
