// The token-local tail of a post-norm transformer encoder layer on TWO-TERM fp16 SPLITS (round 3) -- the arithmetic of
// csrc/xattn_h2.hip (x = hi + 2^-11 lo', three v_mfma_f32_32x32x16_f16 per product block into an accumulator pair, 22-bit
// products = the error of an fp32 FMA chain) applied to layer_tail3_kernel of csrc/token_split3.hip:
//   x1 = LayerNorm1(x + ctx Wo^T + bo)
//   x2 = LayerNorm2(x1 + W2 relu(W1 x1 + b1) + b2)          -> out
//   qkv_next = x2 Wqkv'^T + bqkv'                           -> the NEXT layer's packed q | k | v rows (if there is one)
// (nn.TransformerEncoderLayer, eval mode: reference modules/ObjCAViT.py:155-161,169,188 and modules/layers.py:8-9,23.)
// Half the MFMAs of the three-term bf16 form (480 instead of 960 per wavefront and 32 tokens) and two weight-fragment
// parts instead of three: a workgroup streams 1.27 MB of fragments instead of 1.9 MB -- and the launch is bound by exactly
// that stream (twenty phases, each waiting for fragments requested one phase earlier: 60 us per launch whatever the
// number of workgroups).  LDS 51 KB instead of 69.
// fp16's range applies to the tokens, the hidden activations and the weights (packer saturates); OCV_TOKENS=split3 keeps
// the three-term bf16 kernels, OCV_TOKENS=fp32 the exact ones.
// The split, the staging, the resident fragments, their contraction and the tile LayerNorm are csrc/token_tile.hpp.
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include "token_tile.hpp"
#include "../../include/objcavit_hip.h"

namespace {

struct TailArgs {
  const float *ctx, *x;                 // [M][128]
  const _Float16 *wo_p, *w1_p, *w2_p, *wqkv_p;     // wqkv_p: the next layer's packed in_proj (nullable)
  const float *bo, *g1, *be1, *b1, *b2, *g2, *be2, *bqkv;
  float eps;
  const uint8_t* zero_mask;             // rows written as 0 in `out` (last layer of a masked stack), nullable
  float* out;                           // [M][128]
  float* qkv;                           // [M][384] (nullable with wqkv_p)
  int M, FF;
  float* part;                          // G > 1: [row blocks][G][32][128] raw feed-forward partial sums
  unsigned* cnt;                        // G > 1: [row blocks] arrival tickets, zero at launch, zero again afterwards
};

// Three fragment sets rotate (64 registers each): while a phase multiplies from one, the next TWO phases' fragments are
// in flight -- the three-term kernel, with 96-register sets, could hold two and waited 2 - 3 us per phase for fragments
// requested one 0.75 us phase earlier.
//
// G > 1 (round 4, few tokens -- the reference's own batch of 1 - 2 images, 10 - 19 row blocks on 256 CUs): the launch is bound by
// the 20-phase fragment stream of ONE workgroup (~50 us whatever the batch), so the eight feed-forward chunks of a row block go to
// G workgroups (each repeats the output projection and LN1, walks nchunk / G chunks and leaves its raw partial sums write-through),
// and the row block's LAST workgroup to arrive -- an agent-scope ticket, nobody waits (common.hpp) -- adds the partials in the
// fixed order 0 .. G - 1, does LN2 and the next layer's projection: 3 + 4 phases instead of 20.  G = 1 is the kernel of round 3,
// instruction for instruction.
template <int G>
__global__ __launch_bounds__(256, 1) void layer_tail_h2_kernel(TailArgs p) {
  __shared__ __attribute__((aligned(16))) _Float16 xp[2 * PLANE];   // ctx, then x1, then x2 (two planes)
  __shared__ __attribute__((aligned(16))) _Float16 hp[2 * PLANE];   // hidden chunk
  __shared__ float Cs[TM][E128 + 1];                                 // fp32: sums, x1, x2
  __shared__ unsigned last_flag;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, hh = lane >> 5;
  const int blk = G == 1 ? (int)blockIdx.x : (int)blockIdx.x / G, g = G == 1 ? 0 : (int)blockIdx.x % G;
  const int m0 = blk * TM;
  const int col = wave * 32 + l31;
  const int ksteps2 = p.FF >> 4, nchunk_all = p.FF / KC;
  const int c0 = nchunk_all * g / G, nchunk = nchunk_all * (g + 1) / G - c0;        // this workgroup's chunks [c0, c0 + nchunk)
  auto w1_at = [&](int c) { return p.w1_p + ((long)((c0 + c) * 4 + wave) * NS * 2) * 512 + lane * 8; };
  auto w2_at = [&](int c) { return p.w2_p + (((long)wave * ksteps2 + (c0 + c) * (KC / 16)) * 2) * 512 + lane * 8; };

  // ---- x1 = LN1(x + ctx Wo^T + bo)
  WFragH fa, fb, fc;                    // roles rotate: see the feed-forward loop
  load_wh(fa, p.wo_p + ((long)wave * NS * 2) * 512 + lane * 8);
  load_wh(fb, w1_at(0));                // W1 chunk 0 and W2 chunk 0: in flight under the output projection and LN1
  load_wh(fc, w2_at(0));
  stage_rows_h2(xp, p.ctx, m0, p.M, tid);
  __syncthreads();
  {
    f32x16 a1 = {0}, a2 = {0};
    project_s(xp, fa, l31, hh, a1, a2);
    if (nchunk > 1) load_wh(fa, w1_at(1));
    const float bo = p.bo[col];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = acc_row(r, hh), m = m0 + row;
      Cs[row][col] = a1[r] + a2[r] * LO_DOWN + bo + (m < p.M ? p.x[(long)m * E128 + col] : 0.f);
    }
  }
  __syncthreads();
  ln_tile_inplace(Cs, p.g1, p.be1, p.eps, lane, wave);
  __syncthreads();
  tile_to_planes_h2(xp, Cs, tid);                        // every wavefront is past its reads of the ctx planes
  __syncthreads();

  // ---- x2 = LN2(x1 + W2 relu(W1 x1 + b1) + b2).  Chunk c: phase 1 multiplies by W1(c), phase 2 by W2(c).
  // Entering chunk c the sets hold  s1 = W1(c), s2 = W2(c), s3 = W1(c + 1) (requested a whole chunk ago);  after phase 1 the
  // freed set takes W2(c + 1), after phase 2 the next freed one takes W1(c + 2): every fragment is requested two phases ahead.
  f32x16 acc1 = {0}, acc2 = {0};
  auto ffn_chunk = [&](int c, WFragH& s1, WFragH& s2, WFragH& s3) {
    const float b1 = p.b1[(c0 + c) * KC + col];
    f32x16 h1 = {0}, h2 = {0};
    project_s(xp, s1, l31, hh, h1, h2);
    if (c + 1 < nchunk) load_wh(s1, w2_at(c + 1));
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      _Float16 a, b;
      split_h2(fmaxf(h1[r] + h2[r] * LO_DOWN + b1, 0.f), a, b);
      _Float16* d = hp + acc_row(r, hh) * PROW + col;
      d[0] = a;
      d[PLANE] = b;
    }
    __syncthreads();
    project_s(hp, s2, l31, hh, acc1, acc2);
    if (c + 2 < nchunk) load_wh(s2, w1_at(c + 2));
    __syncthreads();
    (void)s3;
  };
  // rotation of (W1(c), W2(c), W1(c + 1)) over (fb, fc, fa): period three chunks
  int c = 0;
  for (; c + 3 <= nchunk; c += 3) {
    ffn_chunk(c, fb, fc, fa);          // frees fb -> W2(c + 1), fc -> W1(c + 2)
    ffn_chunk(c + 1, fa, fb, fc);      // W1(c + 1) in fa, W2(c + 1) in fb, W1(c + 2) in fc
    ffn_chunk(c + 2, fc, fa, fb);      // W1(c + 2) in fc, W2(c + 2) in fa, W1(c + 3) in fb
  }
  if (c < nchunk) {
    ffn_chunk(c, fb, fc, fa);
    if (c + 1 < nchunk) ffn_chunk(c + 1, fa, fb, fc);
  }
  if constexpr (G > 1) {
    // raw partial sums of this workgroup's chunks, write-through; then the ticket
    float* mine = p.part + ((long)(blk * G + g) * TM) * E128 + col;
#pragma unroll
    for (int r = 0; r < 16; ++r) ocv_store_sc1(mine + acc_row(r, hh) * E128, acc1[r] + acc2[r] * LO_DOWN);
    ocv_wait_vm<0>();
    __syncthreads();
    if (tid == 0) {
      const unsigned old = __hip_atomic_fetch_add((ocv_gu32*)(p.cnt + blk), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const bool last = old == (unsigned)(G - 1);
      if (last) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        ocv_wait_vm<0>();
        __hip_atomic_store((ocv_gu32*)(p.cnt + blk), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);       // nobody else touches it any more
      }
      last_flag = last ? 1u : 0u;
    }
    __syncthreads();
    if (last_flag == 0u) return;
    // the row block's last workgroup: partials of all G workgroups, fixed order (its own comes back from memory like the others)
    const float* all = p.part + ((long)blk * G * TM) * E128 + col;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = acc_row(r, hh);
      float v[G];
#pragma unroll
      for (int gg = 0; gg < G; ++gg) v[gg] = all[((long)gg * TM + row) * E128];
      float sacc = v[0];
#pragma unroll
      for (int gg = 1; gg < G; ++gg) sacc += v[gg];
      acc1[r] = sacc;
      acc2[r] = 0.f;
    }
  }
  const bool next = p.wqkv_p != nullptr;
  WFragH& q0 = fa;
  WFragH& q1 = fb;
  WFragH& q2 = fc;
  if (next) {                                                      // the three projection tiles of this wavefront: under LN2
    load_wh(q0, p.wqkv_p + ((long)(wave * 3 + 0) * NS * 2) * 512 + lane * 8);
    load_wh(q1, p.wqkv_p + ((long)(wave * 3 + 1) * NS * 2) * 512 + lane * 8);
    load_wh(q2, p.wqkv_p + ((long)(wave * 3 + 2) * NS * 2) * 512 + lane * 8);
  }
  {
    const float b2 = p.b2[col];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = acc_row(r, hh);
      Cs[row][col] = acc1[r] + acc2[r] * LO_DOWN + b2 + Cs[row][col];   // residual = x1 (each element read and written by one lane)
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
  tile_to_planes_h2(xp, Cs, tid);
  __syncthreads();
  auto qkv_tile = [&](int t, const WFragH& f) {
    const int n = (wave * 3 + t) * 32 + l31;
    const float bn = p.bqkv[n];
    f32x16 a1 = {0}, a2 = {0};
    project_s(xp, f, l31, hh, a1, a2);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + acc_row(r, hh);
      if (m < p.M) p.qkv[(long)m * 3 * E128 + n] = a1[r] + a2[r] * LO_DOWN + bn;
    }
  };
  qkv_tile(0, q0);
  qkv_tile(1, q1);
  qkv_tile(2, q2);
}

}  // namespace

extern "C" int ocv_layer_tail_h2_fwd(const float* ctx, const float* x, const ocv_encoder_layer_params* p_caller,
                                     const void* next_in_proj_h2, const float* next_in_proj_b, float eps,
                                     const uint8_t* zero_row_mask, float* out, float* qkv_next, int M, int E, int FF,
                                     ocv_stream_t stream) {
  return ocv_layer_tail_h2_ws_fwd(ctx, x, p_caller, next_in_proj_h2, next_in_proj_b, eps, zero_row_mask, out, qkv_next, M, E, FF, nullptr, 0,
                                  stream);
}

// Feed-forward chunks per row block over G workgroups: only where the launch leaves most of the chip idle (see the kernel)
extern "C" int ocv_layer_tail_h2_groups(int M, int FF) {
  const int nblk = ocv_cdiv(M, TM), nchunk = FF / KC;
  int G = nblk <= 24 ? 8 : nblk <= 56 ? 4 : 1;          // (2 groups at 75 - 105 row blocks measured neutral: 870 vs 870, 641 vs 640 img/s)
  while (G > 1 && nchunk % G != 0) G >>= 1;
  return G;
}

extern "C" size_t ocv_layer_tail_h2_workspace_bytes(int M, int FF) {
  if (M < 1 || FF < KC) return 0;
  const int G = ocv_layer_tail_h2_groups(M, FF);
  if (G == 1) return 0;
  const size_t nblk = (size_t)ocv_cdiv(M, TM);
  return nblk * G * TM * E128 * sizeof(float) + ((nblk * sizeof(unsigned) + 255) / 256) * 256;
}

// workspace (ocv_layer_tail_h2_workspace_bytes; may be null / 0 = one workgroup per row block): partial sums, then the row blocks'
// arrival tickets, which must be ZERO when the call starts and are zero again when it has finished.
extern "C" int ocv_layer_tail_h2_ws_fwd(const float* ctx, const float* x, const ocv_encoder_layer_params* p_caller,
                                        const void* next_in_proj_h2, const float* next_in_proj_b, float eps,
                                        const uint8_t* zero_row_mask, float* out, float* qkv_next, int M, int E, int FF,
                                        void* workspace, size_t workspace_bytes, ocv_stream_t stream) {
  ocv_encoder_layer_params pv;
  if (ocv_layer_tail_check("ocv_layer_tail_h2_fwd", "h2", ctx, x, p_caller,
                           [](const ocv_encoder_layer_params& v) { return v.out_proj_h2 && v.linear1_h2 && v.linear2_h2; },
                           "needs the packed two-term fp16 weights (ocv_pack_split_h2_fwd)", next_in_proj_h2, next_in_proj_b, zero_row_mask, out,
                           qkv_next, E, FF, &pv) != 0)
    return -1;
  const ocv_encoder_layer_params* p = &pv;
  OCV_CHECK_ARG(M >= 0&& ocv_aligned16(ctx) && ocv_aligned16(x) && ocv_aligned16(out) && ocv_aligned16(qkv_next) &&
                    ocv_aligned16(p->out_proj_h2) && ocv_aligned16(p->linear1_h2) && ocv_aligned16(p->linear2_h2) && ocv_aligned16(next_in_proj_h2),
                "ocv_layer_tail_h2_fwd: bad M / alignment");
  if (M == 0) return 0;
  TailArgs a{ctx, x, (const _Float16*)p->out_proj_h2, (const _Float16*)p->linear1_h2, (const _Float16*)p->linear2_h2,
             (const _Float16*)next_in_proj_h2, p->out_proj_b, p->norm1_w, p->norm1_b, p->linear1_b, p->linear2_b, p->norm2_w,
             p->norm2_b, next_in_proj_b, eps, zero_row_mask, out, qkv_next, M, FF, nullptr, nullptr};
  const int nblk = ocv_cdiv(M, TM);
  const size_t need = ocv_layer_tail_h2_workspace_bytes(M, FF);
  const int G = (workspace != nullptr && need != 0 && workspace_bytes >= need && ocv_aligned16(workspace)) ? ocv_layer_tail_h2_groups(M, FF) : 1;
  if (G > 1) {
    a.part = (float*)workspace;
    a.cnt = (unsigned*)((char*)workspace + (size_t)nblk * G * TM * E128 * sizeof(float));
  }
  switch (G) {
    case 8: hipLaunchKernelGGL(layer_tail_h2_kernel<8>, dim3(nblk * 8), dim3(256), 0, (hipStream_t)stream, a); break;
    case 4: hipLaunchKernelGGL(layer_tail_h2_kernel<4>, dim3(nblk * 4), dim3(256), 0, (hipStream_t)stream, a); break;
    case 2: hipLaunchKernelGGL(layer_tail_h2_kernel<2>, dim3(nblk * 2), dim3(256), 0, (hipStream_t)stream, a); break;
    default: hipLaunchKernelGGL(layer_tail_h2_kernel<1>, dim3(nblk), dim3(256), 0, (hipStream_t)stream, a); break;
  }
  OCV_CHECK_LAUNCH("ocv_layer_tail_h2_fwd");
  return 0;
}
