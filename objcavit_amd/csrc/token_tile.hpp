// Shared device pieces of the token path (csrc/token_h2.hip, token_split3.hip, xattn_h2.hip, xattn_split3.hip, token_pack.hip;
// linear.hip takes ln_rows, attention.hip the two-term split and its product step, bin_head.hip the typedef and constants): ONE
// definition of each split, of the staging of a 32-row tile as split planes, of the resident weight fragments and the straight
// and transposed contraction over them, and of the tile LayerNorm.  Helpers and constants only, no kernels.  Two plain sections --
// two-term fp16 ("h2") and three-term bf16 ("split3") -- and what both share.
//
// A helper is used at a call site only where the kernel's instruction stream stays what it was written out: check with
// tools/kernel_table.py.  profiles/token_tile_refactor.txt has the table, the forms that were tried and the sites that therefore
// stay written out (each says so in a comment).
#pragma once
#include "common.hpp"
#include "../../include/objcavit_hip.h"

// ---------------------------------------------------------------------------
// geometry: a workgroup of 256 threads owns TM = 32 rows of E128 = 128 columns; contractions are 128 long (NS steps of 16)
// ---------------------------------------------------------------------------
constexpr int TM = 32;               // rows (tokens, queries) per tile
constexpr int E128 = 128;
constexpr int KC = 128;              // K chunk staged at a time / hidden units per feed-forward chunk
constexpr int NS = E128 / 16;        // K steps of a 128-long contraction
// 2-byte elements per plane row: 256 + 16 = 272 bytes.  An MFMA operand read is a ds_read_b128 of 32 rows x one K octet per
// lane-half; at a pitch of 272 bytes = 68 banks consecutive rows start 4 banks apart, so the eight rows of a 128-byte LDS
// beat cover 32 distinct banks: conflict-free, as are the 16-byte plane stores of the staging (row tid / 8, octet tid % 8).
constexpr int PROW = KC + 8;
constexpr int PLANE = TM * PROW;     // elements per plane

// ---------------------------------------------------------------------------
// h2: x = hi + 2^-11 lo', hi = fp16(x), lo' = fp16((x - hi) 2^11)  (csrc/xattn_h2.hip has the why)
// ---------------------------------------------------------------------------
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
constexpr float LO_UP = 2048.0f, LO_DOWN = 1.0f / 2048.0f;
constexpr float H_MAX = 65504.0f;

__device__ __forceinline__ void split_h2(float x, _Float16& hi, _Float16& lo) {
  hi = (_Float16)x;
  lo = (_Float16)((x - (float)hi) * LO_UP);
}

__device__ __forceinline__ void split8_h2(const float4 u, const float4 v, h16x8& h, h16x8& l) {
  const float f[8] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    _Float16 a, c;
    split_h2(f[i], a, c);
    h[i] = a;
    l[i] = c;
  }
}

// one product block step: small terms into acc2 (carries 2^-11) first, the hi hi term into acc1 last
__device__ __forceinline__ void mfma3(const h16x8 ah, const h16x8 al, const h16x8 bh, const h16x8 bl, f32x16& acc1, f32x16& acc2) {
  acc2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc2, 0, 0, 0);
  acc2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc2, 0, 0, 0);
  acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc1, 0, 0, 0);
}

// the weight fragments of one 32-row tile over the whole 128-long contraction: 8 steps x 2 parts x 16 bytes per lane = 64 VGPRs
struct WFragH { h16x8 w[NS][2]; };

__device__ __forceinline__ void load_wh(WFragH& f, const _Float16* wp) {
#pragma unroll
  for (int s = 0; s < NS; ++s) {
#pragma unroll
    for (int p = 0; p < 2; ++p) f.w[s][p] = *reinterpret_cast<const h16x8*>(wp + (long)s * 1024 + p * 512);
  }
}

// Staging of rows [0, 32) of a row-major [*, 128] fp32 matrix as two fp16 planes (rows >= M: zeros), thread = row tid / 8, two K
// octets -- in two halves: global loads into registers (issued early), split + LDS stores (once the planes are free).
struct RowRegs { float4 u[2], v[2]; };

__device__ __forceinline__ void rows_load(RowRegs& r, const float* __restrict__ src, int M, int tid) {
  const int row = tid >> 3;
  const bool ok = row < M;
  const float* s = src + (long)(ok ? row : 0) * E128;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int o = (tid & 7) + 8 * i;
    r.u[i] = r.v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ok) {
      r.u[i] = ld4(s + 8 * o);
      r.v[i] = ld4(s + 8 * o + 4);
    }
  }
}

__device__ __forceinline__ void rows_store(_Float16* planes, const RowRegs& r, int tid) {
  const int row = tid >> 3;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int o = (tid & 7) + 8 * i;
    h16x8 h, l;
    split8_h2(r.u[i], r.v[i], h, l);
    _Float16* d = planes + row * PROW + 8 * o;
    *reinterpret_cast<h16x8*>(d) = h;
    *reinterpret_cast<h16x8*>(d + PLANE) = l;
  }
}

// both halves in one, rows [m0, m0 + 32).  Written out: composed of rows_load + rows_store, every layer_tail_h2_kernel and
// xattn_main_h2_kernel instance came out different (up to 9 more s_waitcnt)
__device__ __forceinline__ void stage_rows_h2(_Float16* planes, const float* __restrict__ src, int m0, int M, int tid) {
  const int row = tid >> 3;
  const bool ok = m0 + row < M;
  const float* s = src + (long)(ok ? m0 + row : 0) * E128;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int o = (tid & 7) + 8 * i;                     // octet of the row
    float4 u = make_float4(0.f, 0.f, 0.f, 0.f), v = u;
    if (ok) {
      u = ld4(s + 8 * o);
      v = ld4(s + 8 * o + 4);
    }
    h16x8 h, l;
    split8_h2(u, v, h, l);
    _Float16* d = planes + row * PROW + 8 * o;
    *reinterpret_cast<h16x8*>(d) = h;
    *reinterpret_cast<h16x8*>(d + PLANE) = l;
  }
}

// the 32 x 128 fp32 tile in Cs -> two fp16 planes
__device__ __forceinline__ void tile_to_planes_h2(_Float16* planes, const float (*Cs)[E128 + 1], int tid) {
  const int row = tid >> 3;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int o = (tid & 7) + 8 * i;
    const float* c = &Cs[row][8 * o];
    h16x8 h, l;
    split8_h2(make_float4(c[0], c[1], c[2], c[3]), make_float4(c[4], c[5], c[6], c[7]), h, l);
    _Float16* d = planes + row * PROW + 8 * o;
    *reinterpret_cast<h16x8*>(d) = h;
    *reinterpret_cast<h16x8*>(d + PLANE) = l;
  }
}

// D^T[n][m] = sum_k W[n][k] X[m][k]: weight fragments = A operand, plane rows = B operand.  FENCE: a scheduling barrier every
// two steps keeps the compiler from hoisting all sixteen LDS reads (64 registers) above the MFMAs (the 128-VGPR pre-pass).
template <bool FENCE = false>
__device__ __forceinline__ void project_t(const WFragH& f, const _Float16* planes, int l31, int hh, f32x16& a1, f32x16& a2) {
  const _Float16* pb = planes + l31 * PROW + 8 * hh;
#pragma unroll
  for (int st = 0; st < NS; ++st) {
    const h16x8 xh = *reinterpret_cast<const h16x8*>(pb + 16 * st);
    const h16x8 xl = *reinterpret_cast<const h16x8*>(pb + 16 * st + PLANE);
    mfma3(f.w[st][0], f.w[st][1], xh, xl, a1, a2);
    if (FENCE && (st & 1)) __builtin_amdgcn_sched_barrier(0);
  }
}

// D[m][n] = sum_k X[m][k] W[n][k]: plane rows = A operand, weight fragments = B operand (rows = the tile's rows, columns = the
// fragment's 32 outputs).  No FENCE flag: its two fenced uses, the V projections of csrc/xattn_h2.hip, stay written out there --
// through this helper xattn_kv_h2_kernel took 4 more VGPRs, and with only one of the two through it the other kernel changed.
__device__ __forceinline__ void project_s(const _Float16* planes, const WFragH& f, int l31, int hh, f32x16& a1, f32x16& a2) {
  const _Float16* pa = planes + l31 * PROW + 8 * hh;
#pragma unroll
  for (int st = 0; st < NS; ++st) {
    const h16x8 xh = *reinterpret_cast<const h16x8*>(pa + 16 * st);
    const h16x8 xl = *reinterpret_cast<const h16x8*>(pa + 16 * st + PLANE);
    mfma3(xh, xl, f.w[st][0], f.w[st][1], a1, a2);
  }
}

// registers 8 t .. 8 t + 7 of an accumulator-shaped value -> the two fp16 parts of k-step t of an MFMA operand
__device__ __forceinline__ void pack_steps(const f32x16 v, h16x8 (&hi)[2], h16x8 (&lo)[2]) {
#pragma unroll
  for (int t = 0; t < 2; ++t) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      _Float16 a, c;
      split_h2(v[8 * t + e], a, c);
      hi[t][e] = a;
      lo[t][e] = c;
    }
  }
}

// ---------------------------------------------------------------------------
// split3: v = h + m + l, h = bf16(v), m = bf16(v - h), l = bf16(v - h - m)  (csrc/token_split3.hip has the why)
// ---------------------------------------------------------------------------
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ void split1x3(float v, __bf16& h, __bf16& m, __bf16& l) {
  const __bf16 a = (__bf16)v;
  const float r1 = v - (float)a;
  const __bf16 b = (__bf16)r1;
  h = a;
  m = b;
  l = (__bf16)(r1 - (float)b);
}

__device__ __forceinline__ void split8x3(const float4 u, const float4 v, bf16x8& h, bf16x8& m, bf16x8& l) {
  const float f[8] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 8; ++i) {       // written out, not through split1x3: with it every lin3_kernel schedules its conversions differently
    const __bf16 a = (__bf16)f[i];
    const float r1 = f[i] - (float)a;
    const __bf16 b = (__bf16)r1;
    h[i] = a;
    m[i] = b;
    l[i] = (__bf16)(r1 - (float)b);
  }
}

__device__ __forceinline__ f32x16 mfma6(const bf16x8 ah, const bf16x8 am, const bf16x8 al, const bf16x8 bh, const bf16x8 bm,
                                        const bf16x8 bl, f32x16 acc) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);      // small terms first
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
  return acc;
}

// The weight fragments of one channel tile over a whole K chunk, resident in VGPRs (8 K steps x 3 parts x 16 bytes per
// lane = 96 registers): loaded a phase ahead of their use, so the L2 latency of the stream sits under the previous
// phase's MFMAs (loaded just in time, each group of six MFMAs waited for its own three loads: the first version of
// these kernels ran SLOWER than the exact-fp32 ones, 160 us against 122 us per encoder layer).
struct WFrag3 { bf16x8 w[KC / 16][3]; };

__device__ __forceinline__ void load_w3(WFrag3& f, const __bf16* wp, int nsteps) {
#pragma unroll
  for (int s = 0; s < KC / 16; ++s) {
    if (s < nsteps) {
#pragma unroll
      for (int p = 0; p < 3; ++p) f.w[s][p] = *reinterpret_cast<const bf16x8*>(wp + (long)s * 1536 + p * 512);
    }
  }
}

// 256 threads stage rows [m0, m0 + 32) x columns [k0, k0 + kc) of a row-major fp32 matrix as three bf16 planes
__device__ __forceinline__ void stage_rows3(__bf16* planes, const float* __restrict__ src, int ld, int m0, int M, int k0, int kc,
                                            int tid) {
  const int row = tid >> 3;
  const bool ok = m0 + row < M;
  const float* s = src + (long)(ok ? m0 + row : 0) * ld + k0;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int o = (tid & 7) + 8 * i;                     // K octet of the chunk
    float4 u = make_float4(0.f, 0.f, 0.f, 0.f), v = u;
    if (ok && 8 * o < kc) {
      u = ld4(s + 8 * o);
      v = ld4(s + 8 * o + 4);
    }
    bf16x8 h, m, l;
    split8x3(u, v, h, m, l);
    __bf16* d = planes + row * PROW + 8 * o;
    *reinterpret_cast<bf16x8*>(d) = h;
    *reinterpret_cast<bf16x8*>(d + PLANE) = m;
    *reinterpret_cast<bf16x8*>(d + 2 * PLANE) = l;
  }
}

// the 32 x 128 fp32 tile in Cs -> three bf16 planes
__device__ __forceinline__ void tile_to_planes3(__bf16* planes, const float (*Cs)[E128 + 1], int tid) {
  const int row = tid >> 3;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int o = (tid & 7) + 8 * i;
    const float* c = &Cs[row][8 * o];
    bf16x8 h, m, l;
    split8x3(make_float4(c[0], c[1], c[2], c[3]), make_float4(c[4], c[5], c[6], c[7]), h, m, l);
    __bf16* d = planes + row * PROW + 8 * o;
    *reinterpret_cast<bf16x8*>(d) = h;
    *reinterpret_cast<bf16x8*>(d + PLANE) = m;
    *reinterpret_cast<bf16x8*>(d + 2 * PLANE) = l;
  }
}

// acc += planes[32 x (16 nsteps)] . (resident fragments)^T : plane rows = A operand, fragments = B operand
__device__ __forceinline__ f32x16 chunk_mfma3(f32x16 acc, const __bf16* planes, const WFrag3& f, int nsteps, int l31, int hh) {
  const __bf16* pa = planes + l31 * PROW + 8 * hh;
#pragma unroll
  for (int s = 0; s < KC / 16; ++s) {
    if (s < nsteps) {
      const bf16x8 ah = *reinterpret_cast<const bf16x8*>(pa + 16 * s);
      const bf16x8 am = *reinterpret_cast<const bf16x8*>(pa + 16 * s + PLANE);
      const bf16x8 al = *reinterpret_cast<const bf16x8*>(pa + 16 * s + 2 * PLANE);
      acc = mfma6(ah, am, al, f.w[s][0], f.w[s][1], f.w[s][2], acc);
    }
  }
  return acc;
}

// ---------------------------------------------------------------------------
// common
// ---------------------------------------------------------------------------
// LayerNorm of the 32 x 128 tile in Cs, IN PLACE (one wavefront per 8 rows)
__device__ __forceinline__ void ln_tile_inplace(float (*Cs)[E128 + 1], const float* gamma, const float* beta, float eps, int lane,
                                                int wave) {
  const float g0 = gamma[lane], g1 = gamma[lane + 64];
  const float b0 = beta[lane], b1 = beta[lane + 64];
#pragma unroll 4
  for (int i = 0; i < TM / 4; ++i) {
    const int row = wave * (TM / 4) + i;
    const float x0 = Cs[row][lane], x1 = Cs[row][lane + 64];
    const float mean = wave_sum(x0 + x1) * (1.0f / E128);
    const float d0 = x0 - mean, d1 = x1 - mean;
    const float var = wave_sum(d0 * d0 + d1 * d1) * (1.0f / E128);
    const float rstd = 1.0f / sqrtf(var + eps);
    Cs[row][lane] = d0 * rstd * g0 + b0;
    Cs[row][lane + 64] = d1 * rstd * g1 + b1;
  }
}

// LayerNorm over the 128 columns of a 32-row tile held in Cs (one wavefront per 8 rows), stored to rows m0 .. of ``out``;
// rows flagged in zero_mask (nullable) are written as zeros
__device__ __forceinline__ void ln_rows(const float (*Cs)[E128 + 1], const float* gamma, const float* beta, float eps,
                                        const uint8_t* zero_mask, float* out, int ldo, int m0, int M, int lane, int wave) {
  const float g0 = gamma[lane], g1 = gamma[lane + 64];
  const float b0 = beta[lane], b1 = beta[lane + 64];
#pragma unroll
  for (int i = 0; i < TM / 4; ++i) {
    const int row = wave * (TM / 4) + i, m = m0 + row;
    const float x0 = Cs[row][lane], x1 = Cs[row][lane + 64];
    const float mean = wave_sum(x0 + x1) * (1.0f / E128);
    const float d0 = x0 - mean, d1 = x1 - mean;
    const float var = wave_sum(d0 * d0 + d1 * d1) * (1.0f / E128);
    const float rstd = 1.0f / sqrtf(var + eps);
    if (m < M) {
      const bool z = zero_mask != nullptr && zero_mask[m] != 0;
      out[(long)m * ldo + lane] = z ? 0.f : d0 * rstd * g0 + b0;
      out[(long)m * ldo + lane + 64] = z ? 0.f : d1 * rstd * g1 + b1;
    }
  }
}

// NOT here: the softmax over <= 32 keys of the three few-key attention kernels (mask add, in-lane max + xor-32, "every key masked
// -> NaN as torch").  As a helper -- scores by reference or by value, the exponential a callable or a template flag, the mask a
// pointer or an array reference -- it changed cross_attn_fused_kernel and xattn_main3_kernel<2> (which lost its 36 bytes of scratch
// and 14 instructions: another kernel), so the block stays written out at its three sites; a change to the all-masked rule is
// made in csrc/linear.hip, xattn_split3.hip and xattn_h2.hip.

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// What both ocv_layer_tail_*_fwd entry points check, in their order, before they look at alignment.  ``name``: the entry point for
// the messages; ``sfx``: "h2" | "p3", as in its next_in_proj_* argument; ``has_weights(view)``: whether the layer carries the route's
// packed weights, ``weights_text`` the message if not.  Fills ``pv`` with the library's view of the caller's struct.  0 / -1.
template <class HasWeights>
static inline int ocv_layer_tail_check(const char* name, const char* sfx, const float* ctx, const float* x,
                                       const ocv_encoder_layer_params* p_caller, HasWeights has_weights, const char* weights_text,
                                       const void* next_in_proj, const float* next_in_proj_b, const uint8_t* zero_row_mask,
                                       const float* out, const float* qkv_next, int E, int FF, ocv_encoder_layer_params* pv) {
  OCV_CHECK_ARG(ctx && x && p_caller && out, "%s: null pointer", name);
  OCV_CHECK_ARG(ocv_layer_params_view(p_caller, 0, pv), "%s: params->struct_size (%zu) is not a valid ocv_encoder_layer_params size", name, p_caller->struct_size);
  OCV_CHECK_ARG(has_weights(*pv), "%s: %s", name, weights_text);
  OCV_CHECK_ARG(E == E128 && FF >= KC && FF % KC == 0, "%s: needs E = %d and FF a multiple of %d (got %d, %d)", name, E128, KC, E, FF);
  OCV_CHECK_ARG((next_in_proj == nullptr) == (qkv_next == nullptr) && (next_in_proj == nullptr || next_in_proj_b != nullptr),
                "%s: next_in_proj_%s / next_in_proj_b / qkv_next go together", name, sfx);
  // (the kernel projects the LN2 tile it holds, not the zeroed rows it stores: only the last layer of a stack is masked, and it has no next)
  OCV_CHECK_ARG(zero_row_mask == nullptr || qkv_next == nullptr, "%s: zero_row_mask together with a next projection (qkv_next) is not supported", name);
  return 0;
}
