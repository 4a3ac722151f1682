// Weight packers of the token path: a static W [N][K] fp32 (row stride ldw) -> MFMA operand fragments, split once on the device,
//   Wp[((jt * (K/16) + s) * PARTS + part) * 512 + lane * 8 + e] = part of W[32 jt + (lane & 31)][16 s + 8 (lane >> 5) + e],
// zero beyond N and K, so a wavefront's weight load is one contiguous 1 KB run per (channel tile, K step, part).
//   ocv_pack_split3_fwd     three bf16 terms (csrc/token_split3.hip, xattn_split3.hip, bin_head.hip)
//   ocv_pack_split_h2_fwd   two fp16 terms, saturated at +-65504 (csrc/token_h2.hip, xattn_h2.hip, bin_head.hip)
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include "token_tile.hpp"
#include "../../include/objcavit_hip.h"

namespace {

// item i = (jt, s, lane) -> row n and first column k0 of its eight source elements, js = jt * nsteps + s
struct PackItem { int n, k0; long js; };

__device__ __forceinline__ PackItem pack_item(long i, int K) {
  const int lane = (int)(i & 63);
  const long js = i >> 6;
  const int nsteps = (K + 15) >> 4;
  const int s = (int)(js % nsteps), jt = (int)(js / nsteps);
  return {jt * 32 + (lane & 31), 16 * s + 8 * (lane >> 5), js};
}

// one thread per (jt, s, lane); zero beyond N and K
__global__ __launch_bounds__(256) void pack3_kernel(const float* __restrict__ W, int ldw, int N, int K, __bf16* __restrict__ out,
                                                    long items) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= items) return;
  const PackItem it = pack_item(i, K);
  float f[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) f[e] = (it.n < N && it.k0 + e < K) ? W[(long)it.n * ldw + it.k0 + e] : 0.f;
  bf16x8 h, m, l;
  split8x3(make_float4(f[0], f[1], f[2], f[3]), make_float4(f[4], f[5], f[6], f[7]), h, m, l);
  __bf16* d = out + (it.js * 3) * 512 + (i & 63) * 8;
  *reinterpret_cast<bf16x8*>(d) = h;
  *reinterpret_cast<bf16x8*>(d + 512) = m;
  *reinterpret_cast<bf16x8*>(d + 1024) = l;
}

__global__ __launch_bounds__(256) void pack_h2_kernel(const float* __restrict__ W, int ldw, int N, int K, _Float16* __restrict__ out,
                                                      long items) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= items) return;
  const PackItem it = pack_item(i, K);
  float f[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float w = (it.n < N && it.k0 + e < K) ? W[(long)it.n * ldw + it.k0 + e] : 0.f;
    f[e] = fabsf(w) > H_MAX ? copysignf(H_MAX, w) : w;                 // saturate; a NaN fails the comparison and stays a NaN
  }
  h16x8 h, l;
  split8_h2(make_float4(f[0], f[1], f[2], f[3]), make_float4(f[4], f[5], f[6], f[7]), h, l);
  _Float16* d = out + (it.js * 2) * 512 + (i & 63) * 8;
  *reinterpret_cast<h16x8*>(d) = h;
  *reinterpret_cast<h16x8*>(d + 512) = l;
}

long pack_items(int N, int K) { return (long)((N + 31) / 32) * ((K + 15) / 16) * 64; }

}  // namespace

extern "C" size_t ocv_split3_packed_elems(int N, int K) {
  if (N < 1 || K < 1) return 0;
  return (size_t)pack_items(N, K) * 8 * 3;
}

extern "C" size_t ocv_split_h2_packed_elems(int N, int K) {
  if (N < 1 || K < 1) return 0;
  return (size_t)pack_items(N, K) * 8 * 2;
}

extern "C" int ocv_pack_split3_fwd(const float* W, int ldw, int N, int K, void* packed, ocv_stream_t stream) {
  OCV_CHECK_ARG(W && packed, "ocv_pack_split3_fwd: null pointer");
  OCV_CHECK_ARG(N >= 1 && K >= 1 && ldw >= K, "ocv_pack_split3_fwd: bad sizes N=%d K=%d ldw=%d", N, K, ldw);
  OCV_CHECK_ARG(ocv_aligned16(packed), "ocv_pack_split3_fwd: packed must be 16-byte aligned");
  const long items = pack_items(N, K);
  hipLaunchKernelGGL(pack3_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, (hipStream_t)stream, W, ldw, N, K,
                     (__bf16*)packed, items);
  OCV_CHECK_LAUNCH("ocv_pack_split3_fwd");
  return 0;
}

extern "C" int ocv_pack_split_h2_fwd(const float* W, int ldw, int N, int K, void* packed, ocv_stream_t stream) {
  OCV_CHECK_ARG(W && packed, "ocv_pack_split_h2_fwd: null pointer");
  OCV_CHECK_ARG(N >= 1 && K >= 1 && ldw >= K, "ocv_pack_split_h2_fwd: bad sizes N=%d K=%d ldw=%d", N, K, ldw);
  OCV_CHECK_ARG(ocv_aligned16(packed), "ocv_pack_split_h2_fwd: packed must be 16-byte aligned");
  const long items = pack_items(N, K);
  hipLaunchKernelGGL(pack_h2_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, (hipStream_t)stream, W, ldw, N, K,
                     (_Float16*)packed, items);
  OCV_CHECK_LAUNCH("ocv_pack_split_h2_fwd");
  return 0;
}
