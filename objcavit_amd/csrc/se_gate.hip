// Squeeze-excite of the EfficientNet MBConv blocks (row N1 of SURVEY.md section 8; the reference runs the se module of the hub
// backbone's blocks, modules/DenseFeatureExtractor.py:18-27,149):
//
//   gate[b][c] = sigmoid( b2[c] + sum_r W2t[r][c] * silu( b1[r] + sum_c' W1[r][c'] * mean[b][c'] ) )
//
// mean = the per-(image, channel) mean over H x W of the depthwise output, from either of two sources:
//   ocv_channel_mean_nhwc_fwd + ocv_se_gate_fwd   a pass of its own over the activation (channel_sum_kernel,
//                                                 channel_mean_finish_kernel), then se_hidden_kernel + se_gate_hid_kernel
//   ocv_se_gate_partials_fwd                      the pooling partials part[b][tile][c] the depthwise kernels write beside their
//                                                 output (csrc/depthwise_se.hip, mbconv_fused.hip): se_fused_small_kernel, or
//                                                 se_hidden_partials_kernel + se_gate_hid_kernel where the weights are large
//   ocv_se_gate_weights_fwd                       the same with the gate FOLDED INTO the project weights per image
//                                                 (se_hidden_partials_kernel + se_gate_weights_kernel), for csrc/pointwise_hl.hip
// All of them are latency-bound launches of a few us.  The three pieces -- pooling of the partials (se_pool_mean), a hidden
// unit's dot (se_hidden_sum), a channel's gate dot (se_gate_sum) -- exist once, so every route sums in the same fixed order and
// the routes' gates are bit-identical to each other (tests/test_hip_memory_bounds.py compares them with torch.equal).
#include "mbconv_tile.hpp"

namespace {

// Pooling of the partials of one image: mean[c] = (sum_tile pb[tile][c]) * inv, by all 1024 threads of the workgroup, through
// red[TG][C]; returns TG.  Item = (channel QUAD, row group); every thread keeps eight independent 16-byte loads in flight.  (Round 4:
// the first version summed one float per load, four in flight -- at bs 1, where a depthwise launch leaves up to 600 partial rows per
// image, that was 38 dependent round trips and 10.7 us per launch, 0.42 ms of a 4 ms forward; profiles/r04a_*.)  Out-of-range rows
// are clamped to a valid address and selected away: no branch around a load.  Fixed order: rows ascending within a group, groups
// ascending.  C % 4 == 0 (the depthwise kernels' contract); TG * C <= max(C, 4096) floats (se_pool_lds).
__device__ __forceinline__ int se_pool_mean(const float* __restrict__ pb, int tiles, float inv, int C, float* mean, float* red) {
  const int tid = threadIdx.x;
  const int nq = C >> 2;
  const int TG = nq >= 1024 ? 1 : min(tiles, 1024 / nq);
  for (int idx = tid; idx < TG * nq; idx += 1024) {
    const int q = idx % nq, tg = idx / nq;
    float4 a[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    const float* src = pb + 4 * q;
    for (int t0 = tg; t0 < tiles; t0 += 8 * TG) {
      float4 u[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) u[j] = ld4(src + (long)min(t0 + j * TG, tiles - 1) * C);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bool ok = t0 + j * TG < tiles;
        a[j].x += ok ? u[j].x : 0.f; a[j].y += ok ? u[j].y : 0.f; a[j].z += ok ? u[j].z : 0.f; a[j].w += ok ? u[j].w : 0.f;
      }
    }
    float4 r;
    r.x = ((a[0].x + a[1].x) + (a[2].x + a[3].x)) + ((a[4].x + a[5].x) + (a[6].x + a[7].x));
    r.y = ((a[0].y + a[1].y) + (a[2].y + a[3].y)) + ((a[4].y + a[5].y) + (a[6].y + a[7].y));
    r.z = ((a[0].z + a[1].z) + (a[2].z + a[3].z)) + ((a[4].z + a[5].z) + (a[6].z + a[7].z));
    r.w = ((a[0].w + a[1].w) + (a[2].w + a[3].w)) + ((a[4].w + a[5].w) + (a[6].w + a[7].w));
    *reinterpret_cast<float4*>(red + tg * C + 4 * q) = r;
  }
  __syncthreads();
  for (int c = tid; c < C; c += 1024) {
    float s = red[c];
    for (int tg = 1; tg < TG; ++tg) s += red[tg * C + c];
    mean[c] = s * inv;
  }
  __syncthreads();
  return TG;
}

// W1[r] . mean by one wavefront (``wr`` = the row of W1, ``mean`` in LDS, nq = C / 4): a lane takes channel QUADS lane, lane + 64,
// ... -- 16-byte loads, four of them in flight (C <= 1024: the whole row of W1 in one round trip; one float per load took C / 256
// dependent rounds).  Every lane returns the sum.
__device__ __forceinline__ float se_hidden_sum(const float* __restrict__ wr, const float* mean, int nq, int lane) {
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int q = lane;
  for (; q + 192 < nq; q += 256) {
    const float4 u0 = ld4(wr + 4 * q), u1 = ld4(wr + 4 * (q + 64)), u2 = ld4(wr + 4 * (q + 128)), u3 = ld4(wr + 4 * (q + 192));
    const float4 m0 = *reinterpret_cast<const float4*>(mean + 4 * q), m1 = *reinterpret_cast<const float4*>(mean + 4 * (q + 64));
    const float4 m2 = *reinterpret_cast<const float4*>(mean + 4 * (q + 128)), m3 = *reinterpret_cast<const float4*>(mean + 4 * (q + 192));
    s0 = fmaf(u0.x, m0.x, fmaf(u0.y, m0.y, fmaf(u0.z, m0.z, fmaf(u0.w, m0.w, s0))));
    s1 = fmaf(u1.x, m1.x, fmaf(u1.y, m1.y, fmaf(u1.z, m1.z, fmaf(u1.w, m1.w, s1))));
    s2 = fmaf(u2.x, m2.x, fmaf(u2.y, m2.y, fmaf(u2.z, m2.z, fmaf(u2.w, m2.w, s2))));
    s3 = fmaf(u3.x, m3.x, fmaf(u3.y, m3.y, fmaf(u3.z, m3.z, fmaf(u3.w, m3.w, s3))));
  }
  for (; q < nq; q += 64) {
    const float4 u0 = ld4(wr + 4 * q);
    const float4 m0 = *reinterpret_cast<const float4*>(mean + 4 * q);
    s0 = fmaf(u0.x, m0.x, fmaf(u0.y, m0.y, fmaf(u0.z, m0.z, fmaf(u0.w, m0.w, s0))));
  }
  return wave_sum((s0 + s1) + (s2 + s3));
}

// b2[c] + sum_r W2t[r][c] hs[r] for one channel (``w`` = W2t + c, ``hs`` = the image's hidden units in LDS, ``bias`` = b2[c]): four
// accumulators over r mod 4, sixteen loads in flight (four were: R / 4 dependent round trips).
__device__ __forceinline__ float se_gate_sum(const float* __restrict__ w, const float* hs, float bias, int C, int R) {
  float s0 = bias, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int r = 0;
  for (; r + 15 < R; r += 16) {
    float u[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) u[j] = w[(long)(r + j) * C];
#pragma unroll
    for (int j = 0; j < 16; j += 4) {
      s0 = fmaf(u[j], hs[r + j], s0);
      s1 = fmaf(u[j + 1], hs[r + j + 1], s1);
      s2 = fmaf(u[j + 2], hs[r + j + 2], s2);
      s3 = fmaf(u[j + 3], hs[r + j + 3], s3);
    }
  }
  for (; r + 3 < R; r += 4) {
    s0 = fmaf(w[(long)r * C], hs[r], s0);
    s1 = fmaf(w[(long)(r + 1) * C], hs[r + 1], s1);
    s2 = fmaf(w[(long)(r + 2) * C], hs[r + 2], s2);
    s3 = fmaf(w[(long)(r + 3) * C], hs[r + 3], s3);
  }
  for (; r < R; ++r) s0 = fmaf(w[(long)r * C], hs[r], s0);
  return (s0 + s1) + (s2 + s3);
}

// ---------------------------------------------------------------------------
// channel mean over H*W (squeeze), NHWC.  Stage 1: grid (C/64 chunks, splits, B), 256 threads = 16 pixel lanes x
// 16 channel quads; partial sums in fixed order.  Stage 2: add the splits in order and scale.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void channel_sum_kernel(const float* __restrict__ x, float* __restrict__ part, long P,
                                                          int C, int splits) {
  __shared__ float4 red[16][16];
  const int q = threadIdx.x & 15, pl = threadIdx.x >> 4;
  const int c = (blockIdx.x * 16 + q) * 4;
  const int sp = blockIdx.y;
  const long b = blockIdx.z;
  const long per = (P + splits - 1) / splits;
  const long p0 = sp * per, p1 = min(P, p0 + per);
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (c < C) {
    const float* src = x + b * P * C + c;
    for (long pix = p0 + pl; pix < p1; pix += 16) {
      const float4 v = ld4(src + pix * C);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
  }
  red[pl][q] = s;
  __syncthreads();
  if (pl == 0 && c < C) {
    float4 t = red[0][q];
#pragma unroll
    for (int i = 1; i < 16; ++i) { t.x += red[i][q].x; t.y += red[i][q].y; t.z += red[i][q].z; t.w += red[i][q].w; }
    *reinterpret_cast<float4*>(part + ((b * splits + sp) * (long)C) + c) = t;
  }
}

__global__ __launch_bounds__(256) void channel_mean_finish_kernel(const float* __restrict__ part, float* __restrict__ out,
                                                                  int C, int splits, float inv, long total) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;      // over B * C
  if (i >= total) return;
  const long b = i / C;
  const int c = (int)(i - b * C);
  float s = 0.f;
  for (int sp = 0; sp < splits; ++sp) s += part[(b * splits + sp) * (long)C + c];
  out[i] = s * inv;
}

int mean_splits(int B, int C, long P) {
  const int chunks = (C + 63) / 64;
  int s = 1;
  while (s < 64 && (long)B * chunks * s < 1024 && P / (s * 2) >= 256) s *= 2;
  return s;
}

// Hidden layer from a mean in MEMORY (ocv_se_gate_fwd): one wavefront per (r, b), one float per lane and load, coalesced over c.
// Its scalar summation order is not se_hidden_sum's quad order -- other bits -- so it stays a kernel of its own.
__global__ __launch_bounds__(256) void se_hidden_kernel(const float* __restrict__ mean, const float* __restrict__ w1,
                                                        const float* __restrict__ b1, float* __restrict__ hid, int C,
                                                        int R) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  const long b = blockIdx.y;
  const float* mb = mean + b * C;
  const float* wr = w1 + (long)r * C;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int c = lane;
  for (; c + 192 < C; c += 256) {
    s0 = fmaf(wr[c], mb[c], s0);
    s1 = fmaf(wr[c + 64], mb[c + 64], s1);
    s2 = fmaf(wr[c + 128], mb[c + 128], s2);
    s3 = fmaf(wr[c + 192], mb[c + 192], s3);
  }
  for (; c < C; c += 64) s0 = fmaf(wr[c], mb[c], s0);
  const float s = wave_sum((s0 + s1) + (s2 + s3));
  if (lane == 0) {
    const float v = s + b1[r];
    hid[b * R + r] = fast_silu(v);
  }
}

// squeeze-excite gate from the pooling partials, two small launches (both latency-bound, so both are spread wide):
//   se_hidden_partials_kernel  grid (ceil(R / 16), B): mean[c] = (sum_tile part) / P into LDS (every workgroup of an
//                              image repeats this: tiles x C floats from L2), then one wavefront per hidden unit:
//                              hid[b][r] = silu(b1[r] + W1[r] . mean)
//   se_gate_hid_kernel         grid (ceil(C / 256), B): gate[b][c] = sigmoid(b2[c] + sum_r W2t[r][c] hid[b][r])
__global__ __launch_bounds__(1024) void se_hidden_partials_kernel(const float* __restrict__ part, int tiles, float inv,
                                                                 const float* __restrict__ w1, const float* __restrict__ b1,
                                                                 float* __restrict__ hid, int C, int R) {
  extern __shared__ float sm[];            // mean[C] | red[TG][C]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long b = blockIdx.y;
  se_pool_mean(part + b * tiles * (long)C, tiles, inv, C, sm, sm + C);
  const int r = blockIdx.x * 16 + wave;
  if (r >= R) return;
  const float s = se_hidden_sum(w1 + (long)r * C, sm, C >> 2, lane);
  if (lane == 0) hid[b * R + r] = fast_silu(s + b1[r]);
}

__global__ __launch_bounds__(256) void se_gate_hid_kernel(const float* __restrict__ hid, const float* __restrict__ w2t,
                                                          const float* __restrict__ b2, float* __restrict__ gate, int C,
                                                          int R) {
  __shared__ float hs[256];
  const long b = blockIdx.y;
  if (threadIdx.x < R) hs[threadIdx.x] = hid[b * R + threadIdx.x];
  __syncthreads();
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  gate[b * C + c] = fast_sigmoid(se_gate_sum(w2t + c, hs, b2[c], C, R));
}

// Both launches above as ONE, for the blocks whose squeeze-excite weights are small (round 4: B5's stages 1 - 5, 27 of 39 blocks):
// grid (ceil(C / 256), B), 1024 threads; every workgroup of an image repeats the pooling and ALL hidden units (<= 64 of them: W1 is
// <= 186 KB, L2-resident) and then forms the gate of its own 256 channels.  The same three pieces with the same thread -> element
// maps, so the gate is bit-identical to the two kernels'; what goes away is one launch floor (~4.5 us) and the hidden units' round
// trip through memory: 7.3 + 5.1 -> ~8.5 us at bs 1.
__global__ __launch_bounds__(1024) void se_fused_small_kernel(const float* __restrict__ part, int tiles, float inv,
                                                             const float* __restrict__ w1, const float* __restrict__ b1,
                                                             const float* __restrict__ w2t, const float* __restrict__ b2,
                                                             float* __restrict__ gate, int C, int R) {
  extern __shared__ float sm[];            // mean[C] | red[TG][C] | hs[128]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long b = blockIdx.y;
  const int TG = se_pool_mean(part + b * tiles * (long)C, tiles, inv, C, sm, sm + C);
  float* hs = sm + C + (size_t)TG * C;
  for (int r = wave; r < R; r += 16) {                 // every hidden unit, one wavefront each
    const float s = se_hidden_sum(w1 + (long)r * C, sm, C >> 2, lane);
    if (lane == 0) hs[r] = fast_silu(s + b1[r]);
  }
  __syncthreads();
  const int c = blockIdx.x * 256 + tid;
  if (tid >= 256 || c >= C) return;
  gate[b * C + c] = fast_sigmoid(se_gate_sum(w2t + c, hs, b2[c], C, R));
}

// The gate FOLDED INTO THE PROJECT WEIGHTS, per image: Wg[b][n][k] = W[n][k] * gate[b][k], split (hi = bf16, lo = bf16 of the
// rest) and packed in the B-operand order of the pointwise kernels (w_frag, mbconv_tile.hpp; hip_ops.SplitWeight) -- so that
// the project convolution's row operand is the depthwise output AS STORED (hl32, LDS-DMA) instead of rows re-gated and
// re-split by every workgroup that touches them.  Grid (ceil(K / 64), B): a workgroup forms the gate of its 64 input
// channels and scales / splits / packs their column block of W for all N rows; thread = (octet of 8 inputs, one of 32
// consecutive output rows): a wavefront half writes 512 contiguous bytes.
__global__ __launch_bounds__(256) void se_gate_weights_kernel(const float* __restrict__ hid, const float* __restrict__ w2t,
                                                              const float* __restrict__ b2, const float* __restrict__ W,
                                                              __bf16* __restrict__ wpk, long img_elems, float* __restrict__ gate,
                                                              int C, int R, int N) {
  __shared__ float hs[256];
  __shared__ __attribute__((aligned(16))) float gs[64];
  const long b = blockIdx.y;
  const int tid = threadIdx.x;
  const int k0 = blockIdx.x * 64;
  if (tid < R) hs[tid] = hid[b * R + tid];
  __syncthreads();
  if (tid < 64) {
    const int c = k0 + tid;
    float g = 0.f;                                   // inputs past C (K padded to 16): weight columns of zeros
    if (c < C) {
      g = fast_sigmoid(se_gate_sum(w2t + c, hs, b2[c], C, R));
      if (gate != nullptr) gate[b * C + c] = g;
    }
    gs[tid] = g;
  }
  __syncthreads();
  const int o = tid >> 5, nl = tid & 31;             // octet of the 64-channel block, row inside a 32-row channel tile
  const int k = k0 + 8 * o;
  const int Kp = (C + 15) & ~15;
  if (k >= Kp) return;
  const float4 g0 = *reinterpret_cast<const float4*>(gs + 8 * o), g1 = *reinterpret_cast<const float4*>(gs + 8 * o + 4);
  __bf16* ob = wpk + b * img_elems;
  const int ntl = (N + 31) >> 5;
  for (int jt = 0; jt < ntl; ++jt) {
    const int n = jt * 32 + nl;
    float4 u = make_float4(0.f, 0.f, 0.f, 0.f), v = u;
    if (n < N && k < C) {                            // C is a multiple of 8: an octet is inside or outside as a whole
      u = mul4(ld4(W + (long)n * C + k), g0);
      v = mul4(ld4(W + (long)n * C + k + 4), g1);
    }
    bf16x8 h, l;
    split8(u, v, h, l);
    __bf16* d = w_frag(ob, jt, Kp, k >> 4, ((k >> 3) & 1) * 32 + nl);      // this thread is lane 32 hh + nl of the fragment
    *reinterpret_cast<bf16x8*>(d) = h;
    *reinterpret_cast<bf16x8*>(d + 512) = l;
  }
}

// dynamic LDS of se_pool_mean's callers: mean[C] | red[TG][C], TG * C <= 4096 below C = 4096
size_t se_pool_lds(int C) { return (size_t)(C + (C >= 4096 ? C : 4096)) * sizeof(float); }

}  // namespace

extern "C" size_t ocv_channel_mean_workspace_bytes(int B, int C, long P) {
  if (B < 1 || C < 4 || P < 1) return 0;
  return (size_t)B * mean_splits(B, C, P) * C * sizeof(float);
}

extern "C" int ocv_channel_mean_nhwc_fwd(const float* x, float* out, int B, int C, long P, void* workspace,
                                         size_t workspace_bytes, ocv_stream_t stream) {
  OCV_CHECK_ARG(x && out && workspace, "ocv_channel_mean_nhwc_fwd: null pointer");
  OCV_CHECK_ARG(B >= 1 && B <= 65535 && C >= 4 && C % 4 == 0 && P >= 1, "ocv_channel_mean_nhwc_fwd: bad sizes (C must be a multiple of 4)");
  OCV_CHECK_ARG(workspace_bytes >= ocv_channel_mean_workspace_bytes(B, C, P) && ocv_aligned16(workspace) && ocv_aligned16(x),
                "ocv_channel_mean_nhwc_fwd: workspace too small or operands misaligned");
  const int splits = mean_splits(B, C, P);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(channel_sum_kernel, dim3((C + 63) / 64, splits, B), dim3(256), 0, st, x, (float*)workspace, P, C, splits);
  OCV_CHECK_LAUNCH("ocv_channel_mean_nhwc_fwd(sum)");
  const long total = (long)B * C;
  hipLaunchKernelGGL(channel_mean_finish_kernel, dim3(ocv_cdiv(total, 256)), dim3(256), 0, st, (const float*)workspace, out, C,
                     splits, 1.0f / (float)P, total);
  OCV_CHECK_LAUNCH("ocv_channel_mean_nhwc_fwd(finish)");
  return 0;
}

extern "C" int ocv_se_gate_fwd(const float* mean, const float* w1, const float* b1, const float* w2t, const float* b2,
                               float* gate, float* hidden_ws, int B, int C, int R, ocv_stream_t stream) {
  OCV_CHECK_ARG(mean && w1 && b1 && w2t && b2 && gate && hidden_ws, "ocv_se_gate_fwd: null pointer");
  OCV_CHECK_ARG(B >= 1 && B <= 65535 && C >= 1 && R >= 1 && R <= 256, "ocv_se_gate_fwd: bad sizes (R <= 256)");
  hipLaunchKernelGGL(se_hidden_kernel, dim3(ocv_cdiv(R, 4), B), dim3(256), 0, (hipStream_t)stream, mean, w1, b1, hidden_ws, C, R);
  OCV_CHECK_LAUNCH("ocv_se_gate_fwd(hidden)");
  hipLaunchKernelGGL(se_gate_hid_kernel, dim3(ocv_cdiv(C, 256), B), dim3(256), 0, (hipStream_t)stream, (const float*)hidden_ws, w2t,
                     b2, gate, C, R);
  OCV_CHECK_LAUNCH("ocv_se_gate_fwd");
  return 0;
}

extern "C" int ocv_se_gate_partials_fwd(const float* part, int tiles, long pixels_per_image, const float* w1,
                                        const float* b1, const float* w2t, const float* b2, float* gate, float* hidden_ws,
                                        int B, int C, int R, ocv_stream_t stream) {
  OCV_CHECK_ARG(part && w1 && b1 && w2t && b2 && gate && hidden_ws, "ocv_se_gate_partials_fwd: null pointer");
  OCV_CHECK_ARG(B >= 1 && B <= 65535 && C >= 1 && R >= 1 && R <= 256 && tiles >= 1 && pixels_per_image >= 1, "ocv_se_gate_partials_fwd: bad sizes (R <= 256)");
  OCV_CHECK_ARG(C <= 8192 && C % 4 == 0, "ocv_se_gate_partials_fwd: C must be a multiple of 4, at most 8192 (got %d)", C);
  hipStream_t st = (hipStream_t)stream;
  // (A/B, round 4: limits of 1824 / 76 and 3072 / 128 instead of the two below take stages 6 and 7 in -- measured SLOWER there, every workgroup of an
  //  image re-reading 0.55 / 1.5 MB of W1: bs 16 1000 -> 996 -> 994 img/s one at a time, bs 1 293 -> 286 -> 284)
  constexpr int max_c = 1536, max_r = 64;
  if (C <= max_c && R <= max_r && R <= 128) {                       // small squeeze-excite weights: ONE launch
    hipLaunchKernelGGL(se_fused_small_kernel, dim3((C + 255) / 256, B), dim3(1024), se_pool_lds(C) + 128 * sizeof(float), st, part,
                       tiles, 1.0f / (float)pixels_per_image, w1, b1, w2t, b2, gate, C, R);
    OCV_CHECK_LAUNCH("ocv_se_gate_partials_fwd(fused)");
    return 0;
  }
  hipLaunchKernelGGL(se_hidden_partials_kernel, dim3((R + 15) / 16, B), dim3(1024), se_pool_lds(C), st, part, tiles,
                     1.0f / (float)pixels_per_image, w1, b1, hidden_ws, C, R);
  OCV_CHECK_LAUNCH("ocv_se_gate_partials_fwd(hidden)");
  hipLaunchKernelGGL(se_gate_hid_kernel, dim3((C + 255) / 256, B), dim3(256), 0, st, (const float*)hidden_ws, w2t, b2, gate, C, R);
  OCV_CHECK_LAUNCH("ocv_se_gate_partials_fwd(gate)");
  return 0;
}

extern "C" int ocv_se_gate_weights_fwd(const float* part, int tiles, long pixels_per_image, const float* w1, const float* b1,
                                       const float* w2t, const float* b2, const float* W, void* w_packed, long w_image_elems,
                                       float* gate, float* hidden_ws, int B, int C, int R, int N, ocv_stream_t stream) {
  OCV_CHECK_ARG(part && w1 && b1 && w2t && b2 && W && w_packed && hidden_ws, "ocv_se_gate_weights_fwd: null pointer");
  OCV_CHECK_ARG(B >= 1 && B <= 65535 && C >= 8 && C % 8 == 0 && R >= 1 && R <= 256 && N >= 1 && tiles >= 1 && pixels_per_image >= 1,
                "ocv_se_gate_weights_fwd: bad sizes (C a multiple of 8, R <= 256)");
  OCV_CHECK_ARG(C <= 8192, "ocv_se_gate_weights_fwd: C too large (%d)", C);
  OCV_CHECK_ARG(w_image_elems >= (long)ocv_pointwise_packed_weight_elems(C, N) && (w_image_elems & 7) == 0 && ocv_aligned16(w_packed) && ocv_aligned16(W),
                "ocv_se_gate_weights_fwd: w_image_elems must hold one packed matrix (ocv_pointwise_packed_weight_elems) and keep 16-byte alignment");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(se_hidden_partials_kernel, dim3((R + 15) / 16, B), dim3(1024), se_pool_lds(C), st, part, tiles,
                     1.0f / (float)pixels_per_image, w1, b1, hidden_ws, C, R);
  OCV_CHECK_LAUNCH("ocv_se_gate_weights_fwd(hidden)");
  const int Kp = (C + 15) / 16 * 16;
  hipLaunchKernelGGL(se_gate_weights_kernel, dim3((Kp + 63) / 64, B), dim3(256), 0, st, (const float*)hidden_ws, w2t, b2, W,
                     (__bf16*)w_packed, w_image_elems, gate, C, R, N);
  OCV_CHECK_LAUNCH("ocv_se_gate_weights_fwd(gate + weights)");
  return 0;
}
