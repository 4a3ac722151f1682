// Input end of the predict path (row N5 of DESIGN.md section 6b): decoded frames -> the tensors the model and the metric kernel read.
//   frames  uint8 [B][Hs][Ws][3] (HWC, as decoded) -> crop -> fp32 NCHW, ImageNet-normalised; optionally the batch's mirror behind it
//           modules/Preprocess.py:68-88 (/ image_norm_factor), :91-111 (KITTI benchmark crop), modules/GraphBinsLM.py:45,443 (Normalize)
//   depth   uint16 [B][Hs][Ws] (the 16-bit PNGs) -> crop -> fp32 metres = float(v) / factor                modules/Preprocess.py:45-65
// A channel value is one of 256 numbers, so the frame kernel LOOKS IT UP: the host evaluates the reference's own fp32 statement
// ((v / factor) - mean[c]) / std[c] for v = 0 .. 255 with torch CPU ops (objcavit_amd/predict.py normalisation_table) and the kernel
// holds that [3][256] table in LDS -- bit-equal to the reference arithmetic by construction, no division on the device.
// One launch each, pure streaming: 3 B read and 12 B (24 B with the mirror) written per pixel; 2 B read and 4 B written for depth.
#include "common.hpp"
#include "../../include/objcavit_hip.h"

namespace {

struct IngestArgs {
  const uint8_t* src;
  long frame_stride, row_stride;      // bytes
  const float* table;                 // [3][256]
  float* out;                         // [B][3][H][W]
  long mirror_offset;                 // elements from an image to its mirrored copy (mirror = true)
  int top, left, H, W, B;
};

// VEC: a thread takes 4 consecutive pixels of a row (W % 4 == 0, out 16-byte aligned): 12 bytes in, one 16-byte store per channel
// plane, and the same 16 bytes reversed at the mirrored columns W-4-x .. W-1-x.  !VEC: one pixel per thread, scalar stores (odd W).
template <bool VEC, bool MIRROR>
__global__ __launch_bounds__(256) void frame_ingest_kernel(IngestArgs p) {
  __shared__ float tab[3 * 256];
  for (int i = threadIdx.x; i < 3 * 256; i += 256) tab[i] = p.table[i];
  __syncthreads();
  const long plane = (long)p.H * p.W;
  if constexpr (VEC) {
    const int G = p.W >> 2;
    const long total = (long)p.B * p.H * G;
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
      const int g = (int)(t % G);
      const long r = t / G;
      const int y = (int)(r % p.H), b = (int)(r / p.H), x = g << 2;
      const uint8_t* s = p.src + b * p.frame_stride + (long)(p.top + y) * p.row_stride + (long)(p.left + x) * 3;
      uint8_t px[12];
      __builtin_memcpy(px, s, 12);                               // (any alignment: the crop origin and the row stride are the caller's)
      float* o = p.out + (long)b * 3 * plane + (long)y * p.W + x;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float4 v = make_float4(tab[c * 256 + px[c]], tab[c * 256 + px[3 + c]], tab[c * 256 + px[6 + c]], tab[c * 256 + px[9 + c]]);
        *reinterpret_cast<float4*>(o + c * plane) = v;
        if constexpr (MIRROR)
          *reinterpret_cast<float4*>(o + p.mirror_offset + c * plane - x + (p.W - 4 - x)) = make_float4(v.w, v.z, v.y, v.x);
      }
    }
  } else {
    const long total = (long)p.B * plane;
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
      const int x = (int)(t % p.W);
      const long r = t / p.W;
      const int y = (int)(r % p.H), b = (int)(r / p.H);
      const uint8_t* s = p.src + b * p.frame_stride + (long)(p.top + y) * p.row_stride + (long)(p.left + x) * 3;
      float* o = p.out + (long)b * 3 * plane + (long)y * p.W;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float v = tab[c * 256 + s[c]];
        o[c * plane + x] = v;
        if constexpr (MIRROR) o[p.mirror_offset + c * plane + (p.W - 1 - x)] = v;
      }
    }
  }
}

struct DepthIngestArgs {
  const uint16_t* src;
  long frame_stride, row_stride;      // elements
  float* out;                         // [B][1][H][W]
  int top, left, H, W, B;
  float factor;
};

// float(v) / factor with IEEE division (the library is built without fast-math: `/` is correctly rounded, which is what torch's
// fp32 division gives; tests/test_hip_predict.py checks all 65536 values for both dataset factors)
template <bool VEC>
__global__ __launch_bounds__(256) void depth_ingest_kernel(DepthIngestArgs p) {
  const long plane = (long)p.H * p.W;
  if constexpr (VEC) {
    const int G = p.W >> 2;
    const long total = (long)p.B * p.H * G;
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
      const int g = (int)(t % G);
      const long r = t / G;
      const int y = (int)(r % p.H), b = (int)(r / p.H), x = g << 2;
      const uint16_t* s = p.src + b * p.frame_stride + (long)(p.top + y) * p.row_stride + (p.left + x);
      uint16_t v[4];
      __builtin_memcpy(v, s, 8);
      *reinterpret_cast<float4*>(p.out + b * plane + (long)y * p.W + x) =
          make_float4((float)v[0] / p.factor, (float)v[1] / p.factor, (float)v[2] / p.factor, (float)v[3] / p.factor);
    }
  } else {
    const long total = (long)p.B * plane;
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
      const int x = (int)(t % p.W);
      const long r = t / p.W;
      const int y = (int)(r % p.H), b = (int)(r / p.H);
      p.out[t] = (float)p.src[b * p.frame_stride + (long)(p.top + y) * p.row_stride + (p.left + x)] / p.factor;
    }
  }
}

int stream_grid(long threads) {
  long g = (threads + 255) / 256;
  if (g > 4096) g = 4096;              // 16 workgroups per CU: the rest of the work comes round in the grid-stride loop
  return (int)(g < 1 ? 1 : g);
}

}  // namespace

extern "C" int ocv_frame_ingest_fwd(const uint8_t* frames, long frame_stride, long row_stride, int Hs, int Ws, int top, int left,
                                    const float* table, float* out, int B, int H, int W, int mirror_too, long mirror_offset,
                                    ocv_stream_t stream) {
  OCV_CHECK_ARG(frames && table && out, "ocv_frame_ingest_fwd: null pointer");
  OCV_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && Hs >= 1 && Ws >= 1, "ocv_frame_ingest_fwd: bad sizes (B, H, W, Hs, Ws must be >= 1)");
  OCV_CHECK_ARG(top >= 0 && left >= 0 && (long)top + H <= Hs && (long)left + W <= Ws, "ocv_frame_ingest_fwd: crop window outside the frame");
  OCV_CHECK_ARG(row_stride >= (long)Ws * 3 && (B == 1 || frame_stride >= (long)(Hs - 1) * row_stride + (long)Ws * 3),
                "ocv_frame_ingest_fwd: strides (bytes) smaller than a row / a frame");
  OCV_CHECK_ARG((reinterpret_cast<uintptr_t>(out) & 3) == 0 && (reinterpret_cast<uintptr_t>(table) & 3) == 0,
                "ocv_frame_ingest_fwd: out / table must be 4-byte aligned");
  OCV_CHECK_ARG(!mirror_too || mirror_offset >= (long)B * 3 * H * W || mirror_offset <= -(long)B * 3 * H * W,
                "ocv_frame_ingest_fwd: the mirrored half overlaps the batch (mirror_offset is in elements, |offset| >= B * 3 * H * W)");
  IngestArgs a{frames, frame_stride, row_stride, table, out, mirror_offset, top, left, H, W, B};
  const bool vec = (W & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0 && (!mirror_too || (mirror_offset & 3) == 0);
  hipStream_t st = (hipStream_t)stream;
  const int grid = stream_grid(vec ? (long)B * H * (W >> 2) : (long)B * H * W);
  if (vec && mirror_too) hipLaunchKernelGGL((frame_ingest_kernel<true, true>), dim3(grid), dim3(256), 0, st, a);
  else if (vec) hipLaunchKernelGGL((frame_ingest_kernel<true, false>), dim3(grid), dim3(256), 0, st, a);
  else if (mirror_too) hipLaunchKernelGGL((frame_ingest_kernel<false, true>), dim3(grid), dim3(256), 0, st, a);
  else hipLaunchKernelGGL((frame_ingest_kernel<false, false>), dim3(grid), dim3(256), 0, st, a);
  OCV_CHECK_LAUNCH("ocv_frame_ingest_fwd");
  return 0;
}

extern "C" int ocv_depth_ingest_fwd(const uint16_t* depth, long frame_stride, long row_stride, int Hs, int Ws, int top, int left,
                                    float factor, float* out, int B, int H, int W, ocv_stream_t stream) {
  OCV_CHECK_ARG(depth && out, "ocv_depth_ingest_fwd: null pointer");
  OCV_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && Hs >= 1 && Ws >= 1, "ocv_depth_ingest_fwd: bad sizes (B, H, W, Hs, Ws must be >= 1)");
  OCV_CHECK_ARG(top >= 0 && left >= 0 && (long)top + H <= Hs && (long)left + W <= Ws, "ocv_depth_ingest_fwd: crop window outside the frame");
  OCV_CHECK_ARG(row_stride >= Ws && (B == 1 || frame_stride >= (long)(Hs - 1) * row_stride + Ws),
                "ocv_depth_ingest_fwd: strides (elements) smaller than a row / a frame");
  OCV_CHECK_ARG(factor > 0.f, "ocv_depth_ingest_fwd: factor must be positive");
  OCV_CHECK_ARG((reinterpret_cast<uintptr_t>(depth) & 1) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0,
                "ocv_depth_ingest_fwd: misaligned pointer");
  DepthIngestArgs a{depth, frame_stride, row_stride, out, top, left, H, W, B, factor};
  const bool vec = (W & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  hipStream_t st = (hipStream_t)stream;
  const int grid = stream_grid(vec ? (long)B * H * (W >> 2) : (long)B * H * W);
  if (vec) hipLaunchKernelGGL(depth_ingest_kernel<true>, dim3(grid), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(depth_ingest_kernel<false>, dim3(grid), dim3(256), 0, st, a);
  OCV_CHECK_LAUNCH("ocv_depth_ingest_fwd");
  return 0;
}
