// Input end of the predict path (row N5 of DESIGN.md section 6b): decoded frames -> the tensors the model and the metric kernel read.
//   frames  uint8 [B][Hs][Ws][3] (HWC, as decoded) -> crop -> fp32 NCHW, ImageNet-normalised; optionally the batch's mirror behind it
//           modules/Preprocess.py:68-88 (/ image_norm_factor), :91-111 (KITTI benchmark crop), modules/GraphBinsLM.py:45,443 (Normalize)
//   depth   uint16 [B][Hs][Ws] (the 16-bit PNGs) -> crop -> fp32 metres = float(v) / factor                modules/Preprocess.py:45-65
// A channel value is one of 256 numbers, so the frame kernel LOOKS IT UP: the host evaluates the reference's own fp32 statement
// ((v / factor) - mean[c]) / std[c] for v = 0 .. 255 with torch CPU ops (objcavit_amd/predict.py normalisation_table) and the kernel
// holds that [3][256] table in LDS -- bit-equal to the reference arithmetic by construction, no division on the device.
// One launch each, pure streaming: 3 B read and 12 B (24 B with the mirror) written per pixel; 2 B read and 4 B written for depth.
// Pixel formats (ocv_frame_ingest_format, ocv_frames_to_rgb24; pixel_fetch.hpp): the same kernel with the pixel fetch as a template
// parameter reads bgr24 / rgba32 / bgra32 / nv12 / i420 frames (4:2:0 through Statement P, integer tables made by the host, in LDS).
#include "common.hpp"
#include "../../include/objcavit_hip.h"
#include "pixel_fetch.hpp"

namespace {

// S: pixfmt::Packed (one plane; the rgb24 entry point's arguments, in their order) or pixfmt::Planar (4:2:0 planes + the YCbCr tables)
template <class S>
struct IngestArgs {
  S s;
  const float* table;                 // [3][256]
  float* out;                         // [B][3][H][W]
  long mirror_offset;                 // elements from an image to its mirrored copy (mirror = true)
  int top, left, H, W, B;
};

// FMT: the OCV_PIXFMT_* layout the pixels are fetched from (pixel_fetch.hpp); rgb24 is the instantiation ocv_frame_ingest_fwd launches.
// VEC: a thread takes 4 consecutive pixels of a row (W % 4 == 0, out 16-byte aligned): 12 bytes in, one 16-byte store per channel
// plane, and the same 16 bytes reversed at the mirrored columns W-4-x .. W-1-x.  !VEC: one pixel per thread, scalar stores (odd W).
// 4:2:0: the five int32 tables of Statement P sit in LDS beside the normalisation table; a thread's 4 pixels start at a source column
// of any parity and fetch and look up each of their 2 or 3 chroma samples once.
template <int FMT, bool VEC, bool MIRROR>
__global__ __launch_bounds__(256) void frame_ingest_kernel(IngestArgs<typename pixfmt::Source<FMT>::type> p) {
  __shared__ float tab[3 * 256];
  for (int i = threadIdx.x; i < 3 * 256; i += 256) tab[i] = p.table[i];
  const int* yt = nullptr;
  if constexpr (pixfmt::is_yuv(FMT)) {
    __shared__ int ytab[pixfmt::YUV_TABLE_WORDS];
    for (int i = threadIdx.x; i < pixfmt::YUV_TABLE_WORDS; i += 256) ytab[i] = p.s.yuv[i];
    yt = ytab;
  }
  __syncthreads();
  const long plane = (long)p.H * p.W;
  if constexpr (VEC) {
    const int G = p.W >> 2;
    const long total = (long)p.B * p.H * G;
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
      const int g = (int)(t % G);
      const long r = t / G;
      const int y = (int)(r % p.H), b = (int)(r / p.H), x = g << 2;
      uint8_t px[12];
      if constexpr (FMT == OCV_PIXFMT_RGB24) {
        const uint8_t* s = p.s.src + b * p.s.frame_stride + (long)(p.top + y) * p.s.row_stride + (long)(p.left + x) * 3;
        __builtin_memcpy(px, s, 12);                             // (any alignment: the crop origin and the row stride are the caller's)
      } else {
        pixfmt::fetch4<FMT>(p.s, yt, b, p.top + y, p.left + x, px);
      }
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
      uint8_t rgb[3];
      const uint8_t* s = rgb;
      if constexpr (FMT == OCV_PIXFMT_RGB24)
        s = p.s.src + b * p.s.frame_stride + (long)(p.top + y) * p.s.row_stride + (long)(p.left + x) * 3;
      else
        pixfmt::fetch1<FMT>(p.s, yt, b, p.top + y, p.left + x, rgb);
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

// The Hw x Ww window of frames of any format as packed RGB24 [B][Hw][Ww][3].  VEC (Ww % 4 == 0, out 4-byte aligned): a thread takes 4
// pixels and stores their 12 bytes as three dwords; else one pixel and three byte stores per thread.  Every output byte is written.
struct ToRgbOut {
  uint8_t* out;
  int top, left, H, W, B;
};

template <int FMT, bool VEC>
__global__ __launch_bounds__(256) void frames_to_rgb24_kernel(typename pixfmt::Source<FMT>::type s, ToRgbOut p) {
  const int* yt = nullptr;
  if constexpr (pixfmt::is_yuv(FMT)) {
    __shared__ int ytab[pixfmt::YUV_TABLE_WORDS];
    for (int i = threadIdx.x; i < pixfmt::YUV_TABLE_WORDS; i += 256) ytab[i] = s.yuv[i];
    yt = ytab;
    __syncthreads();
  }
  if constexpr (VEC) {
    const int G = p.W >> 2;
    const long total = (long)p.B * p.H * G;
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
      const int g = (int)(t % G);
      const long r = t / G;
      const int y = (int)(r % p.H), b = (int)(r / p.H), x = g << 2;
      uint8_t px[12];
      pixfmt::fetch4<FMT>(s, yt, b, p.top + y, p.left + x, px);
      uint32_t w[3];
      __builtin_memcpy(w, px, 12);
      uint32_t* o = reinterpret_cast<uint32_t*>(p.out + ((long)b * p.H + y) * p.W * 3 + (long)x * 3);     // (W % 4 == 0: a multiple of 4 bytes)
      o[0] = w[0];
      o[1] = w[1];
      o[2] = w[2];
    }
  } else {
    const long total = (long)p.B * p.H * p.W;
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
      const int x = (int)(t % p.W);
      const long r = t / p.W;
      const int y = (int)(r % p.H), b = (int)(r / p.H);
      uint8_t rgb[3];
      pixfmt::fetch1<FMT>(s, yt, b, p.top + y, p.left + x, rgb);
      uint8_t* o = p.out + t * 3;
      o[0] = rgb[0];
      o[1] = rgb[1];
      o[2] = rgb[2];
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
  IngestArgs<pixfmt::Packed> a{{frames, frame_stride, row_stride}, table, out, mirror_offset, top, left, H, W, B};
  const bool vec = (W & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0 && (!mirror_too || (mirror_offset & 3) == 0);
  hipStream_t st = (hipStream_t)stream;
  const int grid = stream_grid(vec ? (long)B * H * (W >> 2) : (long)B * H * W);
  if (vec && mirror_too) hipLaunchKernelGGL((frame_ingest_kernel<OCV_PIXFMT_RGB24, true, true>), dim3(grid), dim3(256), 0, st, a);
  else if (vec) hipLaunchKernelGGL((frame_ingest_kernel<OCV_PIXFMT_RGB24, true, false>), dim3(grid), dim3(256), 0, st, a);
  else if (mirror_too) hipLaunchKernelGGL((frame_ingest_kernel<OCV_PIXFMT_RGB24, false, true>), dim3(grid), dim3(256), 0, st, a);
  else hipLaunchKernelGGL((frame_ingest_kernel<OCV_PIXFMT_RGB24, false, false>), dim3(grid), dim3(256), 0, st, a);
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

namespace {

template <int FMT>
auto source_of(const pixfmt::Planes& pl, const int* yuv) {
  if constexpr (pixfmt::is_yuv(FMT)) return pixfmt::planar_of(pl, yuv);
  else return pixfmt::packed_of(pl);
}

template <int FMT>
void launch_ingest(const pixfmt::Planes& pl, const int* yuv, const float* table, float* out, long mirror_offset, int top, int left, int H,
                   int W, int B, bool vec, bool mirror, hipStream_t st) {
  IngestArgs<typename pixfmt::Source<FMT>::type> a{source_of<FMT>(pl, yuv), table, out, mirror_offset, top, left, H, W, B};
  const int grid = stream_grid(vec ? (long)B * H * (W >> 2) : (long)B * H * W);
  if (vec && mirror) hipLaunchKernelGGL((frame_ingest_kernel<FMT, true, true>), dim3(grid), dim3(256), 0, st, a);
  else if (vec) hipLaunchKernelGGL((frame_ingest_kernel<FMT, true, false>), dim3(grid), dim3(256), 0, st, a);
  else if (mirror) hipLaunchKernelGGL((frame_ingest_kernel<FMT, false, true>), dim3(grid), dim3(256), 0, st, a);
  else hipLaunchKernelGGL((frame_ingest_kernel<FMT, false, false>), dim3(grid), dim3(256), 0, st, a);
}

template <int FMT>
void launch_to_rgb(const pixfmt::Planes& pl, const int* yuv, uint8_t* out, int top, int left, int H, int W, int B, bool vec, hipStream_t st) {
  ToRgbOut a{out, top, left, H, W, B};
  const int grid = stream_grid(vec ? (long)B * H * (W >> 2) : (long)B * H * W);
  if (vec) hipLaunchKernelGGL((frames_to_rgb24_kernel<FMT, true>), dim3(grid), dim3(256), 0, st, source_of<FMT>(pl, yuv), a);
  else hipLaunchKernelGGL((frames_to_rgb24_kernel<FMT, false>), dim3(grid), dim3(256), 0, st, source_of<FMT>(pl, yuv), a);
}

}  // namespace

#define OCV_PIXFMT_DISPATCH(format, CALL)                        \
  switch (format) {                                              \
    case OCV_PIXFMT_RGB24: CALL(OCV_PIXFMT_RGB24); break;        \
    case OCV_PIXFMT_BGR24: CALL(OCV_PIXFMT_BGR24); break;        \
    case OCV_PIXFMT_RGBA32: CALL(OCV_PIXFMT_RGBA32); break;      \
    case OCV_PIXFMT_BGRA32: CALL(OCV_PIXFMT_BGRA32); break;      \
    case OCV_PIXFMT_NV12: CALL(OCV_PIXFMT_NV12); break;          \
    default: CALL(OCV_PIXFMT_I420); break;                       \
  }

extern "C" int ocv_frame_ingest_format(int format, const uint8_t* plane0, long frame_stride0, long row_stride0, const uint8_t* plane1,
                                       long frame_stride1, long row_stride1, const uint8_t* plane2, long frame_stride2, long row_stride2,
                                       const int* yuv_table, int Hs, int Ws, int top, int left, const float* table, float* out, int B,
                                       int H, int W, int mirror_too, long mirror_offset, ocv_stream_t stream) {
  const pixfmt::Planes pl{{plane0, plane1, plane2}, {frame_stride0, frame_stride1, frame_stride2}, {row_stride0, row_stride1, row_stride2}};
  OCV_CHECK_ARG(table && out, "ocv_frame_ingest_format: null pointer (table / out)");
  OCV_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && Hs >= 1 && Ws >= 1, "ocv_frame_ingest_format: bad sizes (B, H, W, Hs, Ws must be >= 1)");
  if (pixfmt::check_source("ocv_frame_ingest_format", format, pl, yuv_table, B, Hs, Ws)) return -1;
  OCV_CHECK_ARG(top >= 0 && left >= 0 && (long)top + H <= Hs && (long)left + W <= Ws, "ocv_frame_ingest_format: crop window outside the frame");
  OCV_CHECK_ARG((reinterpret_cast<uintptr_t>(out) & 3) == 0 && (reinterpret_cast<uintptr_t>(table) & 3) == 0,
                "ocv_frame_ingest_format: out / table must be 4-byte aligned");
  OCV_CHECK_ARG(!mirror_too || mirror_offset >= (long)B * 3 * H * W || mirror_offset <= -(long)B * 3 * H * W,
                "ocv_frame_ingest_format: the mirrored half overlaps the batch (mirror_offset is in elements, |offset| >= B * 3 * H * W)");
  const bool vec = (W & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0 && (!mirror_too || (mirror_offset & 3) == 0);
  hipStream_t st = (hipStream_t)stream;
#define OCV_CALL(F) launch_ingest<F>(pl, yuv_table, table, out, mirror_offset, top, left, H, W, B, vec, mirror_too != 0, st)
  OCV_PIXFMT_DISPATCH(format, OCV_CALL)
#undef OCV_CALL
  OCV_CHECK_LAUNCH("ocv_frame_ingest_format");
  return 0;
}

extern "C" int ocv_frames_to_rgb24(int format, const uint8_t* plane0, long frame_stride0, long row_stride0, const uint8_t* plane1,
                                   long frame_stride1, long row_stride1, const uint8_t* plane2, long frame_stride2, long row_stride2,
                                   const int* yuv_table, int Hs, int Ws, int top, int left, uint8_t* out, int B, int Hw, int Ww,
                                   ocv_stream_t stream) {
  const pixfmt::Planes pl{{plane0, plane1, plane2}, {frame_stride0, frame_stride1, frame_stride2}, {row_stride0, row_stride1, row_stride2}};
  OCV_CHECK_ARG(out, "ocv_frames_to_rgb24: null pointer (out)");
  OCV_CHECK_ARG(B >= 1 && Hw >= 1 && Ww >= 1 && Hs >= 1 && Ws >= 1, "ocv_frames_to_rgb24: bad sizes (B, Hw, Ww, Hs, Ws must be >= 1)");
  if (pixfmt::check_source("ocv_frames_to_rgb24", format, pl, yuv_table, B, Hs, Ws)) return -1;
  OCV_CHECK_ARG(top >= 0 && left >= 0 && (long)top + Hw <= Hs && (long)left + Ww <= Ws, "ocv_frames_to_rgb24: window outside the frame");
  const bool vec = (Ww & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0;
  hipStream_t st = (hipStream_t)stream;
#define OCV_CALL(F) launch_to_rgb<F>(pl, yuv_table, out, top, left, Hw, Ww, B, vec, st)
  OCV_PIXFMT_DISPATCH(format, OCV_CALL)
#undef OCV_CALL
  OCV_CHECK_LAUNCH("ocv_frames_to_rgb24");
  return 0;
}
