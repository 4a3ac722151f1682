// Lens on ingest ("Lens on ingest"; Statement L in include/objcavit_hip.h): the rectified window of a distorted
// frame, straight to what frame_ingest.hip writes.  The HOST decides the geometry: objcavit_amd/lens.py evaluates the lens model in
// float64 and quantises the source coordinate of every rectified pixel to 1/256 pixel (int32 [M][Hw][Ww][2], M = 1 or B).  The kernel is
// a bilinear gather in INTEGER arithmetic through the pixel fetch of any OCV_PIXFMT_* layout (pixel_fetch.hpp): four taps, each inside the
// frame or black, 8-bit weights, one rounding -- every byte is decided by the statement, so the tests ask for equal bytes.
//   ocv_frame_remap_ingest_fwd   map -> table[c][byte] as fp32 NCHW, optionally the mirrored batch behind it (ocv_frame_ingest_fwd's out)
//   ocv_frames_remap_rgb24_fwd   map -> the rectified window as packed RGB24 [B][Hw][Ww][3]
// Shaped as the ingest kernel: VEC = a thread owns 4 consecutive output pixels of a row (its 8 map words are two 16-byte loads, one
// float4 store per channel plane and the reversed float4 at the mirrored columns), a scalar form for every other width; the
// normalisation table and the YCbCr tables sit in LDS.  The two taps of a source row are fetched together: 2 x bytes-per-pixel contiguous
// bytes for the packed formats, two luma bytes and one chroma sample (two when x0 is odd) for 4:2:0.  Lens maps are smooth: neighbouring
// threads read neighbouring source pixels and the gather is served by L1 / L2; nothing is staged through LDS.
#include "common.hpp"
#include "../../include/objcavit_hip.h"
#include "pixel_fetch.hpp"

namespace {

template <class S>
struct RemapSource {
  S s;
  const int* map;                     // [M][H][W][2]: X, Y in 1/256 source pixel
  long map_image;                     // words from an image's map to the next one's: 0 (M = 1) or H * W * 2 (M = B)
  int Hs, Ws, H, W, B;
};

struct RGB {
  int r, g, b;
};

// the taps (x0, y) and (x0 + 1, y) of image b, y inside the frame; a tap outside 0 <= x < Ws is black
template <int FMT>
__device__ inline void row_taps(const typename pixfmt::Source<FMT>::type& s, const int* yt, int b, int y, int x0, int Ws, uint8_t* p0,
                                uint8_t* p1) {
  const bool in0 = (unsigned)x0 < (unsigned)Ws, in1 = (unsigned)(x0 + 1) < (unsigned)Ws;
  p0[0] = p0[1] = p0[2] = p1[0] = p1[1] = p1[2] = 0;
  if (in0 && in1) {
    if constexpr (pixfmt::is_yuv(FMT)) {
      uint8_t l[2];
      __builtin_memcpy(l, s.src + b * s.frame_stride + (long)y * s.row_stride + x0, 2);
      const pixfmt::ChromaTerms t0 = pixfmt::chroma_at<FMT>(s, yt, b, y >> 1, x0 >> 1);
      pixfmt::yuv_pixel(yt, l[0], t0, p0);
      if (x0 & 1) pixfmt::yuv_pixel(yt, l[1], pixfmt::chroma_at<FMT>(s, yt, b, y >> 1, (x0 >> 1) + 1), p1);
      else pixfmt::yuv_pixel(yt, l[1], t0, p1);
    } else {
      constexpr int BPP = pixfmt::packed_bytes(FMT);
      uint8_t q[2 * BPP];
      __builtin_memcpy(q, s.src + b * s.frame_stride + (long)y * s.row_stride + (long)x0 * BPP, 2 * BPP);
      p0[0] = q[pixfmt::is_bgr(FMT) ? 2 : 0];
      p0[1] = q[1];
      p0[2] = q[pixfmt::is_bgr(FMT) ? 0 : 2];
      p1[0] = q[BPP + (pixfmt::is_bgr(FMT) ? 2 : 0)];
      p1[1] = q[BPP + 1];
      p1[2] = q[BPP + (pixfmt::is_bgr(FMT) ? 0 : 2)];
    }
  } else if (in0) {
    pixfmt::fetch1<FMT>(s, yt, b, y, x0, p0);
  } else if (in1) {
    pixfmt::fetch1<FMT>(s, yt, b, y, x0 + 1, p1);
  }
}

// Statement L for one output pixel: (X, Y) -> the three bytes.  Any int32 X, Y is safe: a tap is read only after the unsigned range test.
template <int FMT>
__device__ inline void remap_pixel(const typename pixfmt::Source<FMT>::type& s, const int* yt, int b, int X, int Y, int Hs, int Ws,
                                   uint8_t* rgb) {
  const int x0 = X >> 8, wx = X & 255, y0 = Y >> 8, wy = Y & 255;
  int acc[3] = {32768, 32768, 32768};
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int y = y0 + j;
    if ((unsigned)y >= (unsigned)Hs) continue;
    uint8_t p0[3], p1[3];
    row_taps<FMT>(s, yt, b, y, x0, Ws, p0, p1);
    const int wr = j ? wy : 256 - wy;
    const int w0 = (256 - wx) * wr, w1 = wx * wr;
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] += w0 * p0[c] + w1 * p1[c];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) rgb[c] = (uint8_t)(acc[c] >> 16);          // acc <= 255 * 65536 + 32768: no clamp is needed
}

template <class S>
struct RemapIngestArgs {
  RemapSource<S> r;
  const float* table;                 // [3][256]
  float* out;                         // [B][3][H][W]
  long mirror_offset;                 // elements from an image to its mirrored copy
};

template <int FMT, bool VEC, bool MIRROR>
__global__ __launch_bounds__(256) void frame_remap_ingest_kernel(RemapIngestArgs<typename pixfmt::Source<FMT>::type> p) {
  __shared__ float tab[3 * 256];
  for (int i = threadIdx.x; i < 3 * 256; i += 256) tab[i] = p.table[i];
  const int* yt = nullptr;
  if constexpr (pixfmt::is_yuv(FMT)) {
    __shared__ int ytab[pixfmt::YUV_TABLE_WORDS];
    for (int i = threadIdx.x; i < pixfmt::YUV_TABLE_WORDS; i += 256) ytab[i] = p.r.s.yuv[i];
    yt = ytab;
  }
  __syncthreads();
  const int H = p.r.H, W = p.r.W;
  const long plane = (long)H * W;
  if constexpr (VEC) {
    const int G = W >> 2;
    const long total = (long)p.r.B * H * G;
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
      const int g = (int)(t % G);
      const long r = t / G;
      const int y = (int)(r % H), b = (int)(r / H), x = g << 2;
      const int4* m = reinterpret_cast<const int4*>(p.r.map + b * p.r.map_image + ((long)y * W + x) * 2);      // (W % 4 == 0: 32-byte steps)
      const int4 m0 = m[0], m1 = m[1];
      uint8_t px[12];
      remap_pixel<FMT>(p.r.s, yt, b, m0.x, m0.y, p.r.Hs, p.r.Ws, px);
      remap_pixel<FMT>(p.r.s, yt, b, m0.z, m0.w, p.r.Hs, p.r.Ws, px + 3);
      remap_pixel<FMT>(p.r.s, yt, b, m1.x, m1.y, p.r.Hs, p.r.Ws, px + 6);
      remap_pixel<FMT>(p.r.s, yt, b, m1.z, m1.w, p.r.Hs, p.r.Ws, px + 9);
      float* o = p.out + (long)b * 3 * plane + (long)y * W + x;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float4 v = make_float4(tab[c * 256 + px[c]], tab[c * 256 + px[3 + c]], tab[c * 256 + px[6 + c]], tab[c * 256 + px[9 + c]]);
        *reinterpret_cast<float4*>(o + c * plane) = v;
        if constexpr (MIRROR)
          *reinterpret_cast<float4*>(o + p.mirror_offset + c * plane - x + (W - 4 - x)) = make_float4(v.w, v.z, v.y, v.x);
      }
    }
  } else {
    const long total = (long)p.r.B * plane;
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
      const int x = (int)(t % W);
      const long r = t / W;
      const int y = (int)(r % H), b = (int)(r / H);
      const int* m = p.r.map + b * p.r.map_image + ((long)y * W + x) * 2;
      uint8_t rgb[3];
      remap_pixel<FMT>(p.r.s, yt, b, m[0], m[1], p.r.Hs, p.r.Ws, rgb);
      float* o = p.out + (long)b * 3 * plane + (long)y * W;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float v = tab[c * 256 + rgb[c]];
        o[c * plane + x] = v;
        if constexpr (MIRROR) o[p.mirror_offset + c * plane + (W - 1 - x)] = v;
      }
    }
  }
}

// VEC (W % 4 == 0, out 4-byte aligned): a thread takes 4 pixels and stores their 12 bytes as three dwords; else one pixel, three bytes.
template <int FMT, bool VEC>
__global__ __launch_bounds__(256) void frames_remap_rgb24_kernel(RemapSource<typename pixfmt::Source<FMT>::type> p, uint8_t* out) {
  const int* yt = nullptr;
  if constexpr (pixfmt::is_yuv(FMT)) {
    __shared__ int ytab[pixfmt::YUV_TABLE_WORDS];
    for (int i = threadIdx.x; i < pixfmt::YUV_TABLE_WORDS; i += 256) ytab[i] = p.s.yuv[i];
    yt = ytab;
    __syncthreads();
  }
  const int H = p.H, W = p.W;
  if constexpr (VEC) {
    const int G = W >> 2;
    const long total = (long)p.B * H * G;
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
      const int g = (int)(t % G);
      const long r = t / G;
      const int y = (int)(r % H), b = (int)(r / H), x = g << 2;
      const int4* m = reinterpret_cast<const int4*>(p.map + b * p.map_image + ((long)y * W + x) * 2);
      const int4 m0 = m[0], m1 = m[1];
      uint8_t px[12];
      remap_pixel<FMT>(p.s, yt, b, m0.x, m0.y, p.Hs, p.Ws, px);
      remap_pixel<FMT>(p.s, yt, b, m0.z, m0.w, p.Hs, p.Ws, px + 3);
      remap_pixel<FMT>(p.s, yt, b, m1.x, m1.y, p.Hs, p.Ws, px + 6);
      remap_pixel<FMT>(p.s, yt, b, m1.z, m1.w, p.Hs, p.Ws, px + 9);
      uint32_t w[3];
      __builtin_memcpy(w, px, 12);
      uint32_t* o = reinterpret_cast<uint32_t*>(out + ((long)b * H + y) * W * 3 + (long)x * 3);      // (W % 4 == 0: a multiple of 4 bytes)
      o[0] = w[0];
      o[1] = w[1];
      o[2] = w[2];
    }
  } else {
    const long total = (long)p.B * H * W;
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
      const int x = (int)(t % W);
      const long r = t / W;
      const int y = (int)(r % H), b = (int)(r / H);
      const int* m = p.map + b * p.map_image + ((long)y * W + x) * 2;
      uint8_t rgb[3];
      remap_pixel<FMT>(p.s, yt, b, m[0], m[1], p.Hs, p.Ws, rgb);
      uint8_t* o = out + t * 3;
      o[0] = rgb[0];
      o[1] = rgb[1];
      o[2] = rgb[2];
    }
  }
}

int stream_grid(long threads) {
  long g = (threads + 255) / 256;
  if (g > 4096) g = 4096;              // 16 workgroups per CU: the rest of the work comes round in the grid-stride loop
  return (int)(g < 1 ? 1 : g);
}

template <int FMT>
RemapSource<typename pixfmt::Source<FMT>::type> source_of(const pixfmt::Planes& pl, const int* yuv, const int* map, int M, int Hs, int Ws,
                                                          int H, int W, int B) {
  const long step = M == 1 ? 0 : (long)H * W * 2;
  if constexpr (pixfmt::is_yuv(FMT)) return {pixfmt::planar_of(pl, yuv), map, step, Hs, Ws, H, W, B};
  else return {pixfmt::packed_of(pl), map, step, Hs, Ws, H, W, B};
}

template <int FMT>
void launch_remap_ingest(const pixfmt::Planes& pl, const int* yuv, const int* map, int M, int Hs, int Ws, const float* table, float* out,
                         long mirror_offset, int H, int W, int B, bool vec, bool mirror, hipStream_t st) {
  RemapIngestArgs<typename pixfmt::Source<FMT>::type> a{source_of<FMT>(pl, yuv, map, M, Hs, Ws, H, W, B), table, out, mirror_offset};
  const int grid = stream_grid(vec ? (long)B * H * (W >> 2) : (long)B * H * W);
  if (vec && mirror) hipLaunchKernelGGL((frame_remap_ingest_kernel<FMT, true, true>), dim3(grid), dim3(256), 0, st, a);
  else if (vec) hipLaunchKernelGGL((frame_remap_ingest_kernel<FMT, true, false>), dim3(grid), dim3(256), 0, st, a);
  else if (mirror) hipLaunchKernelGGL((frame_remap_ingest_kernel<FMT, false, true>), dim3(grid), dim3(256), 0, st, a);
  else hipLaunchKernelGGL((frame_remap_ingest_kernel<FMT, false, false>), dim3(grid), dim3(256), 0, st, a);
}

template <int FMT>
void launch_remap_rgb(const pixfmt::Planes& pl, const int* yuv, const int* map, int M, int Hs, int Ws, uint8_t* out, int H, int W, int B,
                      bool vec, hipStream_t st) {
  const auto a = source_of<FMT>(pl, yuv, map, M, Hs, Ws, H, W, B);
  const int grid = stream_grid(vec ? (long)B * H * (W >> 2) : (long)B * H * W);
  if (vec) hipLaunchKernelGGL((frames_remap_rgb24_kernel<FMT, true>), dim3(grid), dim3(256), 0, st, a, out);
  else hipLaunchKernelGGL((frames_remap_rgb24_kernel<FMT, false>), dim3(grid), dim3(256), 0, st, a, out);
}

// what both entry points ask of the map and the window; 0, or -1 with the message set
int check_map(const char* who, const int* map, int M, int B, int Hw, int Ww) {
  OCV_CHECK_ARG(map != nullptr, "%s: null pointer (map)", who);
  OCV_CHECK_ARG(Hw >= 1 && Ww >= 1, "%s: bad sizes (Hw, Ww must be >= 1)", who);
  OCV_CHECK_ARG((reinterpret_cast<uintptr_t>(map) & 15) == 0, "%s: map (int32 [M][Hw][Ww][2]) must be 16-byte aligned", who);
  OCV_CHECK_ARG(M == 1 || M == B, "%s: M = %d maps for B = %d images (one map for the batch, M = 1, or one per image, M = B)", who, M, B);
  return 0;
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

extern "C" int ocv_frame_remap_ingest_fwd(int format, const uint8_t* plane0, long frame_stride0, long row_stride0, const uint8_t* plane1,
                                          long frame_stride1, long row_stride1, const uint8_t* plane2, long frame_stride2,
                                          long row_stride2, const int* yuv_table, int Hs, int Ws, const int* map, int M, int Hw, int Ww,
                                          const float* table, float* out, int B, int mirror_too, long mirror_offset, ocv_stream_t stream) {
  const pixfmt::Planes pl{{plane0, plane1, plane2}, {frame_stride0, frame_stride1, frame_stride2}, {row_stride0, row_stride1, row_stride2}};
  OCV_CHECK_ARG(table && out, "ocv_frame_remap_ingest_fwd: null pointer (table / out)");
  if (pixfmt::check_source("ocv_frame_remap_ingest_fwd", format, pl, yuv_table, B, Hs, Ws)) return -1;
  if (check_map("ocv_frame_remap_ingest_fwd", map, M, B, Hw, Ww)) return -1;
  OCV_CHECK_ARG((reinterpret_cast<uintptr_t>(out) & 3) == 0 && (reinterpret_cast<uintptr_t>(table) & 3) == 0,
                "ocv_frame_remap_ingest_fwd: out / table must be 4-byte aligned");
  OCV_CHECK_ARG(!mirror_too || mirror_offset >= (long)B * 3 * Hw * Ww || mirror_offset <= -(long)B * 3 * Hw * Ww,
                "ocv_frame_remap_ingest_fwd: the mirrored half overlaps the batch (mirror_offset is in elements, |offset| >= B * 3 * Hw * Ww)");
  const bool vec = (Ww & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0 && (!mirror_too || (mirror_offset & 3) == 0);
  hipStream_t st = (hipStream_t)stream;
#define OCV_CALL(F) launch_remap_ingest<F>(pl, yuv_table, map, M, Hs, Ws, table, out, mirror_offset, Hw, Ww, B, vec, mirror_too != 0, st)
  OCV_PIXFMT_DISPATCH(format, OCV_CALL)
#undef OCV_CALL
  OCV_CHECK_LAUNCH("ocv_frame_remap_ingest_fwd");
  return 0;
}

extern "C" int ocv_frames_remap_rgb24_fwd(int format, const uint8_t* plane0, long frame_stride0, long row_stride0, const uint8_t* plane1,
                                          long frame_stride1, long row_stride1, const uint8_t* plane2, long frame_stride2,
                                          long row_stride2, const int* yuv_table, int Hs, int Ws, const int* map, int M, int Hw, int Ww,
                                          uint8_t* out, int B, ocv_stream_t stream) {
  const pixfmt::Planes pl{{plane0, plane1, plane2}, {frame_stride0, frame_stride1, frame_stride2}, {row_stride0, row_stride1, row_stride2}};
  OCV_CHECK_ARG(out, "ocv_frames_remap_rgb24_fwd: null pointer (out)");
  if (pixfmt::check_source("ocv_frames_remap_rgb24_fwd", format, pl, yuv_table, B, Hs, Ws)) return -1;
  if (check_map("ocv_frames_remap_rgb24_fwd", map, M, B, Hw, Ww)) return -1;
  const bool vec = (Ww & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0;
  hipStream_t st = (hipStream_t)stream;
#define OCV_CALL(F) launch_remap_rgb<F>(pl, yuv_table, map, M, Hs, Ws, out, Hw, Ww, B, vec, st)
  OCV_PIXFMT_DISPATCH(format, OCV_CALL)
#undef OCV_CALL
  OCV_CHECK_LAUNCH("ocv_frames_remap_rgb24_fwd");
  return 0;
}
