// Pixel formats on ingest ("Pixel formats on ingest"): what frame_ingest.hip and frame_resize.hip share to read a
// decoded frame of any OCV_PIXFMT_* layout (include/objcavit_hip.h) as R, G, B bytes.
//   packed   rgb24 / bgr24 (3 bytes per pixel), rgba32 / bgra32 (4 bytes per pixel, alpha ignored): one plane
//   4:2:0    nv12 (Y plane + interleaved CbCr plane), i420 (Y, Cb, Cr planes): pixel (x, y) takes chroma sample (x >> 1, y >> 1)
// YCbCr -> RGB is Statement P: integer sums of five int32 tables [5][256] that the HOST makes (objcavit_amd/pixel_formats.py yuv_tables:
// matrix, range and rounding are decided there), an arithmetic shift by 16 and a clamp to 0 .. 255.  The kernel holds the tables in LDS.
// Every plane has its own base pointer, frame stride and row stride in bytes, at any alignment: all loads go through memcpy of bytes.
#pragma once
#include "common.hpp"
#include "../../include/objcavit_hip.h"

namespace pixfmt {

constexpr int YUV_TABLE_WORDS = 5 * 256;

struct Packed {                       // one plane: the layout of the rgb24 entry points' arguments
  const uint8_t* src;
  long frame_stride, row_stride;      // bytes
};

struct Planar {                       // 4:2:0: plane 0 = Y; plane 1 = CbCr (nv12) or Cb (i420); plane 2 = Cr (i420)
  const uint8_t* src;                 // the Y plane, under the names of Packed's one plane
  long frame_stride, row_stride;
  const uint8_t* c0;
  long c0_frame, c0_row;
  const uint8_t* c1;
  long c1_frame, c1_row;
  const int* yuv;                     // [5][256] int32 in device memory
};

__host__ __device__ constexpr bool is_yuv(int fmt) { return fmt == OCV_PIXFMT_NV12 || fmt == OCV_PIXFMT_I420; }
__host__ __device__ constexpr int packed_bytes(int fmt) { return fmt == OCV_PIXFMT_RGBA32 || fmt == OCV_PIXFMT_BGRA32 ? 4 : 3; }
__host__ __device__ constexpr bool is_bgr(int fmt) { return fmt == OCV_PIXFMT_BGR24 || fmt == OCV_PIXFMT_BGRA32; }

template <int FMT>
struct Source {
  using type = Packed;
};
template <>
struct Source<OCV_PIXFMT_NV12> {
  using type = Planar;
};
template <>
struct Source<OCV_PIXFMT_I420> {
  using type = Planar;
};

// clamp(v >> 16, 0, 255), written as clamp(v, 0, 2^24 - 1) >> 16 -- the same byte for every int.  The first form compiles to gfx950's
// v_ashr_pk_u8_i32 (shift, saturate and pack two bytes), and the bytes OR-ed into the upper half of that instruction's result came out
// wrong on the MI355X (tests/test_hip_pixel_formats.py caught it); the second form is a v_med3 and a plain shift.
__device__ inline uint8_t clamp_shift(int v) {
  v = v < 0 ? 0 : (v > 0xFFFFFF ? 0xFFFFFF : v);
  return (uint8_t)((unsigned)v >> 16);
}

// the three chroma terms of one sample: Cr -> R, Cb and Cr -> G, Cb -> B (four look-ups)
struct ChromaTerms {
  int r, g, b;
};
__device__ inline ChromaTerms chroma_terms(const int* yt, uint8_t cb, uint8_t cr) {
  return ChromaTerms{yt[256 + cr], yt[512 + cb] + yt[768 + cr], yt[1024 + cb]};
}

__device__ inline void yuv_pixel(const int* yt, uint8_t y, const ChromaTerms& t, uint8_t* rgb) {
  const int l = yt[y];
  rgb[0] = clamp_shift(l + t.r);
  rgb[1] = clamp_shift(l + t.g);
  rgb[2] = clamp_shift(l + t.b);
}

// chroma sample (cx, cy) of image b
template <int FMT>
__device__ inline ChromaTerms chroma_at(const Planar& s, const int* yt, int b, int cy, int cx) {
  if constexpr (FMT == OCV_PIXFMT_NV12) {
    const uint8_t* c = s.c0 + b * s.c0_frame + (long)cy * s.c0_row + 2L * cx;
    return chroma_terms(yt, c[0], c[1]);
  } else {
    return chroma_terms(yt, s.c0[b * s.c0_frame + (long)cy * s.c0_row + cx], s.c1[b * s.c1_frame + (long)cy * s.c1_row + cx]);
  }
}

// one pixel (row, col) of image b -> rgb[3].  yt: the LDS copy of the tables (unused by the packed formats)
template <int FMT>
__device__ inline void fetch1(const typename Source<FMT>::type& s, const int* yt, int b, int row, int col, uint8_t* rgb) {
  if constexpr (is_yuv(FMT)) {
    const ChromaTerms t = chroma_at<FMT>(s, yt, b, row >> 1, col >> 1);
    yuv_pixel(yt, s.src[b * s.frame_stride + (long)row * s.row_stride + col], t, rgb);
  } else {
    const uint8_t* p = s.src + b * s.frame_stride + (long)row * s.row_stride + (long)col * packed_bytes(FMT);
    rgb[0] = p[is_bgr(FMT) ? 2 : 0];
    rgb[1] = p[1];
    rgb[2] = p[is_bgr(FMT) ? 0 : 2];
  }
}

// four consecutive pixels (row, col .. col + 3) of image b -> px[12] = R G B R G B ...  col has any parity: the four pixels touch two
// chroma samples (col even) or three (col odd); each is fetched and looked up once
template <int FMT>
__device__ inline void fetch4(const typename Source<FMT>::type& s, const int* yt, int b, int row, int col, uint8_t* px) {
  if constexpr (is_yuv(FMT)) {
    uint8_t y[4];
    __builtin_memcpy(y, s.src + b * s.frame_stride + (long)row * s.row_stride + col, 4);
    const int cy = row >> 1, cx = col >> 1;
    const bool odd = col & 1;
    ChromaTerms t0, t1, t2;
    if constexpr (FMT == OCV_PIXFMT_NV12) {
      const uint8_t* c = s.c0 + b * s.c0_frame + (long)cy * s.c0_row + 2L * cx;
      uint8_t v[4];
      __builtin_memcpy(v, c, 4);
      t0 = chroma_terms(yt, v[0], v[1]);
      t1 = chroma_terms(yt, v[2], v[3]);
      t2 = t1;
      if (odd) {
        uint8_t w[2];
        __builtin_memcpy(w, c + 4, 2);
        t2 = chroma_terms(yt, w[0], w[1]);
      }
    } else {
      const uint8_t* cb = s.c0 + b * s.c0_frame + (long)cy * s.c0_row + cx;
      const uint8_t* cr = s.c1 + b * s.c1_frame + (long)cy * s.c1_row + cx;
      t0 = chroma_terms(yt, cb[0], cr[0]);
      t1 = chroma_terms(yt, cb[1], cr[1]);
      t2 = t1;
      if (odd) t2 = chroma_terms(yt, cb[2], cr[2]);
    }
    // pixel i reads sample ((col & 1) + i) >> 1: 0 0 1 1 (even), 0 1 1 2 (odd)
    yuv_pixel(yt, y[0], t0, px);
    yuv_pixel(yt, y[1], odd ? t1 : t0, px + 3);
    yuv_pixel(yt, y[2], t1, px + 6);
    yuv_pixel(yt, y[3], odd ? t2 : t1, px + 9);
  } else if constexpr (packed_bytes(FMT) == 4) {
    uint8_t q[16];
    __builtin_memcpy(q, s.src + b * s.frame_stride + (long)row * s.row_stride + (long)col * 4, 16);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      px[3 * i] = q[4 * i + (is_bgr(FMT) ? 2 : 0)];
      px[3 * i + 1] = q[4 * i + 1];
      px[3 * i + 2] = q[4 * i + (is_bgr(FMT) ? 0 : 2)];
    }
  } else if constexpr (FMT == OCV_PIXFMT_BGR24) {
    uint8_t q[12];
    __builtin_memcpy(q, s.src + b * s.frame_stride + (long)row * s.row_stride + (long)col * 3, 12);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      px[3 * i] = q[3 * i + 2];
      px[3 * i + 1] = q[3 * i + 1];
      px[3 * i + 2] = q[3 * i];
    }
  } else {
    __builtin_memcpy(px, s.src + b * s.frame_stride + (long)row * s.row_stride + (long)col * 3, 12);
  }
}

// the host's description of a frame batch of any format, as the *_format entry points take it
struct Planes {
  const uint8_t* p[3];
  long frame[3], row[3];
};

inline Packed packed_of(const Planes& pl) { return Packed{pl.p[0], pl.frame[0], pl.row[0]}; }
inline Planar planar_of(const Planes& pl, const int* yuv) {
  return Planar{pl.p[0], pl.frame[0], pl.row[0], pl.p[1], pl.frame[1], pl.row[1], pl.p[2], pl.frame[2], pl.row[2], yuv};
}

// argument checks every *_format entry point shares; 0, or -1 with the message set.  `who` names the entry point.
inline int check_source(const char* who, int format, const Planes& pl, const int* yuv_table, int B, int Hs, int Ws) {
  OCV_CHECK_ARG(format >= OCV_PIXFMT_RGB24 && format <= OCV_PIXFMT_I420, "%s: unknown pixel format id %d (OCV_PIXFMT_*: 0 .. %d)", who,
                format, OCV_PIXFMT_I420);
  OCV_CHECK_ARG(B >= 1 && Hs >= 1 && Ws >= 1, "%s: bad sizes (B, Hs, Ws must be >= 1)", who);
  const int nplanes = format == OCV_PIXFMT_I420 ? 3 : (format == OCV_PIXFMT_NV12 ? 2 : 1);
  for (int i = 0; i < nplanes; ++i) OCV_CHECK_ARG(pl.p[i] != nullptr, "%s: null pointer (plane %d of the format)", who, i);
  const long Hc = (Hs + 1) / 2, Wc = (Ws + 1) / 2;
  for (int i = 0; i < nplanes; ++i) {
    const long rows = i == 0 ? Hs : Hc;
    const long bytes = i == 0 ? (long)Ws * (is_yuv(format) ? 1 : packed_bytes(format)) : (format == OCV_PIXFMT_NV12 ? 2 * Wc : Wc);
    OCV_CHECK_ARG(pl.row[i] >= bytes && (B == 1 || pl.frame[i] >= (rows - 1) * pl.row[i] + bytes),
                  "%s: strides (bytes) of plane %d smaller than a row (%ld bytes) / a frame of that plane", who, i, bytes);
  }
  if (is_yuv(format))
    OCV_CHECK_ARG(yuv_table != nullptr && (reinterpret_cast<uintptr_t>(yuv_table) & 3) == 0,
                  "%s: yuv_table (int32 [5][256]) is null or not 4-byte aligned", who);
  return 0;
}

}  // namespace pixfmt
