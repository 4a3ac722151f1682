// Resize on ingest (row N5 of DESIGN.md section 6b): a window of ANY size of the decoded frames -> the model's H x W, antialiased, in the
// launch that normalises and mirrors -- what ocv_frame_ingest_fwd (frame_ingest.hip) does for a window that already has the model's size.
//   out[b][c][y][x] = sum_j sum_k wy[y][j] wx[x][k] table[c][ frames[b][top + ystart[y] + j][left + xstart[x] + k][c] ]
// The tap tables (per axis int32 start[n_out], fp32 weight[n_out][K], rows with fewer than K taps padded with weight 0) are the
// antialiased triangle filter in float64, rounded to fp32 once BY THE HOST (hip_ops.resize_taps; the statement the tests hold it to is
// tests/resize_ref.py): nothing here decides where a tap falls.  The kernel only stages, looks up, and accumulates.
// One 256-thread workgroup per image and output tile, all three channels:
//   stage   the source rows x columns the tile's taps cover, global -> LDS AS BYTES, each row kept at its global address's phase mod 4 so
//           that whole dwords go through 4-byte loads and stores and only the ragged ends of a row through byte loads
//   pass 1  x taps: bytes -> table (3 KB in LDS, as frame_ingest_kernel keeps it) -> fp32 LDS tile [source row][channel][tile column]
//   pass 2  y taps from that tile -> global: one 16-byte store per channel plane and the same four values reversed at the mirrored
//           columns (W % 4 == 0, 16-byte aligned out), else scalar stores -- the rules of the existing ingest
// Taps are added in ascending source index with fp32 fma; no atomics, no workgroup waits for another: two calls give identical bytes.
// Neighbouring tiles re-read their tap halo from global memory (L2 serves most of it).  The host picks the tile from the ratio and the
// tap counts so that the LDS request stays under FRAME_RESIZE_LDS_BUDGET.  Every staged extent is clamped to the window and to the LDS
// capacity the host sized, and every LDS index to the staged extent: a zero-weight slot -- or a table that is not resize_taps' -- reads
// a staged byte with weight 0 (or a wrong staged byte), never memory outside the window.
// Pixel formats (ocv_frame_resize_ingest_format; pixel_fetch.hpp): frames in bgr24 / rgba32 / bgra32 / nv12 / i420 are converted while
// they are staged -- the staged rows hold RGB bytes either way -- and the two passes do not know the difference.
#include "common.hpp"
#include "../../include/objcavit_hip.h"
#include "pixel_fetch.hpp"

namespace {

constexpr int FRAME_RESIZE_LDS_BUDGET = 48 * 1024;    // preferred request: three workgroups per CU
constexpr int FRAME_RESIZE_LDS_MAX = 64 * 1024;       // what one workgroup may ask for

// S: pixfmt::Packed (one plane; ocv_frame_resize_ingest's arguments, in their order) or pixfmt::Planar (4:2:0 planes + the YCbCr tables)
template <class S>
struct ResizeArgs {
  S s;
  const float* table;                 // [3][256]
  const int* ystart;                  // [H]
  const float* ywt;                   // [H][Ky]
  const int* xstart;                  // [W]
  const float* xwt;                   // [W][Kx]
  float* out;                         // [B][3][H][W]
  long mirror_offset;                 // elements from an image to its mirrored copy
  int top, left, Hw, Ww, H, W, Ky, Kx;
  int th_shift, tw_shift;             // output tile = (1 << th_shift) rows x (1 << tw_shift) columns
  int sr_cap, sc_cap, pw;             // staged source rows / columns at most; dwords per staged row (pitch)
};

__host__ __device__ inline int round4(int v) { return (v + 3) & ~3; }

// LDS carve, in 4-byte words, every offset a multiple of 4 words (16 bytes): table | (4:2:0 formats: the five int32 tables of Statement
// P, yuv_words = pixfmt::YUV_TABLE_WORDS) | x weights | y weights | x starts | y starts | fp32 tile [sr_cap][3][TW] | staged bytes
// [sr_cap][pw dwords]
struct Carve {
  int xw, yw, xs, ys, mid, raw, words;
};

__host__ __device__ inline Carve carve(int TH, int TW, int Ky, int Kx, int sr_cap, int pw, int yuv_words) {
  Carve c;
  c.xw = 768 + yuv_words;
  c.yw = c.xw + round4(TW * Kx);
  c.xs = c.yw + round4(TH * Ky);
  c.ys = c.xs + round4(TW);
  c.mid = c.ys + round4(TH);
  c.raw = c.mid + round4(sr_cap * 3 * TW);
  c.words = c.raw + round4(sr_cap * pw);
  return c;
}

__device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// FMT: the OCV_PIXFMT_* layout of the source (pixel_fetch.hpp).  Only the staging step reads it: for anything but rgb24 it leaves RGB
// BYTES in the staged rows -- Statement P per staged pixel, or the packed format's bytes re-ordered -- at phase 0 and the same pitch, and
// pass 1 and pass 2 run on them as they do on rgb24 bytes: same taps, same fma order.
template <int FMT, bool VEC, bool MIRROR>
__global__ __launch_bounds__(256) void frame_resize_kernel(ResizeArgs<typename pixfmt::Source<FMT>::type> p) {
  constexpr bool RGB24 = FMT == OCV_PIXFMT_RGB24;
  constexpr int YUV_WORDS = pixfmt::is_yuv(FMT) ? pixfmt::YUV_TABLE_WORDS : 0;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int TH = 1 << p.th_shift, TW = 1 << p.tw_shift;
  const Carve cv = carve(TH, TW, p.Ky, p.Kx, p.sr_cap, p.pw, YUV_WORDS);
  float* tab = smem;
  float* xw = smem + cv.xw;
  float* yw = smem + cv.yw;
  int* xs = reinterpret_cast<int*>(smem + cv.xs);
  int* ys = reinterpret_cast<int*>(smem + cv.ys);
  float* mid = smem + cv.mid;
  uint32_t* raw = reinterpret_cast<uint32_t*>(smem + cv.raw);

  const int tid = threadIdx.x;
  const int tx0 = blockIdx.x << p.tw_shift, ty0 = blockIdx.y << p.th_shift, b = blockIdx.z;
  const int nx = min(TW, p.W - tx0), ny = min(TH, p.H - ty0);
  // the source columns [c0, c0 + SC) and rows [r0, r0 + SR) of the window that the tile's taps cover (starts ascend with the index)
  const int c0 = clampi(p.xstart[tx0], 0, p.Ww - 1);
  const int SC = min(clampi(p.xstart[tx0 + nx - 1] + p.Kx, c0 + 1, p.Ww) - c0, p.sc_cap);
  const int r0 = clampi(p.ystart[ty0], 0, p.Hw - 1);
  const int SR = min(clampi(p.ystart[ty0 + ny - 1] + p.Ky, r0 + 1, p.Hw) - r0, p.sr_cap);

  for (int i = tid; i < 3 * 256; i += 256) tab[i] = p.table[i];
  if constexpr (pixfmt::is_yuv(FMT)) {
    for (int i = tid; i < YUV_WORDS; i += 256) reinterpret_cast<int*>(smem + 768)[i] = p.s.yuv[i];
    __syncthreads();                                            // the staging below reads the tables
  }
  for (int i = tid; i < nx * p.Kx; i += 256) xw[i] = p.xwt[(long)tx0 * p.Kx + i];
  for (int i = tid; i < ny * p.Ky; i += 256) yw[i] = p.ywt[(long)ty0 * p.Ky + i];
  if (tid < nx) xs[tid] = p.xstart[tx0 + tid];
  if (tid < ny) ys[tid] = p.ystart[ty0 + tid];

  // stage: a wave per source row; dword k of a row covers the row's bytes 4 k - phase .. + 3 (phase = the row address mod 4), so a
  // dword that lies wholly inside the row is an aligned 4-byte load and lands on an aligned LDS dword
  const uint8_t* base = p.s.src + b * p.s.frame_stride + (long)(p.top + r0) * p.s.row_stride + (long)(p.left + c0) * 3;    // (rgb24 only)
  const int L = SC * 3;
  if constexpr (!RGB24) {
    // a wave per source row, a lane per group of four staged pixels: 12 RGB bytes = dwords 3 k .. 3 k + 2 of the row; the ragged end
    // (SC % 4 pixels) pixel by pixel through byte stores.  Nothing outside the staged extent -- hence the window -- is read.
    const int* yt = reinterpret_cast<const int*>(smem + 768);
    const int groups = SC >> 2;
    for (int r = tid >> 6; r < SR; r += 4) {
      uint32_t* row = raw + r * p.pw;
      for (int k = tid & 63; k < groups; k += 64) {
        uint8_t px[12];
        pixfmt::fetch4<FMT>(p.s, yt, b, p.top + r0 + r, p.left + c0 + 4 * k, px);
        uint32_t w[3];
        __builtin_memcpy(w, px, 12);
        row[3 * k] = w[0];
        row[3 * k + 1] = w[1];
        row[3 * k + 2] = w[2];
      }
      for (int k = 4 * groups + (tid & 63); k < SC; k += 64) {
        uint8_t rgb[3];
        pixfmt::fetch1<FMT>(p.s, yt, b, p.top + r0 + r, p.left + c0 + k, rgb);
        uint8_t* d = reinterpret_cast<uint8_t*>(row) + 3 * k;
        d[0] = rgb[0];
        d[1] = rgb[1];
        d[2] = rgb[2];
      }
    }
  }
  // rgb24: the statements of the kernel as it was, word for word (`base` and `p.s.row_stride` are read under both source types so that
  // they need no wrapper: this instantiation's instruction stream is pinned, and the compiler's schedule follows the source closely)
  if constexpr (RGB24)
  for (int r = tid >> 6; r < SR; r += 4) {
    const uint8_t* rowp = base + (long)r * p.s.row_stride;
    const int phase = (int)(reinterpret_cast<uintptr_t>(rowp) & 3);
    const int ndw = (phase + L + 3) >> 2;                       // <= pw = (3 * sc_cap + 3) / 4 + 1
    for (int k = tid & 63; k < ndw; k += 64) {
      const int lo = 4 * k - phase;
      if (lo >= 0 && lo + 4 <= L) {
        raw[r * p.pw + k] = *reinterpret_cast<const uint32_t*>(rowp + lo);
      } else {
        uint8_t* d = reinterpret_cast<uint8_t*>(raw + r * p.pw + k);
#pragma unroll
        for (int t = 0; t < 4; ++t)
          if (lo + t >= 0 && lo + t < L) d[t] = rowp[lo + t];
      }
    }
  }
  __syncthreads();

  // pass 1: x taps.  mid[r][c][x] = sum_k wx[x][k] table[c][ byte (r, xstart[x] + k, c) ]
  for (int it = tid; it < (SR << p.tw_shift); it += 256) {
    const int r = it >> p.tw_shift, x = it & (TW - 1);
    if (x >= nx) continue;
    int phase = (int)(reinterpret_cast<uintptr_t>(base + (long)r * p.s.row_stride) & 3);
    if constexpr (!RGB24) phase = 0;
    const uint8_t* rb = reinterpret_cast<const uint8_t*>(raw + r * p.pw) + phase;
    const int s0 = xs[x] - c0;
    const float* w = xw + x * p.Kx;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int k = 0; k < p.Kx; ++k) {
      const uint8_t* px = rb + clampi(s0 + k, 0, SC - 1) * 3;
      const float wk = w[k];
      a0 = fmaf(wk, tab[px[0]], a0);
      a1 = fmaf(wk, tab[256 + px[1]], a1);
      a2 = fmaf(wk, tab[512 + px[2]], a2);
    }
    float* m = mid + ((r * 3) << p.tw_shift) + x;
    m[0] = a0;
    m[TW] = a1;
    m[2 * TW] = a2;
  }
  __syncthreads();

  // pass 2: y taps, and out
  const long plane = (long)p.H * p.W;
  if constexpr (VEC) {
    const int gs = p.tw_shift - 2;                               // four columns per thread
    for (int it = tid; it < (3 << (p.th_shift + gs)); it += 256) {
      const int x = (it & ((1 << gs) - 1)) << 2, y = (it >> gs) & (TH - 1), c = it >> (gs + p.th_shift);
      if (x >= nx || y >= ny) continue;                         // (W % 4 == 0: a group of four lies wholly inside or outside)
      const int s0 = ys[y] - r0;
      const float* w = yw + y * p.Ky;
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int j = 0; j < p.Ky; ++j) {
        const float4 v = *reinterpret_cast<const float4*>(mid + ((clampi(s0 + j, 0, SR - 1) * 3 + c) << p.tw_shift) + x);
        const float wj = w[j];
        a.x = fmaf(wj, v.x, a.x);
        a.y = fmaf(wj, v.y, a.y);
        a.z = fmaf(wj, v.z, a.z);
        a.w = fmaf(wj, v.w, a.w);
      }
      const int ox = tx0 + x;
      float* o = p.out + ((long)b * 3 + c) * plane + (long)(ty0 + y) * p.W;
      *reinterpret_cast<float4*>(o + ox) = a;
      if constexpr (MIRROR) *reinterpret_cast<float4*>(o + p.mirror_offset + (p.W - 4 - ox)) = make_float4(a.w, a.z, a.y, a.x);
    }
  } else {
    for (int it = tid; it < (3 << (p.th_shift + p.tw_shift)); it += 256) {
      const int x = it & (TW - 1), y = (it >> p.tw_shift) & (TH - 1), c = it >> (p.tw_shift + p.th_shift);
      if (x >= nx || y >= ny) continue;
      const int s0 = ys[y] - r0;
      const float* w = yw + y * p.Ky;
      float a = 0.f;
      for (int j = 0; j < p.Ky; ++j) a = fmaf(w[j], mid[((clampi(s0 + j, 0, SR - 1) * 3 + c) << p.tw_shift) + x], a);
      const int ox = tx0 + x;
      float* o = p.out + ((long)b * 3 + c) * plane + (long)(ty0 + y) * p.W;
      o[ox] = a;
      if constexpr (MIRROR) o[p.mirror_offset + (p.W - 1 - ox)] = a;
    }
  }
}

// source rows / columns a tile of `tile` outputs can cover: the starts of resize_taps' tables rise by at most floor(ratio * (tile - 1)) + 1
// over the tile, the last row adds its K taps (one more for slack); never more than the window has
int staged_extent(int n_in, int n_out, int tile, int K) {
  const long span = (long)n_in * (tile - 1) / n_out + 2 + K;
  return (int)(span < n_in ? span : n_in);
}

struct Plan {
  int th_shift, tw_shift, sr_cap, sc_cap, pw, lds_bytes;
};

// the largest tile whose LDS request stays under the budget: 8 x 64 up to a ratio of about 2.5 per axis, smaller beyond
bool plan_tile(int Hw, int Ww, int H, int W, int Ky, int Kx, Plan* out, int yuv_words = 0) {
  static const int shapes[4][2] = {{3, 6}, {3, 5}, {2, 5}, {2, 4}};
  for (int i = 0; i < 4; ++i) {
    Plan pl;
    pl.th_shift = shapes[i][0];
    pl.tw_shift = shapes[i][1];
    const int TH = 1 << pl.th_shift, TW = 1 << pl.tw_shift;
    pl.sr_cap = staged_extent(Hw, H, TH, Ky);
    pl.sc_cap = staged_extent(Ww, W, TW, Kx);
    pl.pw = (pl.sc_cap * 3 + 3) / 4 + 1;
    pl.lds_bytes = carve(TH, TW, Ky, Kx, pl.sr_cap, pl.pw, yuv_words).words * 4;
    if (pl.lds_bytes <= FRAME_RESIZE_LDS_BUDGET || (i == 3 && pl.lds_bytes <= FRAME_RESIZE_LDS_MAX)) {
      *out = pl;
      return true;
    }
  }
  return false;
}

bool ratio_ok(int Hw, int Ww, int H, int W) {
  return Hw >= 1 && Ww >= 1 && H >= 1 && W >= 1 && (long)Hw <= (long)OCV_FRAME_RESIZE_MAX_RATIO * H &&
         (long)Ww <= (long)OCV_FRAME_RESIZE_MAX_RATIO * W;
}

}  // namespace

extern "C" int ocv_frame_resize_supported(int Hw, int Ww, int H, int W) { return ratio_ok(Hw, Ww, H, W) ? 1 : 0; }

extern "C" int ocv_frame_resize_ingest(const uint8_t* frames, long frame_stride, long row_stride, int Hs, int Ws, int top, int left,
                                       int Hw, int Ww, const float* table, const int* ystart, const float* yweight, int Ky,
                                       const int* xstart, const float* xweight, int Kx, float* out, int B, int H, int W,
                                       int mirror_too, long mirror_offset, ocv_stream_t stream) {
  OCV_CHECK_ARG(frames && table && out && ystart && yweight && xstart && xweight, "ocv_frame_resize_ingest: null pointer");
  OCV_CHECK_ARG(B >= 1 && B <= 65535 && H >= 1 && W >= 1 && Hs >= 1 && Ws >= 1 && Hw >= 1 && Ww >= 1,
                "ocv_frame_resize_ingest: bad sizes (B, H, W, Hs, Ws, Hw, Ww must be >= 1, B <= 65535)");
  OCV_CHECK_ARG(top >= 0 && left >= 0 && (long)top + Hw <= Hs && (long)left + Ww <= Ws, "ocv_frame_resize_ingest: window outside the frame");
  OCV_CHECK_ARG(row_stride >= (long)Ws * 3 && (B == 1 || frame_stride >= (long)(Hs - 1) * row_stride + (long)Ws * 3),
                "ocv_frame_resize_ingest: strides (bytes) smaller than a row / a frame");
  OCV_CHECK_ARG(ratio_ok(Hw, Ww, H, W),
                "ocv_frame_resize_ingest: window %d x %d -> %d x %d shrinks by more than OCV_FRAME_RESIZE_MAX_RATIO = %d along an axis "
                "(the filter is not truncated: resize in two steps)", Hw, Ww, H, W, OCV_FRAME_RESIZE_MAX_RATIO);
  OCV_CHECK_ARG(Ky >= 1 && Kx >= 1 && Ky <= OCV_FRAME_RESIZE_MAX_TAPS && Kx <= OCV_FRAME_RESIZE_MAX_TAPS,
                "ocv_frame_resize_ingest: %d / %d taps per row; 1 .. OCV_FRAME_RESIZE_MAX_TAPS = %d are taken", Ky, Kx, OCV_FRAME_RESIZE_MAX_TAPS);
  OCV_CHECK_ARG(((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(ystart) |
                  reinterpret_cast<uintptr_t>(yweight) | reinterpret_cast<uintptr_t>(xstart) | reinterpret_cast<uintptr_t>(xweight)) & 3) == 0,
                "ocv_frame_resize_ingest: out / table / tap tables must be 4-byte aligned");
  OCV_CHECK_ARG(!mirror_too || mirror_offset >= (long)B * 3 * H * W || mirror_offset <= -(long)B * 3 * H * W,
                "ocv_frame_resize_ingest: the mirrored half overlaps the batch (mirror_offset is in elements, |offset| >= B * 3 * H * W)");
  Plan pl;
  OCV_CHECK_ARG(plan_tile(Hw, Ww, H, W, Ky, Kx, &pl), "ocv_frame_resize_ingest: no tile fits %d bytes of LDS", FRAME_RESIZE_LDS_MAX);
  ResizeArgs<pixfmt::Packed> a{{frames, frame_stride, row_stride}, table, ystart, yweight, xstart, xweight, out, mirror_offset,
               top, left, Hw, Ww, H, W, Ky, Kx, pl.th_shift, pl.tw_shift, pl.sr_cap, pl.sc_cap, pl.pw};
  const bool vec = (W & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0 && (!mirror_too || (mirror_offset & 3) == 0);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((W + (1 << pl.tw_shift) - 1) >> pl.tw_shift, (H + (1 << pl.th_shift) - 1) >> pl.th_shift, B);
  OCV_CHECK_ARG(grid.y <= 65535, "ocv_frame_resize_ingest: H = %d is more than 65535 tiles tall", H);
  if (vec && mirror_too) hipLaunchKernelGGL((frame_resize_kernel<OCV_PIXFMT_RGB24, true, true>), grid, dim3(256), pl.lds_bytes, st, a);
  else if (vec) hipLaunchKernelGGL((frame_resize_kernel<OCV_PIXFMT_RGB24, true, false>), grid, dim3(256), pl.lds_bytes, st, a);
  else if (mirror_too) hipLaunchKernelGGL((frame_resize_kernel<OCV_PIXFMT_RGB24, false, true>), grid, dim3(256), pl.lds_bytes, st, a);
  else hipLaunchKernelGGL((frame_resize_kernel<OCV_PIXFMT_RGB24, false, false>), grid, dim3(256), pl.lds_bytes, st, a);
  OCV_CHECK_LAUNCH("ocv_frame_resize_ingest");
  return 0;
}

namespace {

struct ResizeCall {
  const float* table;
  const int* ystart;
  const float* ywt;
  const int* xstart;
  const float* xwt;
  float* out;
  long mirror_offset;
  int top, left, Hw, Ww, H, W, Ky, Kx;
};

template <int FMT>
void launch_resize(const pixfmt::Planes& pl, const int* yuv, const ResizeCall& c, const Plan& p, bool vec, bool mirror, dim3 grid,
                   hipStream_t st) {
  using S = typename pixfmt::Source<FMT>::type;
  S src;
  if constexpr (pixfmt::is_yuv(FMT)) src = pixfmt::planar_of(pl, yuv);
  else src = pixfmt::packed_of(pl);
  ResizeArgs<S> a{src, c.table, c.ystart, c.ywt, c.xstart, c.xwt, c.out, c.mirror_offset, c.top, c.left, c.Hw, c.Ww, c.H, c.W, c.Ky, c.Kx,
                  p.th_shift, p.tw_shift, p.sr_cap, p.sc_cap, p.pw};
  if (vec && mirror) hipLaunchKernelGGL((frame_resize_kernel<FMT, true, true>), grid, dim3(256), p.lds_bytes, st, a);
  else if (vec) hipLaunchKernelGGL((frame_resize_kernel<FMT, true, false>), grid, dim3(256), p.lds_bytes, st, a);
  else if (mirror) hipLaunchKernelGGL((frame_resize_kernel<FMT, false, true>), grid, dim3(256), p.lds_bytes, st, a);
  else hipLaunchKernelGGL((frame_resize_kernel<FMT, false, false>), grid, dim3(256), p.lds_bytes, st, a);
}

}  // namespace

extern "C" int ocv_frame_resize_ingest_format(int format, const uint8_t* plane0, long frame_stride0, long row_stride0, const uint8_t* plane1,
                                              long frame_stride1, long row_stride1, const uint8_t* plane2, long frame_stride2,
                                              long row_stride2, const int* yuv_table, int Hs, int Ws, int top, int left, int Hw, int Ww,
                                              const float* table, const int* ystart, const float* yweight, int Ky, const int* xstart,
                                              const float* xweight, int Kx, float* out, int B, int H, int W, int mirror_too,
                                              long mirror_offset, ocv_stream_t stream) {
  const pixfmt::Planes pl{{plane0, plane1, plane2}, {frame_stride0, frame_stride1, frame_stride2}, {row_stride0, row_stride1, row_stride2}};
  OCV_CHECK_ARG(table && out && ystart && yweight && xstart && xweight, "ocv_frame_resize_ingest_format: null pointer (table / out / tap tables)");
  OCV_CHECK_ARG(B >= 1 && B <= 65535 && H >= 1 && W >= 1 && Hs >= 1 && Ws >= 1 && Hw >= 1 && Ww >= 1,
                "ocv_frame_resize_ingest_format: bad sizes (B, H, W, Hs, Ws, Hw, Ww must be >= 1, B <= 65535)");
  if (pixfmt::check_source("ocv_frame_resize_ingest_format", format, pl, yuv_table, B, Hs, Ws)) return -1;
  OCV_CHECK_ARG(top >= 0 && left >= 0 && (long)top + Hw <= Hs && (long)left + Ww <= Ws,
                "ocv_frame_resize_ingest_format: window outside the frame");
  OCV_CHECK_ARG(ratio_ok(Hw, Ww, H, W),
                "ocv_frame_resize_ingest_format: window %d x %d -> %d x %d shrinks by more than OCV_FRAME_RESIZE_MAX_RATIO = %d along an axis "
                "(the filter is not truncated: resize in two steps)", Hw, Ww, H, W, OCV_FRAME_RESIZE_MAX_RATIO);
  OCV_CHECK_ARG(Ky >= 1 && Kx >= 1 && Ky <= OCV_FRAME_RESIZE_MAX_TAPS && Kx <= OCV_FRAME_RESIZE_MAX_TAPS,
                "ocv_frame_resize_ingest_format: %d / %d taps per row; 1 .. OCV_FRAME_RESIZE_MAX_TAPS = %d are taken", Ky, Kx,
                OCV_FRAME_RESIZE_MAX_TAPS);
  OCV_CHECK_ARG(((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(ystart) |
                  reinterpret_cast<uintptr_t>(yweight) | reinterpret_cast<uintptr_t>(xstart) | reinterpret_cast<uintptr_t>(xweight)) & 3) == 0,
                "ocv_frame_resize_ingest_format: out / table / tap tables must be 4-byte aligned");
  OCV_CHECK_ARG(!mirror_too || mirror_offset >= (long)B * 3 * H * W || mirror_offset <= -(long)B * 3 * H * W,
                "ocv_frame_resize_ingest_format: the mirrored half overlaps the batch (mirror_offset is in elements, |offset| >= B * 3 * H * W)");
  Plan p;
  OCV_CHECK_ARG(plan_tile(Hw, Ww, H, W, Ky, Kx, &p, pixfmt::is_yuv(format) ? pixfmt::YUV_TABLE_WORDS : 0),
                "ocv_frame_resize_ingest_format: no tile fits %d bytes of LDS", FRAME_RESIZE_LDS_MAX);
  const ResizeCall c{table, ystart, yweight, xstart, xweight, out, mirror_offset, top, left, Hw, Ww, H, W, Ky, Kx};
  const bool vec = (W & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0 && (!mirror_too || (mirror_offset & 3) == 0);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((W + (1 << p.tw_shift) - 1) >> p.tw_shift, (H + (1 << p.th_shift) - 1) >> p.th_shift, B);
  OCV_CHECK_ARG(grid.y <= 65535, "ocv_frame_resize_ingest_format: H = %d is more than 65535 tiles tall", H);
  switch (format) {
    case OCV_PIXFMT_RGB24: launch_resize<OCV_PIXFMT_RGB24>(pl, yuv_table, c, p, vec, mirror_too != 0, grid, st); break;
    case OCV_PIXFMT_BGR24: launch_resize<OCV_PIXFMT_BGR24>(pl, yuv_table, c, p, vec, mirror_too != 0, grid, st); break;
    case OCV_PIXFMT_RGBA32: launch_resize<OCV_PIXFMT_RGBA32>(pl, yuv_table, c, p, vec, mirror_too != 0, grid, st); break;
    case OCV_PIXFMT_BGRA32: launch_resize<OCV_PIXFMT_BGRA32>(pl, yuv_table, c, p, vec, mirror_too != 0, grid, st); break;
    case OCV_PIXFMT_NV12: launch_resize<OCV_PIXFMT_NV12>(pl, yuv_table, c, p, vec, mirror_too != 0, grid, st); break;
    default: launch_resize<OCV_PIXFMT_I420>(pl, yuv_table, c, p, vec, mirror_too != 0, grid, st); break;
  }
  OCV_CHECK_LAUNCH("ocv_frame_resize_ingest_format");
  return 0;
}
