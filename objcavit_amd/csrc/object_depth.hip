// Per-object readout behind the predict path's final map: depth statistics per detection box, on the device.
//   depth [B][1][H][W] (+ depth_std), boxes xywh [B][cap][>= 4] = centre x, centre y, width, height in the map's pixel grid, counts [B]
//   -> out [B][cap][5 + Q] = n, min, max, mean, std_mean, q_0 .. q_{Q-1}     (the record is defined in include/objcavit_hip.h)
// A segmented ORDER-STATISTIC reduction: the quantiles are elements of the map, selected exactly, not interpolated.
//
// One workgroup per (image, box row).  The box's pixels are read once per pass from the map the finalize launch has just written
// (L2-resident), four passes in all:
//   pass 0   count of the non-NaN pixels, min / max (as integer keys), the float64 sums of depth and depth_std, and the histogram of the
//            keys' top 8 bits;
//   pass 1-3 most-significant-digit-first radix select, 8 bits per pass, for ALL Q ranks at once: a rank owns one 256-bin LDS histogram,
//            a pixel is counted where its key's upper bits equal the rank's prefix so far; ranks that share a prefix share a histogram.
// A key is the order-preserving uint32 image of the fp32 bits (sign flipped for positives, all bits for negatives): unsigned order of the
// keys = numeric order of the values, -0 below +0, NaN never enters.  After a pass one wave per rank scans its 256 digit counts (4 per
// lane + a shuffle scan) and narrows prefix and rank.  The histogram adds are integer LDS atomics (order-free); a depth map is smooth,
// so most lanes of a wave hit ONE bin: the two most common digits of a wave are counted with a ballot and added once by a leader lane,
// only the rest add per lane.  The sums run in a fixed order -- per-thread partials over the thread's fixed pixels, xor shuffles, the
// waves' partials from LDS in wave order -- so two calls are bit-equal; there is no float atomic.
#include "box_edges.hpp"
#include "common.hpp"
#include "../../include/objcavit_hip.h"

namespace {

constexpr int OD_THREADS = 256, OD_WAVES = OD_THREADS / OCV_WAVE, OD_MAXQ = 8, OD_BINS = 256, OD_ROWS = 8;

struct ObjDepthArgs {
  const float *depth, *depth_std, *xywh;
  const int* counts;
  float* out;
  long xywh_row_stride;
  int B, cap, H, W, Q;
  float half;
  double q[OD_MAXQ];
};

__device__ __forceinline__ unsigned od_key(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float od_value(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

// ++hist[digit] for the lanes with `on`, called by a whole wave: two rounds of "the first such lane's digit, counted by ballot, added
// once", then one atomic per lane that is left
__device__ __forceinline__ void od_hist_add(unsigned* hist, unsigned digit, bool on, int lane) {
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const unsigned long long m = __ballot(on);
    if (m == 0ull) return;                                                   // (wave-uniform)
    const int leader = __ffsll((long long)m) - 1;
    const unsigned d = (unsigned)__shfl((int)digit, leader, OCV_WAVE);
    const bool same = on && digit == d;
    const unsigned long long peers = __ballot(same);
    if (lane == leader) atomicAdd(&hist[d], (unsigned)__popcll(peers));
    on = on && !same;
  }
  if (on) atomicAdd(&hist[digit], 1u);
}

__device__ __forceinline__ double od_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, OCV_WAVE);
  return v;
}

// One wave: the digit d with  sum(h[0..d)) <= rank < sum(h[0..d]),  and the rank within it.  rank < sum(h) by construction.
__device__ __forceinline__ void od_narrow(const unsigned* h, unsigned rank, int lane, unsigned& digit, unsigned& rank_in) {
  const unsigned c0 = h[4 * lane], c1 = h[4 * lane + 1], c2 = h[4 * lane + 2], c3 = h[4 * lane + 3];
  const unsigned own = c0 + c1 + c2 + c3;
  unsigned incl = own;
#pragma unroll
  for (int o = 1; o < OCV_WAVE; o <<= 1) {
    const unsigned up = (unsigned)__shfl_up((int)incl, o, OCV_WAVE);
    if (lane >= o) incl += up;
  }
  const unsigned excl = incl - own;
  const bool hit = rank >= excl && rank < incl;
  unsigned d = 0, r = 0;
  if (hit) {
    r = rank - excl;
    d = 4 * lane;
    if (r >= c0) { r -= c0; ++d;
      if (r >= c1) { r -= c1; ++d;
        if (r >= c2) { r -= c2; ++d; } } }
  }
  const unsigned long long m = __ballot(hit);
  const int src = m ? __ffsll((long long)m) - 1 : 0;
  digit = (unsigned)__shfl((int)d, src, OCV_WAVE);
  rank_in = (unsigned)__shfl((int)r, src, OCV_WAVE);
}

__global__ __launch_bounds__(OD_THREADS) void object_depth_kernel(ObjDepthArgs p) {
  __shared__ unsigned hist[OD_MAXQ][OD_BINS];
  __shared__ double s_sum[OD_WAVES], s_ssum[OD_WAVES];
  __shared__ unsigned s_n[OD_WAVES], s_min[OD_WAVES], s_max[OD_WAVES];
  __shared__ unsigned s_prefix[OD_MAXQ], s_rank[OD_MAXQ];
  __shared__ int s_rep[OD_MAXQ];

  const int tid = threadIdx.x, lane = tid & (OCV_WAVE - 1), wave = tid / OCV_WAVE;
  const int K = 5 + p.Q;
  const long row = blockIdx.x;
  const int b = (int)(row / p.cap), j = (int)(row - (long)b * p.cap);
  float* out = p.out + row * K;

  // everything up to the first barrier is uniform over the workgroup
  int x0 = 0, x1 = 0, y0 = 0, y1 = 0;
  bool live = j < p.counts[b];
  if (live) {
    const float* box = p.xywh + row * p.xywh_row_stride;
    const bool okx = od_edges(box[0], box[2], p.half, p.W, x0, x1);
    const bool oky = od_edges(box[1], box[3], p.half, p.H, y0, y1);
    live = okx && oky;
  }
  if (!live) {
    if (tid < K) out[tid] = 0.f;
    return;
  }

  // the box as TW columns x TH rows of threads, TW the power of two that covers its width (at most the workgroup)
  int log_tw = 0;
  while ((1 << log_tw) < x1 - x0 && (1 << log_tw) < OD_THREADS) ++log_tw;
  const int TW = 1 << log_tw, TH = OD_THREADS >> log_tw;
  const int tx = tid & (TW - 1), ty = tid >> log_tw;
  const long plane = (long)b * p.H * p.W;
  const float* dm = p.depth + plane;
  const float* sm = p.depth_std != nullptr ? p.depth_std + plane : nullptr;
  const float nan = __uint_as_float(0x7fc00000u);

  for (int i = tid; i < OD_MAXQ * OD_BINS; i += OD_THREADS) (&hist[0][0])[i] = 0u;
  __syncthreads();

  // ---- pass 0
  unsigned n = 0, kmin = 0xffffffffu, kmax = 0u;
  double sum = 0.0, ssum = 0.0;
  for (int yb = y0; yb < y1; yb += OD_ROWS * TH) {
    for (int xb = x0; xb < x1; xb += TW) {
      const int x = xb + tx;
      float v[OD_ROWS], s[OD_ROWS];
#pragma unroll
      for (int u = 0; u < OD_ROWS; ++u) {
        const int y = yb + ty + u * TH;
        const bool in = x < x1 && y < y1;
        v[u] = in ? dm[(long)y * p.W + x] : nan;
        s[u] = (in && sm != nullptr) ? sm[(long)y * p.W + x] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < OD_ROWS; ++u) {
        const bool on = v[u] == v[u];
        const unsigned k = od_key(v[u]);
        if (on) {
          ++n;
          kmin = min(kmin, k);
          kmax = max(kmax, k);
          sum += (double)v[u];
          ssum += (double)s[u];
        }
        od_hist_add(hist[0], k >> 24, on, lane);
      }
    }
  }
  sum = od_wave_sum(sum);
  ssum = od_wave_sum(ssum);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    n += (unsigned)__shfl_xor((int)n, o, OCV_WAVE);
    kmin = min(kmin, (unsigned)__shfl_xor((int)kmin, o, OCV_WAVE));
    kmax = max(kmax, (unsigned)__shfl_xor((int)kmax, o, OCV_WAVE));
  }
  if (lane == 0) { s_sum[wave] = sum; s_ssum[wave] = ssum; s_n[wave] = n; s_min[wave] = kmin; s_max[wave] = kmax; }
  __syncthreads();
  n = 0; kmin = 0xffffffffu; kmax = 0u; sum = 0.0; ssum = 0.0;
#pragma unroll
  for (int w = 0; w < OD_WAVES; ++w) {
    n += s_n[w]; kmin = min(kmin, s_min[w]); kmax = max(kmax, s_max[w]); sum += s_sum[w]; ssum += s_ssum[w];
  }
  if (n == 0u) {                                                             // all NaN
    if (tid < K) out[tid] = 0.f;
    return;
  }

  // ---- ranks, and their first digit from pass 0's histogram
  for (int i = wave; i < p.Q; i += OD_WAVES) {
    const double r = floor(p.q[i] * (double)(n - 1u));
    const unsigned rank = min((unsigned)r, n - 1u);
    unsigned d, rin;
    od_narrow(hist[0], rank, lane, d, rin);
    if (lane == 0) { s_prefix[i] = d; s_rank[i] = rin; }
  }

  for (int pass = 1; pass < 4; ++pass) {
    __syncthreads();                                                         // prefixes written, histograms read
    if (tid < p.Q) {                                                         // the first rank with this prefix counts for all of them
      int rep = tid;
      for (int i = tid - 1; i >= 0; --i) rep = s_prefix[i] == s_prefix[tid] ? i : rep;
      s_rep[tid] = rep;
    }
    for (int i = tid; i < OD_MAXQ * OD_BINS; i += OD_THREADS) (&hist[0][0])[i] = 0u;
    __syncthreads();
    const int shift = 24 - 8 * pass;
    for (int yb = y0; yb < y1; yb += OD_ROWS * TH) {
      for (int xb = x0; xb < x1; xb += TW) {
        const int x = xb + tx;
        float v[OD_ROWS];
#pragma unroll
        for (int u = 0; u < OD_ROWS; ++u) {
          const int y = yb + ty + u * TH;
          v[u] = (x < x1 && y < y1) ? dm[(long)y * p.W + x] : nan;
        }
#pragma unroll
        for (int u = 0; u < OD_ROWS; ++u) {
          const bool on = v[u] == v[u];
          const unsigned k = od_key(v[u]);
          const unsigned upper = (k >> shift) >> 8, digit = (k >> shift) & 255u;
          for (int i = 0; i < p.Q; ++i) {
            if (s_rep[i] != i) continue;                                     // (uniform)
            od_hist_add(hist[i], digit, on && upper == s_prefix[i], lane);
          }
        }
      }
    }
    __syncthreads();
    for (int i = wave; i < p.Q; i += OD_WAVES) {
      unsigned d, rin;
      od_narrow(hist[s_rep[i]], s_rank[i], lane, d, rin);
      // (a rank's own prefix and rank: no other wave reads them before the next barrier -- s_rep is not recomputed until then)
      if (lane == 0) { s_prefix[i] = (s_prefix[i] << 8) | d; s_rank[i] = rin; }
    }
  }
  __syncthreads();

  if (tid == 0) {
    out[0] = (float)n;
    out[1] = od_value(kmin);
    out[2] = od_value(kmax);
    out[3] = (float)(sum / (double)n);
    out[4] = sm != nullptr ? (float)(ssum / (double)n) : 0.f;
  }
  if (tid < p.Q) out[5 + tid] = od_value(s_prefix[tid]);
}

}  // namespace

extern "C" int ocv_object_depth_fwd(const float* depth, const float* depth_std, const float* xywh, long xywh_row_stride, const int* counts,
                                    int B, int cap, int H, int W, float half, const double* quantiles, int Q, float* out,
                                    ocv_stream_t stream) {
  OCV_CHECK_ARG(depth && xywh && counts && quantiles && out, "ocv_object_depth_fwd: null pointer (depth, xywh, counts, quantiles, out)");
  OCV_CHECK_ARG(B >= 1 && cap >= 1 && H >= 1 && W >= 1, "ocv_object_depth_fwd: bad sizes (B, cap, H, W must be >= 1)");
  OCV_CHECK_ARG(H <= (1 << 24) && W <= (1 << 24) && (long)H * W <= 0x7fffffffL && (long)B * cap <= 0x7fffffffL,
                "ocv_object_depth_fwd: bad sizes (H, W <= 2^24, H * W and B * cap below 2^31)");
  OCV_CHECK_ARG(xywh_row_stride >= 4, "ocv_object_depth_fwd: xywh_row_stride must be >= 4 (cx, cy, w, h)");
  OCV_CHECK_ARG(Q >= 1 && Q <= OD_MAXQ, "ocv_object_depth_fwd: Q = %d quantiles (1 .. %d)", Q, OD_MAXQ);
  OCV_CHECK_ARG(half > 0.f && half <= 0.5f, "ocv_object_depth_fwd: half = 0.5 * shrink must be in (0, 0.5]");
  ObjDepthArgs a{depth, depth_std, xywh, counts, out, xywh_row_stride, B, cap, H, W, Q, half, {}};
  for (int i = 0; i < Q; ++i) {
    OCV_CHECK_ARG(quantiles[i] >= 0.0 && quantiles[i] <= 1.0, "ocv_object_depth_fwd: quantile %d = %g is outside [0, 1]", i, quantiles[i]);
    a.q[i] = quantiles[i];
  }
  OCV_CHECK_ARG((reinterpret_cast<uintptr_t>(depth) & 3) == 0 && (reinterpret_cast<uintptr_t>(depth_std) & 3) == 0 &&
                (reinterpret_cast<uintptr_t>(xywh) & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0, "ocv_object_depth_fwd: misaligned pointer");
  hipLaunchKernelGGL(object_depth_kernel, dim3((unsigned)((long)B * cap)), dim3(OD_THREADS), 0, (hipStream_t)stream, a);
  OCV_CHECK_LAUNCH("ocv_object_depth_fwd");
  return 0;
}
