// Depthwise k x k convolution (+ folded BatchNorm + SiLU) that also produces the squeeze-excite pooling sums, and the
// squeeze-excite gate computed from them (csrc/se_gate.hip) -- 3 launches per MBConv block where the plain kernels need 5
// (depthwise, channel sum, mean, hidden layer, gate), and no second pass over the depthwise output (the largest
// activations of the network: 295 MB at 120 x 160 x 240 x 16 images).
// Row N1 of SURVEY.md section 8; the reference runs conv_dw / bn / act / se of the hub backbone's blocks
// (modules/DenseFeatureExtractor.py:18-27,149).
//
// dw_slide_kernel<K,S,PX>: a workgroup owns (image, chunk of <= 64 channel quads, PL work items); thread = (channel
//   quad q, work item pl); a work item is a PX-wide, RY-tall strip of outputs walked top to bottom with the K input
//   rows under it held in registers (see the kernel).  Every thread keeps the running sum of its own outputs; the
//   work items of a quad are added through LDS in lane order and the workgroup writes ONE partial per channel:
//   part[b][tile][c].  Fixed order everywhere -> bit-reproducible.
// dw_rows_kernel<S,QLP> (k = 5): a workgroup owns (image, chunk of <= QLP quads, TW x TH output tile); a producer wavefront
//   brings every input row of the tile into an LDS ring once (LDS-DMA), the consumers read the window from there with
//   the weights in registers; same arithmetic, bit-identical outputs, part[b][tile][c] with its own tile count.
//   ocv_depthwise_set_dispatch chooses between the two (tests, tools); automatic: see dw_use_rows.
// The gate from the partials: csrc/se_gate.hip.
#include <stdlib.h>

#include "mbconv_tile.hpp"

namespace {

struct DWSArgs {
  const float *in, *w, *bias;
  float *out, *part;               // out nullable when out_hl is given
  __bf16* out_hl;                  // nullable: the output in the "hl32" split layout (C a multiple of 32), what the project
                                   // 1x1 convolution reads by LDS-DMA (csrc/pointwise_hl.hip): split ONCE, where it is produced
  int C, H, W, Ho, Wo, pad_t, pad_l;
  int QL, PL, RY;                  // quads per chunk, pixel lanes, output rows per work item
  int wox, nwork, tiles, chunks;   // x-blocks per output row, work items per image, workgroups per (image, chunk), chunks
};

// Sliding window: a work item = (x-block of PX output columns, run of RY output rows) of one channel quad.  The K input
// rows under the current output row live in VGPRs as a ring (static indices: the row loop is unrolled K times); moving
// down one output row loads only the S NEW input rows.  Every input element is therefore fetched (PX - 1 + K) / PX / S
// times per run (+ K - S rows of run-in) instead of K * (PX - 1 + K) / PX times: 1.5x instead of 4.5x at k = 3,
// 3x instead of 15x at k = 5 (PX = 2).  The L1 <- L2 path, not HBM, is what bounded the plain kernel (its 18 / 40
// loads per x-block moved 6.5 TB/s out of L2 for 2.9 TB/s of useful traffic).
// Weights: K = 3 in VGPRs (36); K = 5 in LDS (the 100 registers go to the window instead).
// (Round 4 built the squeeze-excite gate INTO this launch -- the image's last workgroup to arrive formed it: correct under load, 50
// launches fewer, not faster (profiles/r04_se_tail.txt); removed in round 5, source in tools/diag/se_tail.patch.txt.)
template <int K, int S, int PX>
__global__ __launch_bounds__(256, 2) void dw_slide_kernel(DWSArgs p) {
  constexpr int NIN = (PX - 1) * S + K;
  constexpr bool WLDS = K > 3;
  __shared__ float4 red[256];
  __shared__ float4 wsh[WLDS ? K * K * 64 : 1];
  const int tid = threadIdx.x;
  const int q = tid % p.QL, pl = tid / p.QL;
  const int c4n = p.C >> 2;
  int tile, chunk;
  long b;
  dw_xcd_decode(p.tiles, p.chunks, tile, chunk, b);
  const int cq = chunk * p.QL + q;
  const int wi = tile * p.PL + pl;
  const bool active = pl < p.PL && cq < c4n && wi < p.nwork;
  const int c = (cq < c4n ? cq : 0) * 4;

  float4 wv[WLDS ? 1 : K * K];
  if (WLDS) {
    for (int t = pl; t < K * K; t += 256 / p.QL) wsh[t * 64 + q] = ld4(p.w + (long)t * p.C + c);
    __syncthreads();
  } else {
#pragma unroll
    for (int t = 0; t < K * K; ++t) wv[t] = ld4(p.w + (long)t * p.C + c);
  }
  const float4 bv = p.bias ? ld4(p.bias + c) : make_float4(0.f, 0.f, 0.f, 0.f);
  float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);

  if (active) {
    const int run = wi / p.wox, xb = wi - run * p.wox;
    const int y0 = run * p.RY, y1 = min(p.Ho, y0 + p.RY);
    const int ox = xb * PX, ix0 = ox * S - p.pad_l;
    const int iyb = y0 * S - p.pad_t;                           // input row of window-relative row 0
    const bool allc = ix0 >= 0 && ix0 + NIN <= p.W;
    const float* ib = p.in + b * (long)p.H * p.W * p.C + c;
    const long opix = (b * p.Ho + y0) * (long)p.Wo + ox;
    float* ob = p.out + opix * p.C + c;
    __bf16* ohb = hl_at(p.out_hl, opix, c, p.C);                            // hl32: hi quad here, lo quad 32 elements on
    float4 win[K][NIN];
    auto load_row = [&](int rel, float4 (&dst)[NIN]) {
      const int iy = iyb + rel;
      const bool rok = iy >= 0 && iy < p.H;
      const float* row = ib + ((long)(rok ? iy : 0) * p.W + ix0) * p.C;
      if (rok && allc) {
#pragma unroll
        for (int j = 0; j < NIN; ++j) dst[j] = ld4(row + (long)j * p.C);
      } else {
#pragma unroll
        for (int j = 0; j < NIN; ++j) {
          const int ix = ix0 + j;
          dst[j] = (rok && ix >= 0 && ix < p.W) ? ld4(row + (long)j * p.C) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
      }
    };
    // PRE (k = 3): the S input rows the NEXT output row adds are requested BEFORE this row's stores, into the ring slots
    // this row has just finished with.  A store counts in vmcnt like a load and vmcnt retires in order, so loads issued
    // behind the stores cannot be waited for without waiting for the stores' acknowledgement as well (240 x 320 x 24:
    // 79 -> 66 us).  It keeps the accumulators alive across the load issue, +16 VGPRs: at k = 5 that costs the second
    // wavefront per SIMD and loses (56 -> 80 us at 30 x 40 x 1056), so k = 5 loads at the top of the row.
    constexpr bool PRE = K == 3;
#pragma unroll
    for (int i = 0; i < (PRE ? K : K - S); ++i) load_row(i, win[i % K]);
    for (int y = y0; y < y1; y += K) {
#pragma unroll
      for (int u = 0; u < K; ++u) {
        if (y + u < y1) {
          if (!PRE) {
#pragma unroll
            for (int sidx = 0; sidx < S; ++sidx) load_row((y + u - y0) * S + K - S + sidx, win[(S * u + K - S + sidx) % K]);
          }
          float4 acc[PX];
#pragma unroll
          for (int o = 0; o < PX; ++o) acc[o] = bv;
#pragma unroll
          for (int r = 0; r < K; ++r) {
            // LDS-resident weights: re-read one row of taps at a time (the fence keeps the compiler from hoisting all
            // K x K x 4 weights of all K unrolled bodies into registers, which costs the occupancy the window needs)
            if (WLDS) asm volatile("" ::: "memory");
#pragma unroll
            for (int j = 0; j < K; ++j) {
              const float4 w4 = WLDS ? wsh[(r * K + j) * 64 + q] : wv[WLDS ? 0 : r * K + j];
#pragma unroll
              for (int o = 0; o < PX; ++o) {
                acc[o] = fma4(w4, win[(S * u + r) % K][o * S + j], acc[o]);
              }
            }
          }
          if (PRE && y + u + 1 < y1) {
#pragma unroll
            for (int sidx = 0; sidx < S; ++sidx) load_row((y + u + 1 - y0) * S + K - S + sidx, win[(S * (u + 1) + K - S + sidx) % K]);
          }
          const long roff = (long)(y + u - y0) * p.Wo;
#pragma unroll
          for (int o = 0; o < PX; ++o) {
            if (ox + o < p.Wo) {
              const float4 r4 = silu4(acc[o]);
              if (p.out != nullptr) *reinterpret_cast<float4*>(ob + (roff + o) * p.C) = r4;
              if (p.out_hl != nullptr) {
                const float f[4] = {r4.x, r4.y, r4.z, r4.w};     // (split4 written out: through the helper, in every form tried,
                bf16x4 h, l;                                      //  dw_slide_kernel<5, 2, 1> is compiled to another stream)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                  const __bf16 hb = (__bf16)f[e];
                  h[e] = hb;
                  l[e] = (__bf16)(f[e] - (float)hb);
                }
                __bf16* d = ohb + (roff + o) * 2 * p.C;
                *reinterpret_cast<bf16x4*>(d) = h;
                *reinterpret_cast<bf16x4*>(d + 32) = l;
              }
              sum.x += r4.x; sum.y += r4.y; sum.z += r4.z; sum.w += r4.w;
            }
          }
        }
      }
    }
  }
  red[tid] = sum;
  __syncthreads();
  if (pl == 0 && cq < c4n) {
    float4 t = red[q];
    for (int l = 1; l < p.PL; ++l) {
      const float4 u = red[l * p.QL + q];
      t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
    }
    float* dst = p.part + ((b * p.tiles + tile) * (long)p.C) + c;
    *reinterpret_cast<float4*>(dst) = t;
  }
}

// workgroup geometry shared by the size query and the launch
struct DWSGeom { int QL, PL, RY, PX, chunks, wox, nruns, nwork, tiles; };
DWSGeom dws_geom(int B, int C, int Ho, int Wo, int k, int stride) {
  DWSGeom g;
  g.PX = (stride == 1 && k == 3) ? 4 : ((stride == 2 && k == 5) ? 1 : 2);
  const int c4n = C / 4;
  g.chunks = (c4n + 63) / 64;
  g.QL = (c4n + g.chunks - 1) / g.chunks;
  g.PL = 256 / g.QL;
  g.wox = (Wo + g.PX - 1) / g.PX;
  // rows per work item: up to 8 (measured: 16 was slower on the 120 x 160 and 240 x 320 stages, fewer workgroups in
  // flight), shorter while the launch would have fewer than ~800 workgroups (a run re-reads k - stride rows)
  int ry = 8;
  while (ry > 2 && (long)g.wox * ((Ho + ry - 1) / ry) * g.chunks * B < 800L * g.PL) ry >>= 1;
  g.RY = ry;
  g.nruns = (Ho + ry - 1) / ry;
  g.nwork = g.wox * g.nruns;
  g.tiles = (g.nwork + g.PL - 1) / g.PL;
  return g;
}

// ---------------------------------------------------------------------------------------------------------------------
// dw_rows_kernel<S, QLP> (k = 5): every input row of a tile is brought into LDS ONCE and the window is read from there.
// dw_slide_kernel's threads each fetch their own NIN = 6 columns of every input row and every run of RY = 8 output rows
// re-reads K - S rows: 4.5 sixteen-byte loads per output quad at stride 1, all but one of them re-reads (L1 hits on the
// large maps, L2 requests on the deep ones: profiles/dw_lds_rows.txt).  Here a workgroup owns (image, chunk of <= QLP channel quads, tile of
// TW output columns x TH output rows) and one more, producer wavefront stages the tile's footprint (S TW + K - S pixels
// wide) row by row with LDS-DMA (16 bytes per lane, no registers): footprint / tile = (1 + 4 / TW)(1 + 4 / TH) at
// stride 1, TW = 12 or 24: <= 2.25 on every k = 5 shape of the benchmark.
//
// Ring: NB row slots [pixel][QLP quads] (a DMA instruction writes 64 consecutive quads); window row rel of the tile
// lives in slot rel % NB.  ONE raw s_barrier per output row n: the producer arrives once rows <= n S + K - 1 have landed
// (counted vmcnt: the NB - S - K younger rows stay in flight), the consumers once their LDS reads of output row n - 1
// have returned (lgkmcnt(0)); behind it the consumers read the K rows of the window and the producer issues the next S
// rows into the slots of the rows that output row n - 1 was the last to use.  The consumers issue no global loads in
// the loop, so their stores never stand in front of anything they wait for, and the DMA is never issued by a wavefront
// that reads the ring (the compiler would put vmcnt(0) before every LDS read).  Rows / columns outside the image and
// the quads past the chunk come from a zero page: selected addresses.
// Consumers: thread = (quad q, pixel lane pl) as in dw_slide_kernel with its PX output columns, the K x K weights in
// REGISTERS (the window's 100 - 120 registers are free: it stays in LDS), and dw_slide_kernel's arithmetic statement
// for statement (acc = bias, fmaf over r outer / j inner, padded taps multiplied as zeros, fast_silu): out and out_hl
// are bit-identical to its.  part[b][tile][c]: one row per workgroup tile.
struct DWRArgs {
  const float *in, *w, *bias;
  float *out, *part;
  __bf16* out_hl;
  int C, H, W, Ho, Wo, pad_t, pad_l;
  int QL, TH;                      // quads per chunk (<= QLP), output rows per tile
  int nxt, tiles, chunks;          // tiles per output row, tiles per (image, chunk) = nxt x row bands, chunks
};

// consumer wavefronts + the producer; wavefronts per SIMD.  Stride 1 holds 100 weight + 2 x 4 accumulator + 24 row registers
// and gets 256 (two workgroups of 3 + 1 per CU), stride 2 fits 168 (two workgroups of 4 + 1).
constexpr int dwr_threads(int s) { return s == 1 ? 256 : 320; }
constexpr int dwr_waves_per_simd(int s) { return s == 1 ? 2 : 3; }

template <int S, int QLP>
struct DWRShape {
  static constexpr int K = 5, PX = S == 1 ? 2 : 1;
  static constexpr int NCT = dwr_threads(S) - 64;             // consumer threads
  static constexpr int PL = NCT / QLP, TW = PX * PL;
  static constexpr int RW = S * TW + K - S;                   // staged pixels per input row
  static constexpr int NI = (RW * QLP + 63) / 64;             // DMA instructions per row
  static constexpr int ROWE = NI * 64;                        // float4s per staged row
  // ring slots (rows): K under the window + S arriving + the rest ahead, as many as leave room for two workgroups per CU
  static constexpr int NB = S == 1 ? (QLP == 32 ? 9 : 10) : (QLP == 32 ? 7 : 8);
  static constexpr size_t LDS = ((size_t)NB * ROWE + NCT) * sizeof(float4);
  static_assert(2 * LDS <= 160 * 1024, "two workgroups per CU");
};

template <int S, int QLP>
__global__ __launch_bounds__(dwr_threads(S), dwr_waves_per_simd(S)) void dw_rows_kernel(DWRArgs p) {
  using G = DWRShape<S, QLP>;
  constexpr int K = G::K, PX = G::PX, PL = G::PL, NCT = G::NCT, TW = G::TW, RW = G::RW, NI = G::NI, ROWE = G::ROWE, NB = G::NB;
  constexpr int NIN = (PX - 1) * S + K;
  constexpr int AHEAD = NB - S - K;                           // rows still in flight when the producer meets the consumers
  static_assert(NCT % QLP == 0 && 64 % QLP == 0 && AHEAD >= 0 && AHEAD * NI <= 63, "counted vmcnt must fit its 6-bit field");
  extern __shared__ __attribute__((aligned(16))) float4 dwr_sm[];      // ring[NB][ROWE] | red[NCT]
  float4* ring = dwr_sm;
  float4* red = dwr_sm + NB * ROWE;
  const int tid = threadIdx.x;
  const int c4n = p.C >> 2;
  int tile, chunk;
  long b;
  dw_xcd_decode(p.tiles, p.chunks, tile, chunk, b);
  const int band = tile / p.nxt, xt = tile - band * p.nxt;
  const int y0 = band * p.TH, y1 = min(p.Ho, y0 + p.TH);      // one barrier per output row, the same for all five wavefronts
  const int iyb = y0 * S - p.pad_t;                           // input row of window row 0
  const int ixb = xt * TW * S - p.pad_l;                      // input column of staged pixel 0

  if (tid >= NCT) {
    // =========================== PRODUCER wavefront: LDS-DMA issuer ===========================
    const int lane = tid & 63;
    const int qd = lane % QLP, cq = chunk * p.QL + qd;
    const bool qok = qd < p.QL && cq < c4n;
    int coff[NI];                                             // element offset inside an input row, -1 = zero page
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int px = j * (64 / QLP) + lane / QLP, ix = ixb + px;
      coff[j] = qok && px < RW && ix >= 0 && ix < p.W ? ix * p.C + cq * 4 : -1;
    }
    const float* ib = p.in + b * (long)p.H * p.W * p.C;
    const int nrel = (y1 - y0 - 1) * S + K;                   // window rows the tile reads; later ones are zero-page rows
    auto issue = [&](int rel, int slot) {
      const int iy = iyb + rel;
      const bool rok = rel < nrel && iy >= 0 && iy < p.H;
      const float* row = ib + (long)(rok ? iy : 0) * p.W * p.C;
      __attribute__((address_space(3))) float4* dst = (__attribute__((address_space(3))) float4*)ring + slot * ROWE;
#pragma unroll
      for (int j = 0; j < NI; ++j) {
        const float* src = rok && coff[j] >= 0 ? row + coff[j] : ocv_zero_page;
        __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(dst + j * 64), 16, 0, 0);
      }
    };
#pragma unroll
    for (int rel = 0; rel < NB - S; ++rel) issue(rel, rel);
    int slot = NB - S, rel = NB - S;
#pragma unroll 1
    for (int y = y0; y < y1; ++y) {
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(AHEAD * NI) : "memory");          // the window of this output row has landed
      __builtin_amdgcn_s_barrier();                           // ... and the consumers have read the previous one
#pragma unroll
      for (int sidx = 0; sidx < S; ++sidx) {                  // into the slots of the S rows that window left behind
        issue(rel, slot);
        ++rel;
        slot = slot + 1 == NB ? 0 : slot + 1;
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // nothing lands in LDS after the workgroup's last barrier
  } else {
    // =========================== CONSUMERS ===========================
    const int q = tid % QLP, pl = tid / QLP;
    const int cq = chunk * p.QL + q;
    const bool active = q < p.QL && cq < c4n;
    const int c = (active ? cq : 0) * 4;
    const int ox = (xt * PL + pl) * PX;
    const bool act0 = active && ox < p.Wo;                    // threads with no output column only meet the barriers
    const bool ok1 = PX > 1 && ox + 1 < p.Wo;
    float4 wv[K * K];
#pragma unroll
    for (int t = 0; t < K * K; ++t) wv[t] = ld4(p.w + (long)t * p.C + c);
    const float4 bv = p.bias ? ld4(p.bias + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
    const long opix = (b * p.Ho + y0) * (long)p.Wo + ox;
    float* ob = p.out + opix * p.C + c;
    __bf16* ohb = hl_at(p.out_hl, opix, c, p.C);                            // hl32: hi quad here, lo quad 32 elements on
    const float4* rp = ring + pl * PX * S * QLP + q;
    int s0 = 0;                                               // slot of the window's first row
#pragma unroll 1
    for (int y = y0; y < y1; ++y) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      if (act0) {
        float4 acc[PX];
#pragma unroll
        for (int o = 0; o < PX; ++o) acc[o] = bv;
#pragma unroll
        for (int r = 0; r < K; ++r) {
          __builtin_amdgcn_sched_barrier(0);                  // one window row at a time: all K x NIN reads at once cost scratch
          const int t = s0 + r;
          const float4* rr = rp + (t >= NB ? t - NB : t) * ROWE;
          float4 x[NIN];
#pragma unroll
          for (int j = 0; j < NIN; ++j) x[j] = rr[j * QLP];
#pragma unroll
          for (int j = 0; j < K; ++j) {
            const float4 w4 = wv[r * K + j];
#pragma unroll
            for (int o = 0; o < PX; ++o) {
              acc[o] = fma4(w4, x[o * S + j], acc[o]);
            }
          }
        }
        const long roff = (long)(y - y0) * p.Wo;
#pragma unroll
        for (int o = 0; o < PX; ++o) {
          // A second column past the row's end repeats the first column's store (same thread, same address, same value)
          // and adds zero: no branch, so the compiler cannot sink that column's FMAs into one.
          const bool ok = o == 0 || ok1;
          const int oo = ok ? o : 0;
          float4 r4 = silu4(acc[o]);
          if (o > 0) {
            const float4 f4 = silu4(acc[0]);
            r4.x = ok ? r4.x : f4.x; r4.y = ok ? r4.y : f4.y; r4.z = ok ? r4.z : f4.z; r4.w = ok ? r4.w : f4.w;
          }
          if (p.out != nullptr) *reinterpret_cast<float4*>(ob + (roff + oo) * p.C) = r4;
          if (p.out_hl != nullptr) {
            bf16x4 h, l;
            split4(r4, h, l);
            __bf16* d = ohb + (roff + oo) * 2 * p.C;
            *reinterpret_cast<bf16x4*>(d) = h;
            *reinterpret_cast<bf16x4*>(d + 32) = l;
          }
          sum.x += ok ? r4.x : 0.f; sum.y += ok ? r4.y : 0.f; sum.z += ok ? r4.z : 0.f; sum.w += ok ? r4.w : 0.f;
        }
      }
      s0 = s0 + S >= NB ? s0 + S - NB : s0 + S;
    }
    red[tid] = sum;
  }
  __syncthreads();
  if (tid < QLP && tid < p.QL && chunk * p.QL + tid < c4n) {  // pixel lane 0 of every quad of the chunk
    float4 t = red[tid];
    for (int l = 1; l < PL; ++l) {
      const float4 u = red[l * QLP + tid];
      t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
    }
    float* dst = p.part + ((b * p.tiles + tile) * (long)p.C) + (chunk * p.QL + tid) * 4;
    *reinterpret_cast<float4*>(dst) = t;
  }
}

// Geometry of dw_rows_kernel, shared by the size query and the launch.  QLP (the quads a DMA row holds per pixel, which
// fixes the tile width: consumer threads / QLP pixel lanes) is the one of {16, 32} that wastes least:
// lanes past the balanced chunk x columns past the row's end x the halo columns staged per tile column.  Row bands: the
// whole height unless the launch would have fewer than ~1024 workgroups (2 per CU x 256 CUs x 2), never under 8 rows
// (a band re-stages K - S rows).
struct DWRGeom { int QLP, QL, chunks, nxt, TH, tiles; };
DWRGeom dwr_geom(int B, int C, int Ho, int Wo, int stride) {
  DWRGeom g{};
  const int c4n = C / 4, px = stride == 1 ? 2 : 1;
  double best = -1.0;
  for (int qlp = 32; qlp >= 16; qlp >>= 1) {
    const int chunks = (c4n + qlp - 1) / qlp, tw = px * (stride == 1 ? 192 : 256) / qlp, nxt = (Wo + tw - 1) / tw;
    const double eff = (double)c4n / ((double)chunks * qlp) * Wo / ((double)nxt * tw) * (stride * tw) / (stride * tw + 5 - stride);
    if (eff > best * 1.0000001) {
      best = eff;
      g.QLP = qlp;
      g.chunks = chunks;
      g.nxt = nxt;
    }
  }
  g.QL = (c4n + g.chunks - 1) / g.chunks;
  int nb = 1;
  while ((long)B * g.chunks * g.nxt * nb < 1024 && (Ho + nb) / (nb + 1) >= 8) ++nb;
  g.TH = (Ho + nb - 1) / nb;
  g.tiles = g.nxt * ((Ho + g.TH - 1) / g.TH);
  return g;
}

// 0 = automatic, 1 = dw_slide_kernel everywhere, 2 = dw_rows_kernel wherever it is supported (ocv_depthwise_set_dispatch)
int& dw_dispatch() {
  static int mode = 0;
  return mode;
}
// dw_rows_kernel supports k = 5 at both strides (mode 2).  Automatic takes it where it measured faster at bs 16
// (profiles/dw_lds_rows.txt): every stride-1 shape, and stride 2 from 1200 output pixels per image (60 x 80: -9 %;
// 15 x 20: +44 %, the register window stays; nothing in between is measured).  An input row's element offsets are ints:
// decided from the OUTPUT width, which is all the size query knows (W <= stride Wo + k), with a margin for the rest.
bool dw_use_rows(int C, int Ho, int Wo, int k, int stride) {
  const int mode = dw_dispatch();
  if (mode == 1 || k != 5 || ((long)stride * Wo + k) * C >= (1L << 30)) return false;
  return mode == 2 || stride == 1 || (long)Ho * Wo >= 1200;
}

template <int K, int S, int PX>
int launch_dws(const DWSArgs& a, const DWSGeom& g, int B, hipStream_t st) {
  hipLaunchKernelGGL((dw_slide_kernel<K, S, PX>), dim3((unsigned)((long)g.tiles * g.chunks * B)), dim3(256), 0, st, a);
  OCV_CHECK_LAUNCH("ocv_depthwise_conv_nhwc_sum_fwd");
  return 0;
}

template <int S, int QLP>
int launch_dwr(const DWRArgs& a, int B, hipStream_t st) {
  ocv_allow_dynamic_lds<dw_rows_kernel<S, QLP>>();
  constexpr size_t lds = DWRShape<S, QLP>::LDS;
  hipLaunchKernelGGL((dw_rows_kernel<S, QLP>), dim3((unsigned)((long)a.tiles * a.chunks * B)), dim3(dwr_threads(S)), lds, st, a);
  OCV_CHECK_LAUNCH("ocv_depthwise_conv_nhwc_sum_fwd(rows)");
  return 0;
}

}  // namespace

extern "C" int ocv_depthwise_set_dispatch(int mode) {
  OCV_CHECK_ARG(mode >= 0 && mode <= 2, "ocv_depthwise_set_dispatch: mode must be 0 (automatic), 1 (register window) or 2 (LDS rows), got %d", mode);
  dw_dispatch() = mode;
  return 0;
}

extern "C" int ocv_depthwise_sum_tiles(int B, int C, int Ho, int Wo, int k, int stride) {
  if (B < 1 || C < 4 || C % 4 != 0 || Ho < 1 || Wo < 1 || (k != 3 && k != 5) || (stride != 1 && stride != 2)) return 0;
  if (dw_use_rows(C, Ho, Wo, k, stride)) return dwr_geom(B, C, Ho, Wo, stride).tiles;
  return dws_geom(B, C, Ho, Wo, k, stride).tiles;
}

extern "C" int ocv_depthwise_conv_nhwc_sum_fwd(const float* in, const float* w, const float* bias, float* out, float* part,
                                               int B, int C, int H, int W, int k, int stride, int pad_t, int pad_l,
                                               int Ho, int Wo, ocv_stream_t stream) {
  return ocv_depthwise_conv_nhwc_sum_hl_fwd(in, w, bias, out, nullptr, part, B, C, H, W, k, stride, pad_t, pad_l, Ho, Wo, stream);
}

extern "C" int ocv_depthwise_conv_nhwc_sum_hl_fwd(const float* in, const float* w, const float* bias, float* out, void* out_hl,
                                                  float* part, int B, int C, int H, int W, int k, int stride, int pad_t,
                                                  int pad_l, int Ho, int Wo, ocv_stream_t stream) {
  OCV_CHECK_ARG(in && w && (out || out_hl) && part, "ocv_depthwise_conv_nhwc_sum_fwd: null pointer");
  OCV_CHECK_ARG(out_hl == nullptr || (C % 32 == 0 && ocv_aligned16(out_hl)), "ocv_depthwise_conv_nhwc_sum_hl_fwd: the split output needs C to be a multiple of 32 (got %d) and 16-byte alignment", C);
  if (ocv_check_dw_geometry("ocv_depthwise_conv_nhwc_sum_fwd", true, B, C, H, W, k, stride, pad_t, pad_l, Ho, Wo,
                            ocv_aligned16(in) && ocv_aligned16(w) && ocv_aligned16(out) && ocv_aligned16(bias) && ocv_aligned16(part)) != 0)
    return -1;
  hipStream_t st = (hipStream_t)stream;
  if (dw_use_rows(C, Ho, Wo, k, stride)) {
    const DWRGeom r = dwr_geom(B, C, Ho, Wo, stride);
    OCV_CHECK_ARG((long)r.tiles * r.chunks * B < (1L << 31), "ocv_depthwise_conv_nhwc_sum_fwd: too many workgroups");
    OCV_CHECK_ARG((long)W * C < (1L << 31), "ocv_depthwise_conv_nhwc_sum_fwd: input rows of 2^31 elements or more");
    DWRArgs a{in, w, bias, out, part, (__bf16*)out_hl, C, H, W, Ho, Wo, pad_t, pad_l, r.QL, r.TH, r.nxt, r.tiles, r.chunks};
    if (stride == 1) return r.QLP == 32 ? launch_dwr<1, 32>(a, B, st) : launch_dwr<1, 16>(a, B, st);
    return r.QLP == 32 ? launch_dwr<2, 32>(a, B, st) : launch_dwr<2, 16>(a, B, st);
  }
  const DWSGeom g = dws_geom(B, C, Ho, Wo, k, stride);
  OCV_CHECK_ARG((long)g.tiles * g.chunks * B < (1L << 31), "ocv_depthwise_conv_nhwc_sum_fwd: too many workgroups");
  DWSArgs a{in, w, bias, out, part, (__bf16*)out_hl, C, H, W, Ho, Wo, pad_t, pad_l, g.QL, g.PL, g.RY, g.wox, g.nwork, g.tiles, g.chunks};
  if (k == 3 && stride == 1) return launch_dws<3, 1, 4>(a, g, B, st);
  if (k == 3 && stride == 2) return launch_dws<3, 2, 2>(a, g, B, st);
  if (k == 5 && stride == 1) return launch_dws<5, 1, 2>(a, g, B, st);
  return launch_dws<5, 2, 1>(a, g, B, st);
}
