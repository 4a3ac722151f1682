// The convolutions on a PRE-SPLIT ("hl32", conv_tile.hpp) input: the tap ring (conv_split_dma_kernel), the halo-staged dense
// 3 x 3 (conv_halo_dma_kernel), the split-K finish pass, the choice between them, and the entry points
// ocv_conv_nhwc_split*_fwd and ocv_conv3x3_split_packed_taps_fwd.  The split arithmetic is described at the head of
// conv_igemm.hip; the Winograd form (conv_winograd.hip) and the split patch embedding (patch_embed.hip) run their GEMMs
// on conv_split_dma_kernel through ocv_conv_launch.
#include <type_traits>

#include "conv_tile.hpp"

namespace {

// ---------------------------------------------------------------------------
// Pre-split input, LDS-DMA variant.  With the activation already stored as (hi, lo) bf16 the A and B tiles are pure
// copies, so the producers move them global -> LDS with global_load_lds_dwordx4 (no VGPR staging, no ds_write: the
// ablation of the register-staged kernel put 25 % of its time in the ds_write_b128 path).  An LDS-DMA instruction
// writes wave-uniform base + lane x 16 B, i.e. rows cannot be padded; bank conflicts are avoided instead by an XOR
// swizzle of the 16-byte chunk index with (row >> 1) & 3, applied on the SOURCE side (each lane fetches the logical
// chunk that belongs at its linear LDS slot) and on the fragment reads.
// ---------------------------------------------------------------------------
// F16: the operands are fp16 (hi, lo) pairs instead of bf16 ones -- the same bytes through the same LDS-DMA pipeline, the
// MFMA of the other 2-byte type (the Winograd F(4x4, 3x3) GEMM batch of conv_winograd.hip: 22-bit products).
template <bool F16>
__global__ __launch_bounds__(512) void conv_split_dma_kernel(ConvArgs p) {
  extern __shared__ __attribute__((aligned(1024))) unsigned char lds[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  const int ntile = p.mtiles * p.ntiles;
  int wg = ocv_xcd_remap(blockIdx.x, ntile * (p.zflat > 0 ? p.zflat : p.ksplit * p.zbatch));
  const int kz = wg / ntile;                                     // (GEMM of the batch, K part) of this workgroup
  wg -= kz * ntile;
  const int taps = p.ks * p.ks, pad = p.ks >> 1;
  const int nchunk = p.Cp / CBK;
  int zb, ch0, nsteps;
  if (p.zflat > 0) {                                             // steps [s0, s1) of the zbatch GEMMs' chunks laid end to end
    const int S = p.zbatch * nchunk;
    const int s0 = (int)((long)S * kz / p.zflat), s1 = (int)((long)S * (kz + 1) / p.zflat);
    zb = s0 / nchunk;
    ch0 = s0 - zb * nchunk;
    nsteps = s1 - s0;
  } else {
    zb = kz / p.ksplit;                                          // zb: 0 unless zbatch > 1
    const int kh = kz - zb * p.ksplit;                           // kh: 0 unless ksplit == 2
    ch0 = nchunk * kh / p.ksplit;                                // channel chunks [ch0, ch1)
    nsteps = p.gpt > 0 ? p.Kp / CBK : taps * (nchunk * (kh + 1) / p.ksplit - ch0);
  }
  const char* xz = (const char*)p.xhl + (long)zb * p.xz_bytes;   // (advanced by the producers in zflat mode)
  const char* whz = (const char*)p.whi + (long)zb * p.wz_bytes;
  const char* wlz = (const char*)p.wlo + (long)zb * p.wz_bytes;
  const int mt = wg / p.ntiles, nt = wg - mt * p.ntiles;
  const long m0 = (long)mt * CBM;
  const int n0 = nt * CBN;
  const long yoff = (long)kz * p.M * p.Cout;
  auto rowm = [m0](int R) { return m0 + R; };                    // tile row -> output pixel: 256 flat-consecutive pixels

  if (wave < 4) {
    // =========================== CONSUMERS, v_mfma_f32_16x16x32_bf16 ===========================
    // 2 x 2 over the tile, 128 x 64 outputs each (32 accumulators of 16 x 16); per step 24 ds_read_b128 and 96 MFMAs.
    // The 16 x 16 x 32 shape costs the same matrix-pipe cycles as 48 of 32 x 32 x 16 over the same LDS image and the
    // same reads, but the chip sustains a higher clock under it: A/B in one process on one device, 3-9 % faster per
    // launch (2224 -> 1024 at 30 x 40: 2.55 -> 2.33 ms).  Operand lanes: row / column l & 15, K octet l >> 4 (one
    // 16-byte chunk of the 64-byte row).  Swizzle key (row >> 1) & 3: any 8 consecutive rows of one K octet land in
    // 8 different 16-byte bank groups of a 128-byte LDS cycle.  (With the key (row >> 2) & 3 of the 32 x 32 consumers
    // this read pattern counted 1.4e8 SQ_LDS_BANK_CONFLICT cycles per launch and ran 1-3.5 % slower.)
    const int wm = wave >> 1, wn = wave & 1;
    const int l15 = lane & 15, q4 = lane >> 4;
    const int co = ((q4 ^ ((l15 >> 1) & 3)) * 16);
    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    __syncthreads();
    for (int step = 0; step < nsteps; ++step) {
      const unsigned char* base = lds + (step % DNBUF) * DBUF;
      const unsigned char* pa = base + (wm * 128 + l15) * DROW + co;
      const unsigned char* pb = base + 2 * DA + (wn * 64 + l15) * DROW + co;
      bf16x8 ah[8], al[8], bh[4], bl[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        bh[j] = *reinterpret_cast<const bf16x8*>(pb + j * 16 * DROW);
        bl[j] = *reinterpret_cast<const bf16x8*>(pb + DB + j * 16 * DROW);
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        ah[i] = *reinterpret_cast<const bf16x8*>(pa + i * 16 * DROW);
        al[i] = *reinterpret_cast<const bf16x8*>(pa + DA + i * 16 * DROW);
      }
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) mma3<F16>(ah[i], al[i], bh[j], bl[j], acc[i][j]);
      __syncthreads();
    }

    // ---- epilogue (conv_tile.hpp): through LDS and out from all eight wavefronts, or element-wise from this one
    if ((p.Cout & 7) == 0) {
      // (written out in both kernels: behind a helper that takes the accumulator array by reference the compiler lays out the
      // whole kernel differently -- 69 more instructions -- and the tap ring measured 0.65 % slower: profiles/conv_tile_refactor.txt)
      float* tile = reinterpret_cast<float*>(lds) + wave * (128 * ERS);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) tile[(16 * i + 4 * q4 + r) * ERS + 16 * j + l15] = acc[i][j][r];
      __syncthreads();
      conv_store_rows<F16>(p, lds, wave, lane, rowm, n0, yoff);
    } else {
      conv_store_elems<F16>(p, acc, rowm, (int)min((long)CBM, p.M - m0), wm, wn, lane, n0, yoff);
    }
    return;
  }

  // =========================== PRODUCERS (LDS-DMA issuers) ===========================
  // wave pw moves A rows [64 pw, 64 pw + 64) (hi and lo: 8 x 1 KiB pieces) and B rows [32 pw, 32 pw + 32) (4 pieces).
  // Lane L of a piece lands at piece base + 16 L  =  row L >> 2, stored chunk L & 3, which must hold LOGICAL chunk
  // (L & 3) ^ ((row >> 1) & 3) = (L & 3) ^ ((L >> 3) & 3)  (piece bases are multiples of 16 rows).
  const int pw = wave - 4;
  const int lrow = lane >> 2;
  const int lchunk = (lane & 3) ^ ((lane >> 3) & 3);               // logical 16-byte chunk (8 channels) this lane fetches
  // (32-bit arithmetic and no division by the runtime kernel size: the 64-bit % and / of a first version, eight per
  // lane plus two per tap, were most of a 14 K-cycle prologue in front of every tile's first load)
  unsigned rbA[4], tapmask[4];
  {
    const unsigned hw = (unsigned)(p.H * p.W);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned am = (unsigned)m0 + 64 * pw + 16 * i + lrow;           // M < 2^30 (4 GiB operand limit)
      const bool valid = am < (unsigned)p.M;
      const unsigned img = valid ? am / hw : 0u;
      const unsigned rem = valid ? am - img * hw : 0u;
      const int y = (int)(rem / (unsigned)p.W), x = (int)(rem - (unsigned)y * (unsigned)p.W);
      unsigned mask = 0;
      int t = 0;
      for (int dy = -pad; dy <= pad; ++dy)
        for (int dx = -pad; dx <= pad; ++dx, ++t)
          if (valid && (unsigned)(y + dy) < (unsigned)p.H && (unsigned)(x + dx) < (unsigned)p.W) mask |= 1u << t;
      tapmask[i] = mask;
      rbA[i] = (p.rowpitch == 0 ? (valid ? am : 0u) * (unsigned)(4 * p.Cp)
                                : (img * (unsigned)p.H + (unsigned)y) * p.rowpitch + (unsigned)x * (unsigned)(4 * p.Cp)) +
               (unsigned)(lchunk * 16);
    }
  }
  unsigned rbB[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int bn = min(n0 + 32 * pw + 16 * i + lrow, p.Cout - 1);
    rbB[i] = (unsigned)(((long)bn * (p.gpt > 0 ? p.Kp : p.Cp) + lchunk * 8) * 2);
  }
  const unsigned wtap = (unsigned)((long)p.Cout * p.Cp * 2);

  // PACKED TAPS: this lane's granule of step s is G = 4 s + lchunk = (tap, granule cg of the tap's pixel); tap and cg differ between
  // the four lanes of a row, so the tap shift and the in-image test are per lane (a dozen VALU instructions per step on wavefronts
  // that otherwise only issue DMA).  Granules beyond the ninth tap (the K padding of the last step) read the zero page; the
  // weights hold zeros there.
  int nx_pk = 0;
  auto issue_dma_packed = [&](int buf) {
    const int G = 4 * nx_pk + lchunk;
    const int tap_raw = (int)(((unsigned)G * (unsigned)p.gpt_inv) >> 16);
    const int cg = G - tap_raw * p.gpt;
    const bool in_k = tap_raw < 9;
    const int tap = in_k ? tap_raw : 8;
    const int ky = (tap * 11) >> 5, kx = tap - 3 * ky;                  // tap / 3 for tap <= 8
    // rbA carries lchunk * 16 (the dense layout's granule of this lane): replaced by the packed granule's place in its pixel
    const int soff = ((ky - 1) * p.W + (kx - 1)) * 4 * p.Cp + (cg >> 2) * 128 + (cg & 3) * 16 - lchunk * 16;
    unsigned char* base = lds + buf * DBUF;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool ok = in_k && ((tapmask[i] >> tap) & 1u);
      const unsigned off = rbA[i] + (unsigned)soff;
      const void* sh = ok ? (const void*)(xz + off) : (const void*)ocv_zero_page;
      const void* sl = ok ? (const void*)(xz + off + 64) : (const void*)ocv_zero_page;
      unsigned char* dst = base + (64 * pw + 16 * i) * DROW;
      __builtin_amdgcn_global_load_lds((gptr_t)sh, (lptr_t)dst, 16, 0, 0);
      __builtin_amdgcn_global_load_lds((gptr_t)sl, (lptr_t)(dst + DA), 16, 0, 0);
    }
    conv_issue_weights(whz, wlz, (unsigned)nx_pk * (CBK * 2), rbB, base + 2 * DA, pw);
    ++nx_pk;
  };

  int nx_tap = 0, nx_c0 = ch0 * CBK, nx_ky = 0, nx_kx = 0;
  auto issue_dma_dense = [&](int buf) {
    const int tap = nx_tap, c0 = nx_c0, ky = nx_ky, kx = nx_kx;
    const char* const xz_ = xz;
    const char* const whz_ = whz;
    const char* const wlz_ = wlz;
    if (++nx_kx == p.ks) { nx_kx = 0; ++nx_ky; }
    if (++nx_tap == taps) { nx_tap = 0; nx_ky = 0; nx_c0 += CBK; }
    if (p.zflat > 0 && nx_c0 == p.Cp) {                          // next step: first chunk of the next GEMM of the batch
      nx_c0 = 0;
      xz += p.xz_bytes; whz += p.wz_bytes; wlz += p.wz_bytes;
    }
    const int soff = (((ky - pad) * p.W + (kx - pad)) * 2 * p.Cp + 2 * c0) * 2;       // hl32: chunk c0 starts at 2 c0
    unsigned char* base = lds + buf * DBUF;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool ok = ((tapmask[i] >> tap) & 1u);               // pad channels are zeros in memory: no channel check
      const unsigned off = rbA[i] + (unsigned)soff;
      const void* sh = ok ? (const void*)(xz_ + off) : (const void*)ocv_zero_page;
      const void* sl = ok ? (const void*)(xz_ + off + 64) : (const void*)ocv_zero_page;   // same 128-B line
      unsigned char* dst = base + (64 * pw + 16 * i) * DROW;
      __builtin_amdgcn_global_load_lds((gptr_t)sh, (lptr_t)dst, 16, 0, 0);
      __builtin_amdgcn_global_load_lds((gptr_t)sl, (lptr_t)(dst + DA), 16, 0, 0);
    }
    conv_issue_weights(whz_, wlz_, (unsigned)tap * wtap + (unsigned)c0 * 2, rbB, base + 2 * DA, pw);
  };

  auto issue_dma = [&](int buf) {
    if (p.gpt > 0) issue_dma_packed(buf);                         // (uniform: a scalar branch)
    else issue_dma_dense(buf);
  };

  // Three LDS buffers, DMA two K steps ahead: in interval t (consumers on buffer t % 3) the producers issue step t+2
  // into buffer (t+2) % 3 -- last read in interval t-1, free since the previous barrier -- and then only wait for step
  // t+1, issued a whole interval earlier: a COUNTED s_waitcnt vmcnt(12) (this wave's 12 newest pieces may stay in
  // flight) followed by a raw s_barrier; __syncthreads() would emit vmcnt(0) and drain the young pieces too.  An
  // LDS-DMA has no register destination, so hand-counting it carries none of the register-copy hazard described at
  // gload16().
  issue_dma(0);
  if (nsteps > 1) {
    issue_dma(1);
    ocv_wait_vm<12>();
  } else {
    ocv_wait_vm<0>();
  }
  __builtin_amdgcn_s_barrier();
  for (int t = 0; t < nsteps; ++t) {
    if (t + 2 < nsteps) {
      issue_dma((t + 2) % DNBUF);
      ocv_wait_vm<12>();                               // step t+1 has landed, step t+2 may still be in flight
    } else {
      ocv_wait_vm<0>();
    }
    __builtin_amdgcn_s_barrier();
  }
  if ((p.Cout & 7) == 0) {                             // the consumers park their accumulators in LDS; all eight waves store
    __syncthreads();
    conv_store_rows<F16>(p, lds, wave, lane, rowm, n0, yoff);
  }
}

// ---------------------------------------------------------------------------
// HALO-STAGED form of the dense 3 x 3 "same" convolution on a pre-split input (ks = 3, stride 1, ksplit = zbatch = 1, no
// packed taps; H % 8 == 0, W % 32 == 0).  conv_split_dma_kernel tiles M as 256 flat-consecutive pixels and stages a complete
// 256-row image of A for each of the nine taps of a 32-channel chunk: nine copies of the same pixels shifted by a row or
// a column, 288 one-KiB pieces where the distinct pixels fill 44.  Here a workgroup is one image-aligned 8 x 32 pixel
// patch x 128 output channels, and per chunk the producers stage the (8 + 2) x (32 + 2) HALO patch ONCE:
//   LDS  A[2] (one per chunk parity): hi plane, lo plane, each 10 halo rows x 40 pixels (34 used) x 64 B = 25 600 B
//        W[3] the weights' ring of one tap step each, as in conv_split_dma_kernel (hi 8 KiB, lo 8 KiB)
//        2 x 51 200 + 3 x 16 384 = 151 552 B (the parked-accumulator epilogue uses the first 139 264 B, as there)
//   tap (ky, kx): the fragment of tile pixel (ty, tx) is the LDS row (ty + ky) x 40 + tx + kx of the chunk's patch.
//   Swizzle: stored 16-byte chunk = logical chunk ^ ((row >> 1) & 3), row = the LDS row.  A fragment read covers 16
//   consecutive rows from ANY start (40 and 16 are multiples of 8: row & 7 = (tx + kx) & 7 whatever ty, ky and the
//   fragment), and (row & 1) x 4 + (chunk ^ ((row >> 1) & 3)) runs over all eight 16-byte bank groups on any eight
//   consecutive rows: conflict-free for all nine taps, and the key of a lane depends on kx alone (three pointers).
// Pixels outside the image, and the six pad pixels of a halo row, come from ocv_zero_page: one mask bit per halo pixel
// a lane fetches (it fetches the same 13 of them for every chunk).  Same eight specialised wavefronts, same MFMA sequence
// per step (chunk outer, tap inner, hi hi / hi lo / lo hi) into the same accumulators: BIT-IDENTICAL results.  Patches run
// in row-major order and the N-tiles of a patch share an XCD, so that neighbouring halos meet in L2.
// ---------------------------------------------------------------------------
constexpr int HTY = 8, HTX = 32, HPITCH = 40;                       // patch, LDS pixels per halo row
constexpr int HROWS = (HTY + 2) * HPITCH;                           // 400 LDS rows per plane
constexpr int HPLANE = HROWS * DROW, HABUF = 2 * HPLANE;            // 25600, 51200
constexpr int HPIECES = 2 * HROWS / 16;                             // 50 one-KiB pieces per chunk (16 LDS rows of the hi or of the lo plane)
constexpr int HAPW = (HPIECES + 3) / 4;                             // 13 per producer wavefront (the last two of 52 repeat piece 49)
constexpr int HW0 = 2 * HABUF, HWSLOT = 2 * DB;                     // weights' ring: offset 102400, 16384 per slot
constexpr int HLDS = HW0 + DNBUF * HWSLOT;                          // 151552
static_assert(HROWS % 16 == 0 && HLDS <= 160 * 1024 && 4 * 128 * ERS * 4 <= HLDS, "conv_halo_dma_kernel: LDS budget");
// A pieces of the NEXT chunk a producer wavefront issues beside tap step T's weight pieces: 2 2 2 2 2 1 1 1 0 = 13
__host__ __device__ constexpr int halo_na(int T) { return T < 5 ? 2 : (T < 8 ? 1 : 0); }
__host__ __device__ constexpr int halo_a0(int T) { return T < 5 ? 2 * T : 5 + T; }        // the first of them
static_assert(halo_a0(8) == HAPW && halo_a0(7) + halo_na(7) == HAPW, "conv_halo_dma_kernel: A pieces per chunk");

template <bool F16>
__global__ __launch_bounds__(512) void conv_halo_dma_kernel(ConvArgs p) {
  extern __shared__ __attribute__((aligned(1024))) unsigned char lds[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wg = ocv_xcd_remap(blockIdx.x, p.mtiles * p.ntiles);
  const int nchunk = p.Cp / CBK, nsteps = 9 * nchunk;
  const int mt = wg / p.ntiles, nt = wg - mt * p.ntiles;
  const int n0 = nt * CBN;
  const int ppr = p.W / HTX, ppi = (p.H / HTY) * ppr;               // patches per patch row, per image
  const int img = mt / ppi, prem = mt - img * ppi;
  const int ty0 = (prem / ppr) * HTY, tx0 = (prem % ppr) * HTX;     // the patch's first pixel in its image
  const long mbase = ((long)img * p.H + ty0) * p.W + tx0;
  const int Wd = p.W;
  auto rowm = [mbase, Wd](int R) { return mbase + (long)(R >> 5) * Wd + (R & 31); };      // tile row R = 32 ty + tx

  if (wave < 4) {
    // =========================== CONSUMERS: the MFMA sequence of conv_split_dma_kernel ===========================
    // Fragment i of consumer (wm, wn) = tile rows 128 wm + 16 i + l15 = patch pixel (4 wm + (i >> 1), 16 (i & 1) + l15).
    const int wm = wave >> 1, wn = wave & 1;
    const int l15 = lane & 15, q4 = lane >> 4;
    unsigned aofs[3];                                               // per kx: this lane's byte offset in a plane, fragment 0, ky = 0
#pragma unroll
    for (int kx = 0; kx < 3; ++kx)
      aofs[kx] = (unsigned)(((wm * 4) * HPITCH + l15 + kx) * DROW + ((q4 ^ (((l15 + kx) >> 1) & 3)) * 16));
    const unsigned char* pbw = lds + HW0 + (wn * 64 + l15) * DROW + ((q4 ^ ((l15 >> 1) & 3)) * 16);
    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    __syncthreads();
    for (int c = 0; c < nchunk; ++c) {
      const unsigned char* abuf = lds + (c & 1) * HABUF;
#pragma unroll 1
      for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {                            // step 9 c + 3 ky + kx reads weight slot (step % 3) = kx
          const unsigned char* pa = abuf + ky * (HPITCH * DROW) + aofs[kx];
          const unsigned char* pb = pbw + kx * HWSLOT;
          bf16x8 ah[8], al[8], bh[4], bl[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            bh[j] = *reinterpret_cast<const bf16x8*>(pb + j * 16 * DROW);
            bl[j] = *reinterpret_cast<const bf16x8*>(pb + DB + j * 16 * DROW);
          }
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            ah[i] = *reinterpret_cast<const bf16x8*>(pa + ((i >> 1) * HPITCH + (i & 1) * 16) * DROW);
            al[i] = *reinterpret_cast<const bf16x8*>(pa + HPLANE + ((i >> 1) * HPITCH + (i & 1) * 16) * DROW);
          }
#pragma unroll
          for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) mma3<F16>(ah[i], al[i], bh[j], bl[j], acc[i][j]);
          __syncthreads();
        }
      }
    }

    // ---- epilogue: as conv_split_dma_kernel, with the patch's tile-row -> pixel map
    if ((p.Cout & 7) == 0) {
      // (written out in both kernels: behind a helper that takes the accumulator array by reference the compiler lays out the
      // whole kernel differently -- 69 more instructions -- and the tap ring measured 0.65 % slower: profiles/conv_tile_refactor.txt)
      float* tile = reinterpret_cast<float*>(lds) + wave * (128 * ERS);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) tile[(16 * i + 4 * q4 + r) * ERS + 16 * j + l15] = acc[i][j][r];
      __syncthreads();
      conv_store_rows<F16>(p, lds, wave, lane, rowm, n0, 0L);
    } else {
      conv_store_elems<F16>(p, acc, rowm, CBM, wm, wn, lane, n0, 0L);         // (whole patches: every tile row has a pixel)
    }
    return;
  }

  // =========================== PRODUCERS (LDS-DMA issuers) ===========================
  // A: piece q of a chunk = plane q & 1 (hi, lo), LDS rows [16 (q >> 1), +16) of it; wavefront pw owns pieces 4 j + pw,
  // j < 13 (52 slots for 50 pieces: slots 50 and 51 fetch piece 49 a second time -- the same bytes to the same place).
  // The hi and the lo half of a pixel's 128-byte line are fetched by two wavefronts in the same step, so that the second
  // can hit in L1.  Lane L of a piece is LDS row 16 (q >> 1) + (L >> 2) = halo pixel (row / 40, row % 40), stored chunk L & 3 = logical chunk
  // (L & 3) ^ ((L >> 3) & 3) (piece bases are multiples of 16 rows).  The lane's source offsets and in-image bits do not
  // depend on the chunk: computed once.  B: rows [32 pw, +32) of the step's weights, 4 pieces, as conv_split_dma_kernel.
  const int pw = wave - 4;
  const int lrow = lane >> 2;
  const int lchunk = (lane & 3) ^ ((lane >> 3) & 3);
  unsigned aoff[HAPW], amask = 0, adst[HAPW];
#pragma unroll
  for (int j = 0; j < HAPW; ++j) {
    const int q = min(4 * j + pw, HPIECES - 1);
    const int plane = q & 1, pc = q >> 1;
    const int hp = pc * 16 + lrow, hy = hp / HPITCH, hx = hp - hy * HPITCH;
    const int y = ty0 - 1 + hy, x = tx0 - 1 + hx;
    const bool ok = hx < HTX + 2 && (unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W;
    aoff[j] = (((unsigned)img * (unsigned)p.H + (unsigned)y) * (unsigned)p.W + (unsigned)x) * (unsigned)(4 * p.Cp) +
              (unsigned)(plane * 64 + lchunk * 16);                 // (operands are below 4 GiB; unused where !ok)
    amask |= ok ? 1u << j : 0u;
    adst[j] = (unsigned)(plane * HPLANE + pc * 1024);               // wave-uniform
  }
  unsigned rbB[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int bn = min(n0 + 32 * pw + 16 * i + lrow, p.Cout - 1);
    rbB[i] = (unsigned)(((long)bn * p.Cp + lchunk * 8) * 2);
  }
  const unsigned wtap = (unsigned)((long)p.Cout * p.Cp * 2);
  const char* xz = (const char*)p.xhl;
  const char* whz = (const char*)p.whi;
  const char* wlz = (const char*)p.wlo;

  auto issue_a = [&](int j, int c) {                                // piece j of this wavefront, chunk c (j: a constant after unrolling)
    const void* src = ((amask >> j) & 1u) ? (const void*)(xz + aoff[j] + (unsigned)c * 128u) : (const void*)ocv_zero_page;
    __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(lds + (c & 1) * HABUF + adst[j]), 16, 0, 0);
  };
  auto issue_w = [&](int tap, int c) {                              // the weights of step 9 c + tap into slot tap % 3
    conv_issue_weights(whz, wlz, (unsigned)tap * wtap + (unsigned)c * (CBK * 2), rbB, lds + HW0 + (tap % 3) * HWSLOT, pw);
  };

  // Interval s = 9 c + T (consumers on weight slot T % 3 and A buffer c & 1).  The producers issue, in this order,
  //   halo_na(T) A pieces of chunk c + 1 into A buffer (c + 1) & 1 -- last read in chunk c - 1, free since the barrier that
  //                                                                  opened chunk c
  //   the 4 weight pieces of step s + 2 into slot (s + 2) % 3       -- last read in interval s - 1
  // and then wait for step s + 1's weights, issued a whole interval earlier: everything but this interval's own pieces,
  //   T = 0..4  vmcnt(6)   T = 5..7  vmcnt(5)   T = 8  vmcnt(4)     (4 where there is no next chunk, 0 on the last two steps)
  // followed by a raw s_barrier.  At T = 8 only the weights of s + 2 stay in flight: every A piece of chunk c + 1 (issued
  // at T <= 7) has landed before the barrier behind which the consumers first read it.
  auto step = [&](auto tc, int c) {
    constexpr int T = decltype(tc)::value;
    const bool nxt = c + 1 < nchunk;
    if (nxt) {
#pragma unroll
      for (int k = 0; k < halo_na(T); ++k) issue_a(halo_a0(T) + k, c + 1);
    }
    if (9 * c + T + 2 < nsteps) {
      issue_w((T + 2) % 9, c + (T + 2) / 9);
      if (nxt) ocv_wait_vm<4 + halo_na(T)>();
      else ocv_wait_vm<4>();
    } else {
      ocv_wait_vm<0>();
    }
    __builtin_amdgcn_s_barrier();
  };

  // prologue: all of chunk 0's A, the weights of steps 0 and 1; step 1's may stay in flight
#pragma unroll
  for (int j = 0; j < HAPW; ++j) issue_a(j, 0);
  issue_w(0, 0);
  issue_w(1, 0);
  ocv_wait_vm<4>();
  __builtin_amdgcn_s_barrier();
  for (int c = 0; c < nchunk; ++c) {
    step(std::integral_constant<int, 0>{}, c);
    step(std::integral_constant<int, 1>{}, c);
    step(std::integral_constant<int, 2>{}, c);
    step(std::integral_constant<int, 3>{}, c);
    step(std::integral_constant<int, 4>{}, c);
    step(std::integral_constant<int, 5>{}, c);
    step(std::integral_constant<int, 6>{}, c);
    step(std::integral_constant<int, 7>{}, c);
    step(std::integral_constant<int, 8>{}, c);
  }
  if ((p.Cout & 7) == 0) {                             // the consumers park their accumulators in LDS; all eight waves store
    __syncthreads();
    conv_store_rows<F16>(p, lds, wave, lane, rowm, n0, 0L);
  }
}


// Second pass of a split-K convolution: y = act(part0 + part1 + bias) (+ residual), fp32 and / or hl32 split output.
// One thread per (pixel, channel octet); fixed summation order.
struct FinArgs {
  const float *part, *bias, *res;
  float* y;
  __bf16* yhl;
  long M, items;         // items = M * Cout / 8
  int Cout, Cpo, act, ksplit;
  const float* oscale;   // nullable [Cout] (ConvArgs::oscale)
  int f16;               // element type of yhl
  unsigned* range_flag;  // nullable (ConvArgs::range_flag)
};

__global__ __launch_bounds__(256) void conv_splitk_finish_kernel(FinArgs p) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.items) return;
  const int noct = p.Cout >> 3;
  const long m = i / noct;
  const int n = (int)(i - m * noct) * 8;
  const long o = m * p.Cout + n;
  f32x4 a = *reinterpret_cast<const f32x4*>(p.part + o), c = *reinterpret_cast<const f32x4*>(p.part + o + 4);
  for (int k = 1; k < p.ksplit; ++k) {
    a += *reinterpret_cast<const f32x4*>(p.part + k * p.M * p.Cout + o);
    c += *reinterpret_cast<const f32x4*>(p.part + k * p.M * p.Cout + o + 4);
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    a[e] = conv_act(fmaf(a[e], p.oscale != nullptr ? p.oscale[n + e] : 1.f, p.bias != nullptr ? p.bias[n + e] : 0.f), p.act);
    c[e] = conv_act(fmaf(c[e], p.oscale != nullptr ? p.oscale[n + 4 + e] : 1.f, p.bias != nullptr ? p.bias[n + 4 + e] : 0.f), p.act);
  }
  if (p.res != nullptr) {
    a += *reinterpret_cast<const f32x4*>(p.res + o);
    c += *reinterpret_cast<const f32x4*>(p.res + o + 4);
  }
  if (p.y != nullptr) {
    *reinterpret_cast<f32x4*>(p.y + o) = a;
    *reinterpret_cast<f32x4*>(p.y + o + 4) = c;
  }
  if (p.yhl != nullptr) {
    __attribute__((aligned(16))) unsigned short hi[8], lo[8];
    split4_bits(a, hi, lo, p.f16 != 0);
    split4_bits(c, hi + 4, lo + 4, p.f16 != 0);
    if (p.f16 != 0) ocv_range_note(p.range_flag, ocv_amax4(ocv_amax4(0.f, a), c));
    const long oh = hl_index(m, n, p.Cpo);
    *reinterpret_cast<bf16x8*>(p.yhl + oh) = *reinterpret_cast<bf16x8*>(hi);
    *reinterpret_cast<bf16x8*>(p.yhl + oh + 32) = *reinterpret_cast<bf16x8*>(lo);
  }
}

// Split-K pays when the tile count leaves the last round of workgroups mostly empty: 600 tiles on 256 CUs run three
// rounds for 2.34 rounds of work; as 1200 half-K workgroups they run five half-rounds = 2.5.  Returns 1 or 2.
constexpr int KSPLIT_MIN_STEPS = 128;           // split-K is considered from this many K steps on
int conv_ksplit(long M, int Cout, int Cin, int ksize) {
  const long tiles = (long)ocv_cdiv(M, CBM) * ocv_cdiv(Cout, CBN);
  const int nsteps = ksize * ksize * ((Cin + CBK - 1) / CBK);
  if ((Cout & 7) != 0 || nsteps < KSPLIT_MIN_STEPS || tiles <= 256) return 1;
  const double c1 = (double)((tiles + 255) / 256), c2 = (double)((2 * tiles + 255) / 256) / 2.0;
  return c2 <= 0.9 * c1 ? 2 : 1;
}
// 0 = automatic, 1 = conv_split_dma_kernel (the tap ring) everywhere, 2 = conv_halo_dma_kernel, an error where it cannot run
// (ocv_conv3x3_set_dispatch)
int g_conv3x3_dispatch = 0;

// The dense 3 x 3 layers that automatic dispatch gives to conv_halo_dma_kernel: those measured faster than the tap ring
// by the project's rule (every run faster, by more than twice the run-to-run spread; profiles/conv_halo.txt), keyed on
// (H, W, Cin, Cout).  The batch is not part of the key: both kernels run B H W / 256 workgroups of the same K length, so
// the grid scales with B under either and the per-workgroup difference is what was measured (at B = 16 by the rule; at
// B = 4 and 8 every run was faster too, three of those four cells by the rule: same file).
bool conv_halo_auto(int /*B*/, int H, int W, int Cin, int Cout) {
  static const int won[][4] = {{240, 320, 128, 128}, {120, 160, 256, 256}};
  for (const auto& s : won)
    if (H == s[0] && W == s[1] && Cin == s[2] && Cout == s[3]) return true;
  return false;
}
int g_conv3x3_last_kernel = 0;                  // ocv_conv3x3_last_kernel

// the kernels of one element type
template <bool F16>
void launch_conv_kernel(const ConvArgs& a, hipStream_t st) {
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)conv_split_dma_kernel<F16>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute((const void*)conv_halo_dma_kernel<F16>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr = true;
  }
  if (a.halo) {                                   // M = 256 x patches exactly (H % 8 == 0, W % 32 == 0): mtiles is the patch count
    hipLaunchKernelGGL(conv_halo_dma_kernel<F16>, dim3(a.mtiles * a.ntiles), dim3(512), HLDS, st, a);
  } else {
    const unsigned parts = a.zflat > 0 ? a.zflat : a.ksplit * a.zbatch;
    hipLaunchKernelGGL(conv_split_dma_kernel<F16>, dim3(a.mtiles * a.ntiles * parts), dim3(512), DNBUF * DBUF, st, a);
  }
}
}  // namespace

// conv_split_dma_kernel (pre-split input), or conv_halo_dma_kernel where the entry point chose it (ConvArgs::halo)
int ocv_conv_launch(ConvArgs& a, int B, hipStream_t st) {
  a.Cp = (a.Cin + CBK - 1) / CBK * CBK;
  a.M = (long)B * a.H * a.W;
  a.mtiles = ocv_cdiv(a.M, CBM); a.ntiles = ocv_cdiv(a.Cout, CBN);
  if (a.ks == 3 && a.gpt == 0) g_conv3x3_last_kernel = a.halo ? 2 : 1;
  if (a.ksplit < 1) a.ksplit = 1;
  if (a.zbatch < 1) a.zbatch = 1;
  if (a.f16) launch_conv_kernel<true>(a, st);
  else launch_conv_kernel<false>(a, st);
  OCV_CHECK_LAUNCH("ocv_conv_nhwc");
  return 0;
}

extern "C" size_t ocv_split_act_elems(int B, int H, int W, int C) {
  if (B < 1 || H < 1 || W < 1 || C < 1) return 0;
  return (size_t)B * H * W * 2 * ((C + 31) / 32 * 32);
}

namespace {
// What the dense and the packed-taps entry points share: the operands and sizes of one convolution on a pre-split input, the armed
// range guard, and the zeroing of the split output's pad channels.  0 / hipError_t of that zero-fill.
int fill_split_args(ConvArgs& a, const void* x_hl, int Cin, const void* w_hi, const void* w_lo, const float* oscale, int f16,
                    const float* bias, const float* residual, float* y, void* y_hl, int B, int H, int W, int Cout, int ksize, int act,
                    hipStream_t st) {
  a.xhl = (const __bf16*)x_hl; a.yhl = (__bf16*)y_hl; a.Cpo = (Cout + 31) / 32 * 32;
  a.whi = (const __bf16*)w_hi; a.wlo = (const __bf16*)w_lo; a.bias = bias; a.res = residual; a.y = y;
  a.C1 = Cin; a.C2 = 0; a.Cin = Cin; a.Cout = Cout; a.H = H; a.W = W; a.ks = ksize; a.act = act; a.ksplit = 1;
  a.f16 = f16; a.oscale = oscale;
  a.range_flag = (f16 && y_hl != nullptr) ? ocv_range_flag_current() : nullptr;
  if (y_hl != nullptr && Cout % 32 != 0)         // the kernels write channels < Cout only: pad channels must read as zero
    return ocv_zero_async(y_hl, ocv_split_act_elems(B, H, W, Cout) * sizeof(__bf16), st);          // (a launch, not a memset node: common.hpp)
  return 0;
}
}  // namespace

extern "C" size_t ocv_conv_nhwc_split_workspace_bytes(int B, int H, int W, int Cin, int Cout, int ksize) {
  if (B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || (ksize != 1 && ksize != 3)) return 0;
  const long M = (long)B * H * W;
  const int ks = conv_ksplit(M, Cout, Cin, ksize);
  return ks > 1 ? (size_t)ks * M * Cout * sizeof(float) : 0;
}

// conv_halo_dma_kernel: whether it can run a dense 3 x 3 "same" convolution of this shape (pure host arithmetic) -- whole
// 8 x 32 patches, the operand limits of ocv_conv_nhwc_split_x_fwd, and a K axis below the length from which that entry
// point considers split-K (9 x ceil(Cin / 32) < KSPLIT_MIN_STEPS, the threshold of conv_ksplit).
extern "C" int ocv_conv3x3_halo_supported(int B, int H, int W, int Cin, int Cout) {
  if (B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1) return 0;
  if (H % HTY != 0 || W % HTX != 0 || 9 * ((Cin + CBK - 1) / CBK) >= KSPLIT_MIN_STEPS) return 0;
  if ((long)B * H * W * (Cin + 32) * 4 >= (1L << 32) || 9L * Cout * (Cin + 32) * 2 >= (1L << 32)) return 0;
  return 1;
}

extern "C" size_t ocv_conv3x3_halo_lds_bytes(void) { return (size_t)HLDS; }

// 1 = conv_split_dma_kernel, 2 = conv_halo_dma_kernel: the kernel the last dense (not packed-tap) 3 x 3 launch of this
// process ran; 0 before the first.  Tests / tools only.
extern "C" int ocv_conv3x3_last_kernel(void) { return g_conv3x3_last_kernel; }

extern "C" int ocv_conv3x3_set_dispatch(int mode) {
  OCV_CHECK_ARG(mode >= 0 && mode <= 2, "ocv_conv3x3_set_dispatch: mode must be 0 (automatic), 1 (tap ring) or 2 (halo-staged), got %d", mode);
  g_conv3x3_dispatch = mode;
  return 0;
}

extern "C" int ocv_conv_nhwc_split_x_fwd(const void* x_hl, int Cin, const void* w_hi, const void* w_lo, const float* oscale,
                                         int f16, const float* bias, const float* residual, float* y, void* y_hl, int B, int H,
                                         int W, int Cout, int ksize, int act, void* workspace, size_t workspace_bytes,
                                         ocv_stream_t stream) {
  OCV_CHECK_ARG(x_hl && w_hi && w_lo && (y || y_hl), "ocv_conv_nhwc_split_fwd: null pointer");
  OCV_CHECK_ARG(ocv_aligned16(y) && ocv_aligned16(y_hl) && ocv_aligned16(residual) && ocv_aligned16(workspace), "ocv_conv_nhwc_split_fwd: outputs, residual and workspace must be 16-byte aligned");
  OCV_CHECK_ARG(ksize == 1 || ksize == 3, "ocv_conv_nhwc_split_fwd: kernel size must be 1 or 3 (got %d)", ksize);
  OCV_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && Cout >= 1 && Cin >= 1, "ocv_conv_nhwc_split_fwd: bad sizes");
  OCV_CHECK_ARG(act >= 0 && act <= 3, "ocv_conv_nhwc_split_fwd: unknown activation %d", act);
  OCV_CHECK_ARG((reinterpret_cast<uintptr_t>(x_hl) & 127) == 0 && ocv_aligned16(w_hi) && ocv_aligned16(w_lo), "ocv_conv_nhwc_split_fwd: x_hl must be 128-byte aligned, weights 16-byte aligned");
  OCV_CHECK_ARG((long)B * H * W * (Cin + 32) * 4 < (1L << 32) && 9L * Cout * (Cin + 32) * 2 < (1L << 32), "ocv_conv_nhwc_split_fwd: each operand must be smaller than 4 GiB");
  OCV_CHECK_ARG(f16 == 0 || f16 == 1, "ocv_conv_nhwc_split_fwd: f16 must be 0 (bf16 pairs) or 1 (fp16 pairs)");
  bool use_halo = false;                          // dense 3 x 3: conv_halo_dma_kernel where forced, or where automatic picks it
  if (ksize == 3 && g_conv3x3_dispatch != 1) {
    const bool can = ocv_conv3x3_halo_supported(B, H, W, Cin, Cout) != 0;
    OCV_CHECK_ARG(can || g_conv3x3_dispatch != 2, "ocv_conv_nhwc_split_fwd: the halo-staged 3x3 kernel is forced (ocv_conv3x3_set_dispatch(2)) and cannot run B %d, %d x %d, %d -> %d channels (ocv_conv3x3_halo_supported: H %% 8 == 0, W %% 32 == 0, fewer than %d K steps)", B, H, W, Cin, Cout, KSPLIT_MIN_STEPS);
    use_halo = can && (g_conv3x3_dispatch == 2 || conv_halo_auto(B, H, W, Cin, Cout));
  }
  ConvArgs a{};
  const int zrc = fill_split_args(a, x_hl, Cin, w_hi, w_lo, oscale, f16, bias, residual, y, y_hl, B, H, W, Cout, ksize, act, (hipStream_t)stream);
  if (zrc != 0) return zrc;
  if (use_halo) {
    a.halo = 1;                                   // (supported: below the K length from which split-K is considered)
    return ocv_conv_launch(a, B, (hipStream_t)stream);
  }
  const long M = (long)B * H * W;
  const int ks = conv_ksplit(M, Cout, Cin, ksize);
  if (ks > 1 && workspace != nullptr && workspace_bytes >= (size_t)ks * M * Cout * sizeof(float)) {
    // two workgroups per tile, each over half of the channel chunks -> raw partial sums -> finish pass
    ConvArgs h = a;
    h.bias = nullptr; h.res = nullptr; h.yhl = nullptr; h.act = OCV_ACT_NONE; h.y = (float*)workspace; h.ksplit = ks; h.oscale = nullptr;
    const int rc = ocv_conv_launch(h, B, (hipStream_t)stream);
    if (rc != 0) return rc;
    FinArgs f{(const float*)workspace, bias, residual, y, (__bf16*)y_hl, M, M * Cout / 8, Cout, a.Cpo, act, ks, oscale, f16, a.range_flag};
    hipLaunchKernelGGL(conv_splitk_finish_kernel, dim3((unsigned)((f.items + 255) / 256)), dim3(256), 0, (hipStream_t)stream, f);
    OCV_CHECK_LAUNCH("ocv_conv_nhwc_split_fwd(finish)");
    return 0;
  }
  return ocv_conv_launch(a, B, (hipStream_t)stream);
}

// PACKED TAPS (round 6; ConvArgs::gpt): the same 3 x 3 convolution with the K axis = the nine taps' REAL 8-channel granules laid end
// to end.  Pays where Cin is far from a multiple of 32 -- the decoder's skip parts over 24 and 40 encoder channels (7 K steps instead
// of 9, 12 instead of 18): the matrix cores no longer multiply the zero pad channels of every tap.  w_hi / w_lo: ONE [Cout][Kp]
// matrix each, Kp = ocv_conv3x3_packed_taps_k(Cin), element (co, 8 (gpt t + g) + e) = weight[co][8 g + e][tap t] (zero where
// 8 g + e >= Cin, and beyond the ninth tap), split into pairs like the tap-major weights (hip_ops.prep_conv_weight_packed_taps).
extern "C" int ocv_conv3x3_packed_taps_k(int Cin) {
  if (Cin < 1 || Cin > 2040) return 0;
  const int gpt = (Cin + 7) / 8;
  return (9 * gpt + 3) / 4 * CBK;
}

extern "C" int ocv_conv3x3_split_packed_taps_fwd(const void* x_hl, int Cin, const void* w_hi, const void* w_lo, const float* oscale,
                                                 int f16, const float* bias, const float* residual, float* y, void* y_hl, int B,
                                                 int H, int W, int Cout, int act, ocv_stream_t stream) {
  OCV_CHECK_ARG(x_hl && w_hi && w_lo && (y || y_hl), "ocv_conv3x3_split_packed_taps_fwd: null pointer");
  OCV_CHECK_ARG(ocv_aligned16(y) && ocv_aligned16(y_hl) && ocv_aligned16(residual), "ocv_conv3x3_split_packed_taps_fwd: outputs and residual must be 16-byte aligned");
  OCV_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && Cout >= 1 && Cin >= 8 && Cin % 8 == 0 && Cin <= 2040,
                "ocv_conv3x3_split_packed_taps_fwd: bad sizes (Cin must be a multiple of 8 in [8, 2040], got %d)", Cin);
  OCV_CHECK_ARG(act >= 0 && act <= 3, "ocv_conv3x3_split_packed_taps_fwd: unknown activation %d", act);
  OCV_CHECK_ARG(f16 == 0 || f16 == 1, "ocv_conv3x3_split_packed_taps_fwd: f16 must be 0 (bf16 pairs) or 1 (fp16 pairs)");
  OCV_CHECK_ARG((reinterpret_cast<uintptr_t>(x_hl) & 127) == 0 && ocv_aligned16(w_hi) && ocv_aligned16(w_lo),
                "ocv_conv3x3_split_packed_taps_fwd: x_hl must be 128-byte aligned, weights 16-byte aligned");
  const int Kp = ocv_conv3x3_packed_taps_k(Cin), gpt = Cin / 8;
  OCV_CHECK_ARG((long)B * H * W * (Cin + 32) * 4 < (1L << 32) && (long)Cout * Kp * 2 < (1L << 32),
                "ocv_conv3x3_split_packed_taps_fwd: each operand must be smaller than 4 GiB");
  const int inv = (65536 + gpt - 1) / gpt;
  for (int G = 0; G < Kp / 8; ++G)
    OCV_CHECK_ARG((int)(((unsigned)G * (unsigned)inv) >> 16) == G / gpt, "ocv_conv3x3_split_packed_taps_fwd: internal (reciprocal of %d inexact at %d)", gpt, G);
  ConvArgs a{};
  const int zrc = fill_split_args(a, x_hl, Cin, w_hi, w_lo, oscale, f16, bias, residual, y, y_hl, B, H, W, Cout, 3, act, (hipStream_t)stream);
  if (zrc != 0) return zrc;
  a.gpt = gpt; a.gpt_inv = inv; a.Kp = Kp;
  return ocv_conv_launch(a, B, (hipStream_t)stream);
}

extern "C" int ocv_conv_nhwc_split_ws_fwd(const void* x_hl, int Cin, const void* w_hi, const void* w_lo, const float* bias,
                                          const float* residual, float* y, void* y_hl, int B, int H, int W, int Cout,
                                          int ksize, int act, void* workspace, size_t workspace_bytes, ocv_stream_t stream) {
  return ocv_conv_nhwc_split_x_fwd(x_hl, Cin, w_hi, w_lo, nullptr, 0, bias, residual, y, y_hl, B, H, W, Cout, ksize, act, workspace,
                                   workspace_bytes, stream);
}

extern "C" int ocv_conv_nhwc_split_fwd(const void* x_hl, int Cin, const void* w_hi, const void* w_lo, const float* bias,
                                       const float* residual, float* y, void* y_hl, int B, int H, int W, int Cout,
                                       int ksize, int act, ocv_stream_t stream) {
  return ocv_conv_nhwc_split_ws_fwd(x_hl, Cin, w_hi, w_lo, bias, residual, y, y_hl, B, H, W, Cout, ksize, act, nullptr, 0, stream);
}
